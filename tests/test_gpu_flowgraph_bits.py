"""The bits of the three flow-graph sweeps (csrc/flowdist.h: calc_dist_down, calc_dist_up, calc_up_dependence / calc_rev_accum),
pinned: tests/golden/flowgraph_bits.json holds, per field and call, the sha256 of the result plane (its float64 bytes, NaNs
included: every NaN the sweeps store is the canonical one), the call's `levels` and its `n_unresolved`, recorded with the
library of the commit the file names.  A change to the sweeps' code that is meant to leave every result as it is -- a
refactor, a change of the visit protocol that finishes the same cells in the same passes -- must reproduce them; one that is
meant to change a result regenerates the file and says so:

    python tests/test_gpu_flowgraph_bits.py --write --commit <the commit whose library is loaded>

The fields are the designed ones of tests/flow_fields.py (chains over many tiles, 1024 rounds in one visit, two facet sections
over every tile edge and corner, pits with drains far away and around a tile corner, grids longer than the row kernels') and
the smallest fractal tile of tests/test_gpu_dist_down.py with its pits drained (cells with regular and pit out-edges, drains
with several pits).  The default schedule only: test_gpu_flow_fields.test_schedules holds the other three to its bits.  That
the values are RIGHT is the business of the cell-by-cell tests; this one only says they have not moved."""
import functools
import json
import os
import sys
import warnings

import numpy as np
import pytest

from flowgraph_kit import bits, random_weights

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'flowgraph_bits.json')
DESIGNED = ('row_snake', 'tile_snake', 'fan2', 'fan5', 'far_pit_rows', 'near_pit', 'tall', 'wide')
FRACTAL = 'fractal_300x260_seed5'
NAMES = DESIGNED + (FRACTAL,)
KINDS, STATS = ('h', 'v', 's'), ('ave', 'min', 'max')


def processor_and_target(name):
    """(DEMProcessor after calc_uca, target mask of the downslope calls and the dependence, load of racc / dmax)"""
    if name == FRACTAL:
        from pydem_amd import DEMProcessor, synth
        from test_gpu_dist_down import CELL, FRACTALS
        shape, seed = FRACTALS[0]
        assert name == 'fractal_%dx%d_seed%d' % (shape[0], shape[1], seed)
        z = synth.fractal(shape[0], shape[1], seed=seed, top_shift=7, n_octaves=7)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
            dp.calc_slopes_directions()
            dp.calc_uca()
        target = np.asarray(dp.uca) >= 50 * CELL             # the streams at 50 cells
        assert 0.01 < target.mean() < 0.5
    else:
        from test_gpu_flow_fields import FIELDS, processor
        field = FIELDS[name]()
        dp, target = processor(field), field.target
    return dp, target, random_weights(dp.shape, 7)


@functools.lru_cache(maxsize=None)
def results(name):
    """{call: [sha256, levels, n_unresolved]} of every call on the field, all on one processor"""
    dp, target, w = processor_and_target(name)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for kind in KINDS:
            for stat in STATS:
                d = dp.calc_dist_down(target=target, kind=kind, stat=stat)
                out['down %s/%s' % (kind, stat)] = [bits(d), dp.dist_down_stats['levels'], dp.dist_down_stats['n_unresolved']]
                for edge_nan in (False, True):
                    d = dp.calc_dist_up(kind=kind, stat=stat, edge_nan=edge_nan)
                    out['up %s/%s edge_nan=%d' % (kind, stat, edge_nan)] = [bits(d), dp.dist_up_stats['levels'], dp.dist_up_stats['n_unresolved']]
        d = dp.calc_up_dependence(target)
        out['dependence'] = [bits(d), dp.up_dependence_stats['levels'], dp.up_dependence_stats['n_unresolved']]
        racc, dmax = dp.calc_rev_accum(w)
        for key, d in (('sum', racc), ('max', dmax)):
            out['rev_accum %s' % key] = [bits(d), dp.rev_accum_stats[key]['levels'], dp.rev_accum_stats[key]['n_unresolved']]
    return {k: [v[0], int(v[1]), int(v[2])] for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_is_complete():
    g = golden()
    assert len(g['commit']) == 40 and sorted(g['fields']) == sorted(NAMES)
    for name in NAMES:
        assert len(g['fields'][name]) == 9 + 18 + 1 + 2, name
        assert all(len(v[0]) == 64 and v[1] >= 1 and v[2] >= 0 for v in g['fields'][name].values()), name


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_bits_levels_and_unresolved_are_the_recorded_ones(name):
    want, got = golden()['fields'][name], results(name)
    assert sorted(got) == sorted(want)
    moved = [k for k in sorted(want) if got[k][0] != want[k][0]]
    assert not moved, "%s: the result planes of %d calls differ from those of commit %s: %s" % (name, len(moved), golden()['commit'][:7], moved)
    passes = [(k, got[k][1:], want[k][1:]) for k in sorted(want) if got[k][1:] != want[k][1:]]
    assert not passes, "%s: (call, [levels, n_unresolved] now, recorded) %r" % (name, passes)


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--write', action='store_true', required=True)
    ap.add_argument('--commit', required=True, help='full hash of the commit the loaded library was built from')
    ap.add_argument('--out', default=GOLDEN)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    assert len(args.commit) == 40
    doc = dict(commit=args.commit, what='sha256 of the float64 bytes, levels, n_unresolved per field and call', fields={n: results(n) for n in NAMES})
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out, sum(len(v) for v in doc['fields'].values()), 'calls')
