"""Cost of the receiver-tree accumulation (pydem_tree_accum: cut at the link boundaries and over the whole tree, with and without
the edge rule) next to the plain forward accumulation on the resident bench tile, and of one calc_reach_attributes call.

    python tools/time_tree_accum.py [--size 16384] [--repeats 3] [--fraction 0.01] [--reach] [--out profiles/tree_accum_cost.txt]

Builds the tile like bench.py (DEMProcessor.from_synthetic, seed 0, dX = dY = 30 m, no conditioning), runs calc_uca once, takes
uca_threshold at the top `--fraction` of uca (the quantile of a seeded random sample of 2^22 cells), then for edge_nan on and off
runs pydem_tree_accum (op sum, load 1) cut by that threshold and over the whole tree, and in the same process the yardstick
calc_decay_accum(decay=None) -- pydem_fwd_accum without mult and cap: the same open set and visit rule, 20 B staged per slot
where this sweep stages 11 B -- each once cold and `--repeats` times warm, the result plane not downloaded.  The times are the
calls' own device times (hipEvent pairs: for the tree accumulation the two passes over the rows and the sweep); `crc` is a
checksum of the values gathered at 65536 seeded cells, the same at every switch point.  PYDEM_DIST_MIN_PER_VISIT=<n> replaces
TA_MIN_PER_VISIT (and the yardstick's FA_MIN_PER_VISIT) for the process, which is how the candidates are timed;
PYDEM_DIST_DEBUG=1 prints what each schedule finished.  --reach: one full calc_reach_attributes call on the same streams, wall
time and the device time of its sweeps.  Appends one JSON line to `--out` and prints it.
"""
import argparse
import json
import os
import sys
import time
import warnings
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--fraction', type=float, default=0.01)
    ap.add_argument('--reach', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tree_accum_cost.txt'))
    args = ap.parse_args()
    from pydem_amd import DEMProcessor
    warnings.simplefilter('ignore')
    n = args.size
    dp = DEMProcessor.from_synthetic((n, n), dict(seed=0), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    dp.run_uca()
    sweep_ms = dp.timings['sweep_ms']
    uca = np.asarray(dp.uca)
    sample = uca.ravel()[np.random.default_rng(0).integers(0, uca.size, 1 << 22)]
    thr = float(np.nanquantile(sample, 1.0 - args.fraction))
    with np.errstate(invalid='ignore'):
        fraction = float((uca >= thr).mean())
    dp._host.pop('uca', None)
    del uca
    out = {'size': n, 'sweep_ms': round(sweep_ms, 3), 'min_per_visit': os.environ.get('PYDEM_DIST_MIN_PER_VISIT', 'default'),
           'uca_threshold': thr, 'stream_fraction': round(fraction, 5)}
    ones = np.ones((n, n))
    at = np.random.default_rng(1).integers(0, n * n, 1 << 16)
    for edge_nan in (True, False):
        key = 'edge_nan' if edge_nan else 'plain'
        calls = (('cut', lambda: dp._tile.tree_accum(ones, 'sum', None, thr, edge_nan, at, download=False)),
                 ('whole', lambda: dp._tile.tree_accum(ones, 'sum', None, None, edge_nan, at, download=False)),
                 ('fwd_accum', lambda: dp._tile.fwd_accum(ones, None, None, edge_nan, download=False)))
        row = {}
        for name, f in calls:
            f()                                       # first call: allocates the planes, loads the kernels
            res = [f() for _ in range(args.repeats)]
            row[name] = dict(ms=[round(r[2], 3) for r in res], levels=res[-1][3], n_unresolved=res[-1][4])
            if name != 'fwd_accum':
                row[name]['crc'] = zlib.crc32(res[-1][1].tobytes())
        best = lambda k: min(row[k]['ms'])
        row['cut_over_fwd_accum'] = round(best('cut') / best('fwd_accum'), 3)
        row['whole_over_fwd_accum'] = round(best('whole') / best('fwd_accum'), 3)
        out[key] = row
    if args.reach:
        t0 = time.perf_counter()
        table = dp.calc_reach_attributes(uca_threshold=thr)
        wall = time.perf_counter() - t0
        st = dp.reach_attributes_stats
        out['reach_attributes'] = dict(wall_s=round(wall, 2), n_links=int(table.size), complete=int(table['complete'].sum()),
                                       stream_network_ms=[round(t, 3) for t in dp.stream_network_stats['ms']],
                                       sweeps_ms={k: round(v['ms'], 3) for k, v in st['sweeps'].items()}, sweeps_total_ms=round(st['ms'], 3))
    assert dp.timings['sweep_ms'] == sweep_ms
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
