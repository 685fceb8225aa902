"""The three sweeps of the flow-graph engine (csrc/flowdist.h: calc_dist_down, calc_dist_up, calc_up_dependence / calc_rev_accum)
on the designed fields of tests/flow_fields.py, which tests/test_flow_fields.py pins on the CPU: long chains that cross a tile
boundary in every row, 1024 rounds inside one tile visit, one facet section at a time over every tile edge and corner, a pit
whose drains lie two tiles away, chains longer than the grids of the row kernels.

Per field the device's edge set must be the oracle's (assert_edge_set_equals_oracle of tests/test_gpu_parity.py); then every call
is held cell by cell to its reference with the `compare` functions of test_gpu_dist_down / test_gpu_dist_up / test_gpu_rev_accum
and their bounds (NaN patterns identical, 1e-9 * refabs for the sums, bit for bit for the max recursion), the closed forms of the
chains hold, mirrored fans agree, every schedule (the queue alone, tile passes to the end, two passes then the queue) gives the
default schedule's bits, and nothing else on the tile has changed."""
import functools
import re
import warnings

import numpy as np
import pytest

import flow_fields as F
from flowgraph_kit import _same_snapshot, _snapshot, assert_bound, bits, random_weights, run_child
from test_dist_down_ref import KINDS, STATS, dist_down_ref
from test_dist_up_ref import dist_up_ref
from test_rev_accum_ref import rev_accum_ref

pytestmark = pytest.mark.gpu

FIELDS = dict([('row_snake', F.row_snake), ('tile_snake', F.tile_snake)]
              + [('fan%d' % k, functools.partial(F.fan, k)) for k in range(8)]
              + [('far_pit', F.far_pit), ('far_pit_rows', functools.partial(F.far_pit, True)), ('near_pit', F.near_pit),
                 ('tall', F.tall), ('wide', F.wide)]
              + [('fan%d_mirror' % k, functools.partial(F.fan, k, True)) for k in range(8)])
NAMES = [k for k in FIELDS if not k.endswith('_mirror')]
SNAKES = ('row_snake', 'tile_snake', 'tall', 'wide')
FAMILIES = ('row_snake', 'fan2', 'far_pit', 'tall')          # one field of each family


def processor(field):
    """the device processor on the field, after calc_uca"""
    from pydem_amd import DEMProcessor
    kw = dict(field.spacing, **field.options)
    if field.direction is not None:
        kw.update(mag=field.mag.copy(), direction=field.direction.copy(), flats=field.flats.copy())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor(elev=field.elev.copy(), fill_flats=False, drain_pits_path=False, **kw)
        if field.direction is None:
            dp.calc_slopes_directions()
        dp.calc_uca()
    return dp


@functools.lru_cache(maxsize=None)
def pair(name):
    """(oracle after calc_uca, DEMProcessor after calc_uca) on the field `name`, with the precondition of every test here: the
    device's edge set is the oracle's.  The tile's snapshot right after calc_uca is kept for test_state_is_unchanged."""
    from test_gpu_parity import assert_edge_set_equals_oracle
    field = FIELDS[name]()
    o, dp = F.oracle(field), processor(field)
    assert_edge_set_equals_oracle(o, dp)
    SNAPSHOTS[name] = _snapshot(dp)
    return o, dp


SNAPSHOTS = {}
DEPTHS = {}             # (field, call) -> depth of the reference, filled by whoever computes that reference first


def weights(name, seed=7):
    return random_weights(FIELDS[name]().elev.shape, seed)


def far_target(field):
    """the last row and the last column: on far_pit the drains of the pit are open at the start, unlike under `elev < 60`"""
    t = np.zeros(field.elev.shape, bool)
    t[-1, :] = True
    t[:, -1] = True
    return t


def depth_of(name, call):
    if (name, call) not in DEPTHS:
        field, o = FIELDS[name](), pair(name)[0]
        if call[0] == 'down':
            DEPTHS[name, call] = dist_down_ref(o, far_target(field) if call[3] == 'far' else field.target, call[1], call[2])[2]
        elif call[0] == 'up':
            DEPTHS[name, call] = dist_up_ref(o, call[1], call[2], call[3])[2]
        elif call[0] == 'dep':
            DEPTHS[name, call] = rev_accum_ref(o, 0, absorb=field.target)[2]
        else:
            DEPTHS[name, call] = rev_accum_ref(o, call[1], seed=weights(name))[2]
    return DEPTHS[name, call]


# ---- 1. cell by cell
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', NAMES)
def test_dist_down_cell_by_cell(name, kind):
    from test_gpu_dist_down import compare
    field = FIELDS[name]()
    o, dp = pair(name)
    for stat in STATS:
        d = dp.calc_dist_down(target=field.target, kind=kind, stat=stat)
        _, final, depth = compare(d, o, field.target, kind, stat, '%s down %s/%s' % (name, kind, stat), min_finite=0.5)
        DEPTHS[name, ('down', kind, stat, 'near')] = depth
        st = dp.dist_down_stats
        assert final.all() and st['n_unresolved'] == 0 and 1 <= st['levels'] <= depth


@pytest.mark.parametrize('edge_nan', [False, True])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', NAMES)
def test_dist_up_cell_by_cell(name, kind, edge_nan):
    from test_gpu_dist_up import compare
    o, dp = pair(name)
    for stat in STATS:
        d = dp.calc_dist_up(kind=kind, stat=stat, edge_nan=edge_nan)
        _, final, depth = compare(d, o, kind, stat, edge_nan, '%s up %s/%s edge_nan=%r' % (name, kind, stat, edge_nan),
                                  min_finite=None if edge_nan else 1.0)
        DEPTHS[name, ('up', kind, stat, edge_nan)] = depth
        st = dp.dist_up_stats
        assert final.all() and st['n_unresolved'] == 0 and 1 <= st['levels'] <= depth


@pytest.mark.parametrize('name', NAMES)
def test_dependence_and_rev_accum_cell_by_cell(name):
    from test_gpu_rev_accum import compare
    field = FIELDS[name]()
    o, dp = pair(name)
    dep = dp.calc_up_dependence(field.target)
    _, final, depth = compare(dep, o, 0, '%s dependence' % name, absorb=field.target)
    DEPTHS[name, ('dep',)] = depth
    assert final.all() and dp.up_dependence_stats['n_unresolved'] == 0 and 1 <= dp.up_dependence_stats['levels'] <= depth
    assert (dep[field.target] == 1.0).all() and (dep > 0).mean() >= 0.5
    w = weights(name)
    racc, dmax = dp.calc_rev_accum(w)
    _, final, DEPTHS[name, ('rev', 0)] = compare(racc, o, 0, '%s racc' % name, seed=w)
    _, _, DEPTHS[name, ('rev', 1)] = compare(dmax, o, 1, '%s dmax' % name, seed=w)
    assert final.all() and all(s['n_unresolved'] == 0 for s in dp.rev_accum_stats.values()) and (dmax >= w).all()


# ---- 2. closed forms
@pytest.mark.parametrize('name', SNAKES)
def test_closed_forms_on_the_chains(name):
    from test_flow_fields import chain_index
    field = FIELDS[name]()
    _, dp = pair(name)
    to_end, from_head = chain_index(field)
    count, dmax = dp.calc_rev_accum(1.0)
    assert np.array_equal(count, to_end), "%d cells do not hold the count of cells to their chain's end" % (count != to_end).sum()
    assert (dmax == 1.0).all()
    dep = dp.calc_up_dependence(field.target)
    assert (dep == 1.0).all(), "%d cells of a chain do not depend wholly on its last cell" % (dep != 1.0).sum()
    up = dp.calc_dist_up(kind='h', stat='max', edge_nan=False)
    assert np.isfinite(up).all() and (np.abs(up - from_head) <= 1e-9 * from_head).all()
    # ... and the same lengths counted from the other end
    down = dp.calc_dist_down(target=field.target, kind='h', stat='min')
    total = np.zeros(field.elev.shape)
    for p in field.facts['paths']:
        total[p[:, 0], p[:, 1]] = from_head[p[-1, 0], p[-1, 1]]
    assert (np.abs(down - (total - from_head)) <= 1e-9 * total).all()


# ---- 3. mirrored fans
@pytest.mark.parametrize('k', range(8))
def test_fans_agree_with_their_mirror_image(k):
    """a weight given to the wrong neighbour breaks this even if the reference shared the mistake"""
    o, dp = pair('fan%d' % k)
    _, dpm = pair('fan%d_mirror' % k)
    refabs = rev_accum_ref(o, 0, seed=1.0)[0]
    a, _ = dp.calc_rev_accum(1.0)
    b, _ = dpm.calc_rev_accum(1.0)
    assert a.max() > 10 and np.isfinite(a).all()
    bound, floor = 1e-9, 1e-300                  # (those of test_gpu_rev_accum's comparisons)
    assert_bound(a, b[:, ::-1], refabs, 'fan%d against its mirror image' % k, bound, floor)
    # the same for a load that is not symmetric itself
    w = weights('fan%d' % k, 11)
    a, am = dp.calc_rev_accum(w)
    b, bm = dpm.calc_rev_accum(np.ascontiguousarray(w[:, ::-1]))
    assert_bound(a, b[:, ::-1], rev_accum_ref(o, 0, seed=np.abs(w))[0], 'fan%d against its mirror image, random load' % k, bound, floor)
    assert np.array_equal(am, bm[:, ::-1])


# ---- 4. schedules
def schedule_calls(name):
    """the calls whose bits every schedule must reproduce: (call, function of the processor) pairs"""
    field = FIELDS[name]()
    w = weights(name)
    calls = [(('down', 'h', 'ave', 'near'), lambda dp: (dp.calc_dist_down(target=field.target, kind='h', stat='ave'), dp.dist_down_stats)),
             (('down', 's', 'max', 'near'), lambda dp: (dp.calc_dist_down(target=field.target, kind='s', stat='max'), dp.dist_down_stats)),
             (('up', 'h', 'max', False), lambda dp: (dp.calc_dist_up(kind='h', stat='max', edge_nan=False), dp.dist_up_stats)),
             (('up', 'v', 'ave', True), lambda dp: (dp.calc_dist_up(kind='v', stat='ave', edge_nan=True), dp.dist_up_stats)),
             (('dep',), lambda dp: (dp.calc_up_dependence(field.target), dp.up_dependence_stats)),
             (('rev', 0), lambda dp: (dp.calc_rev_accum(w)[0], dp.rev_accum_stats['sum'])),
             (('rev', 1), lambda dp: (dp.calc_rev_accum(w)[1], dp.rev_accum_stats['max']))]
    if name.startswith('far_pit'):
        far = far_target(field)
        calls.append((('down', 'v', 'min', 'far'), lambda dp: (dp.calc_dist_down(target=far, kind='v', stat='min'), dp.dist_down_stats)))
    return calls


def schedule_results(make=None, keep=()):
    """{(field, call): (sha256 of the result, levels, unresolved cells)} for every field; `keep`: fields whose arrays are
    returned too.  A child process makes its own processors (it needs no oracle)."""
    import sys
    out, arrays = {}, {}
    for name in NAMES:
        dp = make(name) if make else processor(FIELDS[name]())
        for call, run in schedule_calls(name):
            sys.stderr.write('--- %s %r\n' % (name, call))
            sys.stderr.flush()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                d, st = run(dp)
            out[name, call] = (bits(d), st['levels'], st['n_unresolved'])
            if name in keep:
                arrays[name, call] = d
    return (out, arrays) if keep else out


@functools.lru_cache(maxsize=None)
def default_schedule():
    return schedule_results(lambda name: pair(name)[1], keep=('far_pit', 'far_pit_rows'))


def test_far_pit_is_finished_by_the_default_schedule():
    """the pit's drains lie two tiles from it, out of the visit rule's sight: the passes stall and the queue finishes the basin"""
    from test_gpu_dist_down import compare as compare_down
    from test_gpu_rev_accum import compare as compare_rev
    here, arrays = default_schedule()
    for name in ('far_pit', 'far_pit_rows'):
        field, (o, _) = FIELDS[name](), pair(name)
        basin = np.s_[:67, :67]
        assert all(v[2] == 0 for k, v in here.items() if k[0] == name)
        d = arrays[name, ('down', 'v', 'min', 'far')]
        ref, final, DEPTHS[name, ('down', 'v', 'min', 'far')] = compare_down(d, o, far_target(field), 'v', 'min', name + ' far target')
        assert final.all() and np.isfinite(ref[basin]).all() and np.isfinite(d[basin]).all() and np.isfinite(d[16, 16])
        ref, final, _ = compare_rev(arrays[name, ('rev', 0)], o, 0, name + ' racc', seed=weights(name))
        assert final.all() and np.isfinite(arrays[name, ('rev', 0)][basin]).all()
        assert np.isfinite(arrays[name, ('up', 'h', 'max', False)]).all()


@pytest.mark.parametrize('env', [{'PYDEM_DIST_PASSES': '0'}, {'PYDEM_DIST_MIN_PER_VISIT': '0'}, {'PYDEM_DIST_PASSES': '2'}])
def test_schedules(env):
    """the queue alone, tile passes to the end, two passes then the queue (the switches are read once per process: a fresh child
    each, one GPU process at a time): the bits of the default schedule, which the other tests hold to the references"""
    here, _ = default_schedule()
    r = run_child("from test_gpu_flow_fields import schedule_results\nprint('RESULTS', schedule_results())\nprint('CHILD-OK')",
                  env=dict(env, PYDEM_DIST_DEBUG='1'), timeout=300)
    there = eval(r.stdout.split('RESULTS', 1)[1].splitlines()[0])
    assert sorted(there) == sorted(here)
    differ = [k for k in here if there[k][0] != here[k][0] or there[k][2] != here[k][2]]
    assert not differ, differ
    # what the schedule got to do: "<what>: <open> open cells, <visits> tile visits finished <cells>, queue: <levels> levels, ..."
    log = {}
    for block in r.stderr.split('--- ')[1:]:
        head = block.splitlines()[0]
        name, call = head.split(' ', 1)
        mt = re.findall(r': (\d+) open cells, (\d+) tile visits finished (\d+), queue: (\d+) levels, (\d+) cells', block)
        call = eval(call)
        log[name, call] = tuple(int(x) for x in (mt[0] if call == ('rev', 0) else mt[-1]))     # (calc_rev_accum: the sum, then the max)
    for (name, call), (_, levels, left) in there.items():
        n_open, visits, by_passes, qlevels, qcells = log[name, call]
        field = FIELDS[name]()
        chain_intact = not (call[0] == 'up' and call[3])              # (edge_nan cuts a chain wherever it touches the border)
        if env.get('PYDEM_DIST_PASSES') == '0':
            assert visits == 0 and by_passes == 0 and qcells == n_open - left
            assert levels == depth_of(name, call), (name, call, levels, depth_of(name, call))
        elif 'PYDEM_DIST_MIN_PER_VISIT' in env:
            if name in ('row_snake', 'tall') and chain_intact:
                # a path advances one tile per pass
                assert field.facts['crossings'] <= levels <= field.facts['depth'], (name, call, levels)
                assert qlevels == 0 and by_passes == n_open
            if name == 'tile_snake' and chain_intact:
                # one visit finishes a whole block: 1024 rounds
                assert levels < field.facts['depth'] / 100, (name, call, levels)
                assert qlevels == 0 and by_passes == n_open
            if name.startswith('far_pit'):
                assert left == 0
                if call in (('rev', 0), ('rev', 1), ('up', 'h', 'max', False), ('down', 'v', 'min', 'far')):
                    assert visits > 0 and qlevels > 0 and qcells > 0, (name, call, log[name, call])     # stall, then the queue
        else:
            assert visits > 0


# ---- 5. state
@pytest.mark.parametrize('name', FAMILIES)
def test_state_is_unchanged(name):
    """fields, graph words, pit lists and timings of the tile are those calc_uca left, after every call above"""
    _, dp = pair(name)
    before = SNAPSHOTS[name]
    assert len(before[0]) >= 6 and before[1].size == dp.shape[0] * dp.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for _, run in schedule_calls(name):
            run(dp)
    _same_snapshot(before, _snapshot(dp))
