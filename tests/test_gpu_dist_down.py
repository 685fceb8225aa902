"""Downslope distance and HAND on the device (DEMProcessor.calc_dist_down / calc_hand, pydem_dist_down) against the reverse
Kahn reference of tests/test_dist_down_ref.py on the oracle's graphs, cell by cell:

    NaN patterns identical, |dev - ref| <= 1e-9 * refabs   (refabs: the same recursion with |cost|),

the bound tests/test_gpu_weighted_uca.py uses for re-associated sums on this graph.  Threshold targets are evaluated on the
device's own uca (that is the call's definition), so the reference gets `dp.uca >= threshold` as its mask.  Then: what the
call must leave alone, run-to-run identity and the memory it holds."""
import warnings

import numpy as np
import pytest

from flowgraph_kit import (_same_snapshot, _snapshot, _strips, assert_same_bits, circular_case, nan_speck_pair, pair, run_child,
                           shared_deep_pair as deep_pair, shared_fractal_pair as fractal_pair)
from test_dist_down_ref import KINDS, STATS, dist_down_ref

pytestmark = pytest.mark.gpu

BOUND = 1e-9
CELL = 900.0            # dX * dY of the fractal tiles


def compare(dev, o, target, kind, stat, what, min_finite=None):
    ref, final, depth = dist_down_ref(o, target, kind, stat)
    refabs = dist_down_ref(o, target, kind, stat, absolute=True)[0] if kind == 'v' else ref
    dev = np.asarray(dev, np.float64)
    nan_ref = np.isnan(ref)
    finite = 1.0 - nan_ref.mean()
    err = np.abs(dev[~nan_ref] - ref[~nan_ref])
    lim = BOUND * np.abs(refabs[~nan_ref])
    with np.errstate(invalid='ignore'):
        worst = float(np.nanmax(np.r_[0.0, err / np.maximum(np.abs(refabs[~nan_ref]), 1e-300)]))
    print("%s: %.1f %% targets, %.1f %% NaN, depth %d, %d cells not final, max %.4g, worst |dev - ref| / refabs %.3g"
          % (what, 100 * np.asarray(target).mean(), 100 * nan_ref.mean(), depth, (~final).sum(),
             np.nanmax(ref) if finite else np.nan, worst))
    if min_finite is not None:
        assert finite >= min_finite, "%s: only %.1f %% of the reference is finite" % (what, 100 * finite)
    assert np.array_equal(np.isnan(dev), nan_ref), "%s: NaN patterns differ (%d device, %d reference)" % (what, np.isnan(dev).sum(), nan_ref.sum())
    assert (err <= lim).all(), "%s: %d cells off, worst %.3g of the scale" % (what, (err > lim).sum(), worst)
    return ref, final, depth


FRACTALS = [((300, 260), 5), ((700, 520), 41), ((1024, 1024), 42)]


@pytest.mark.parametrize('cells', [50, 500])
@pytest.mark.parametrize('shape,seed', FRACTALS)
def test_fractal_tiles_distance_and_hand(shape, seed, cells):
    o, dp = fractal_pair(shape, seed)
    thr = cells * CELL
    target = np.asarray(dp.uca) >= thr
    d = dp.calc_dist_down(uca_threshold=thr)
    assert d is dp.dist_down and d.dtype == np.float64 and d.shape == shape
    _, final, depth = compare(d, o, target, 'h', 'ave', 'h/ave %r %d cells' % (shape, cells), min_finite=0.85)
    st = dp.dist_down_stats
    assert st['n_unresolved'] == (~final).sum() == 0 and 2 <= st['levels'] <= depth and st['ms'] > 0
    hand = dp.calc_hand(uca_threshold=thr)
    assert hand is dp.hand
    ref, _, _ = compare(hand, o, target, 'v', 'ave', 'HAND %r %d cells' % (shape, cells), min_finite=0.85)
    assert not (hand < 0).any() and np.nanmin(hand) == 0.0
    # the mask of the same cells is the same call
    again = dp.calc_dist_down(target=target, kind='v', stat='ave')
    assert np.array_equal(again.view(np.int64), hand.view(np.int64))


@pytest.mark.parametrize('cells', [50, 500])
@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('kind', KINDS)
def test_every_kind_and_statistic(kind, stat, cells):
    o, dp = fractal_pair(*FRACTALS[1])
    thr = cells * CELL
    target = np.asarray(dp.uca) >= thr
    d = dp.calc_dist_down(uca_threshold=thr, kind=kind, stat=stat)
    compare(d, o, target, kind, stat, '%s/%s %d cells' % (kind, stat, cells), min_finite=0.85)


@pytest.mark.parametrize('stat', STATS)
def test_deep_ramp_to_the_last_two_rows(stat):
    """a 900-row ramp with the target at its foot: the reverse depth is the tile's length, not a hillslope's"""
    o, dp = deep_pair()
    target = np.zeros(dp.shape, bool)
    target[-2:] = True
    d = dp.calc_dist_down(target=target, stat=stat)
    _, final, depth = compare(d, o, target, 'h', stat, 'deep ramp h/%s' % stat, min_finite=0.60)
    assert final.all() and depth >= 900
    st = dp.dist_down_stats
    assert 100 <= st['levels'] <= depth and st['n_unresolved'] == 0


@pytest.mark.parametrize('loop', ['two_cells', 'three_cells', 'two_loops'])
def test_circular_drainage_is_nan_and_counted(loop):
    o, dp = circular_case(loop)
    n, m = dp.shape
    target = np.zeros((n, m), bool)
    target[n - 1, m - 1] = True
    for kind, stat in (('h', 'ave'), ('s', 'min'), ('v', 'max')):
        with pytest.warns(UserWarning, match='circular drainage'):
            d = dp.calc_dist_down(target=target, kind=kind, stat=stat)
        _, final, _ = compare(d, o, target, kind, stat, '%s %s/%s' % (loop, kind, stat))
        assert (~final).sum() > 0 and dp.dist_down_stats['n_unresolved'] == (~final).sum()
        assert np.isnan(d[~final]).all() and d[n - 1, m - 1] == 0.0


def test_nan_specks():
    z, o, dp, _ = nan_speck_pair((640, 700), 40, [(0, 5), (639, 300), (200, 0)])
    uca = np.array(dp.uca)
    assert np.isnan(uca).any()
    thr = 200 * CELL
    target = uca >= thr
    assert not target[np.isnan(uca)].any()
    for kind in KINDS:
        d = dp.calc_dist_down(uca_threshold=thr, kind=kind)
        compare(d, o, target, kind, 'ave', 'NaN specks %s/ave' % kind, min_finite=0.5)
        assert np.isnan(d[np.isnan(z)]).all()


def test_row_varying_spacing():
    import capacity_terrain as CT
    from pydem_amd import synth
    n, m = 333, 290
    z = synth.fractal(n, m, seed=19, top_shift=7, n_octaves=7)
    dX, dY = CT.spacing(n, seed=4)
    sp = dict(dX=dX, dY=dY, dX2=np.r_[dX, dX[-1]] + 0.003, dY2=np.r_[dY[0], dY] - 0.007)
    o, dp = pair(z, **sp)
    thr = 150 * 25.0 * 31.0
    target = np.asarray(dp.uca) >= thr
    for kind, stat in (('h', 'ave'), ('s', 'ave'), ('h', 'max'), ('v', 'min')):
        d = dp.calc_dist_down(uca_threshold=thr, kind=kind, stat=stat)
        compare(d, o, target, kind, stat, 'row-varying spacing %s/%s' % (kind, stat), min_finite=0.7)


def test_bench_tile_8192():
    """the bench generator's 8192^2 tile, streams at 500 cells: cell ids, queue offsets and counts at a size where the frontier
    of one level is larger than a launch's grid"""
    from oracle import oracle as O
    from pydem_amd import DEMProcessor
    n = 8192
    z = O.synth_fractal(n, n, seed=1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o = O.OracleDEM(z, dX=30.0, dY=30.0, drain_pits=True)
        o.calc_uca()
        dp = DEMProcessor.from_synthetic((n, n), dict(seed=1), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
        dp.run_slopes_directions(); dp.run_uca()
    del z
    thr = 500 * CELL
    target = np.asarray(dp.uca) >= thr
    dp._host.pop('uca', None)
    d = dp.calc_dist_down(uca_threshold=thr)
    _, final, depth = compare(d, o, target, 'h', 'ave', 'h/ave 8192^2', min_finite=0.85)
    assert 2 <= dp.dist_down_stats['levels'] <= depth and dp.dist_down_stats['n_unresolved'] == (~final).sum()
    del d
    hand = dp.calc_hand(uca_threshold=thr)
    compare(hand, o, target, 'v', 'ave', 'HAND 8192^2', min_finite=0.85)


def check_schedules():
    """(child process) the cases that differ in what the tile passes and the queue each get to do"""
    o, dp = fractal_pair(*FRACTALS[1])
    target = np.asarray(dp.uca) >= 500 * CELL
    for kind, stat in (('h', 'ave'), ('v', 'ave'), ('s', 'max')):
        compare(dp.calc_dist_down(uca_threshold=500 * CELL, kind=kind, stat=stat), o, target, kind, stat, 'schedule %s/%s' % (kind, stat), 0.85)
    levels = [dp.dist_down_stats['levels']]
    o, dp = deep_pair()
    target = np.zeros(dp.shape, bool)
    target[-2:] = True
    compare(dp.calc_dist_down(target=target), o, target, 'h', 'ave', 'schedule deep ramp', 0.60)
    levels.append(dp.dist_down_stats['levels'])
    o, dp = circular_case('two_loops')
    target = np.zeros(dp.shape, bool)
    target[-1, -1] = True
    _, final, _ = compare(dp.calc_dist_down(target=target), o, target, 'h', 'ave', 'schedule two_loops')
    assert dp.dist_down_stats['n_unresolved'] == (~final).sum() > 0
    return levels


@pytest.mark.parametrize('env', [{'PYDEM_DIST_PASSES': '0'}, {'PYDEM_DIST_MIN_PER_VISIT': '0'}, {'PYDEM_DIST_PASSES': '2'}])
def test_schedules(env):
    """the queue alone, tile passes to the end, two passes then the queue (the switches are read once per process)"""
    r = run_child("from test_gpu_dist_down import check_schedules\nprint('LEVELS', check_schedules())\nprint('CHILD-OK')", env=env, timeout=300)
    levels = eval(r.stdout.split('LEVELS', 1)[1].splitlines()[0])
    if env.get('PYDEM_DIST_PASSES') == '0':
        assert levels == [70, 927], levels              # the queue alone runs the reference's levels
    if 'PYDEM_DIST_MIN_PER_VISIT' in env:
        assert levels[0] < 70 and levels[1] < 927, levels       # a pass finishes whole chains inside a tile, not one cell of each


def test_state_integrity():
    from pydem_amd import DEMProcessor, synth
    z = synth.fractal(520, 700, seed=11, top_shift=7, n_octaves=7)
    kw = dict(dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
    n, m = z.shape
    strips = _strips(n, m, 9)
    mask = np.zeros((n, m), bool)
    mask[-1, :] = True; mask[:, 0] = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        runs = []
        for with_dist in (True, False):
            dp = DEMProcessor(elev=z, **kw)
            dp.run_slopes_directions(); dp.run_uca(); dp.run_twi()
            dp.calc_weighted_uca(np.linspace(0.0, 2.0, n * m).reshape(n, m))
            if with_dist:
                before = _snapshot(dp)
                assert len(before[0]) == 11          # all twelve but the weights, which the weighted call consumed
                a = dp.calc_dist_down(uca_threshold=300 * CELL, kind='s', stat='max')
                b = dp.calc_hand(target=mask)
                assert np.isfinite(a).any() and np.isfinite(b).any() and not np.array_equal(a, b, equal_nan=True)
                _same_snapshot(before, _snapshot(dp))
                uca = np.array(dp.uca)
                assert_same_bits(dp.calc_weighted_uca(1.0), uca, 'w = 1 after the distance calls')
                dp.calc_dist_down(uca_threshold=300 * CELL)
            f0 = {k: np.array(getattr(dp, k)) for k in ('uca', 'edge_todo', 'edge_done')}
            dp.calc_uca(uca_init=f0['uca'], edge_init_data=strips)
            runs.append({k: np.array(getattr(dp, k)) for k in ('uca', 'edge_todo', 'edge_done')})
        for k in runs[0]:
            assert np.array_equal(runs[0][k], runs[1][k], equal_nan=True), k
        # ... and the distances still run on the tile's graph after the edge round
        d = dp.calc_dist_down(target=mask)
        assert np.isfinite(d).any()


def test_identical_calls_and_no_growth():
    from pydem_amd import _ffi
    o, dp = fractal_pair(*FRACTALS[1])
    thr = 500 * CELL
    first = dp.calc_dist_down(uca_threshold=thr, kind='s')          # (warm-up: the call's planes exist from here on)
    free0 = _ffi.device_memory(0)[0]
    for _ in range(20):
        again = dp.calc_dist_down(uca_threshold=thr, kind='s')
        assert again.tobytes() == first.tobytes()
    assert _ffi.device_memory(0)[0] >= free0


def test_no_graph_is_an_error():
    from pydem_amd import DEMProcessor, _ffi, synth
    z = synth.fractal(64, 80, seed=2, top_shift=5, n_octaves=5)
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.dist_down('h', 'ave', np.ones((64, 80), bool))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d = dp.calc_dist_down(target=np.ones((64, 80), bool))         # runs calc_uca first
    assert (d == 0).all() and dp._has('uca')
    dp._tile.upload(_ffi.ELEV, z + 1.0)                                # the elevation changed: the graph is gone
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.dist_down('h', 'ave', np.ones((64, 80), bool))
