"""Upslope dependence, watersheds and reverse accumulation on the device (DEMProcessor.calc_up_dependence / calc_watershed /
calc_rev_accum, pydem_rev_accum) against the reverse Kahn reference of tests/test_rev_accum_ref.py on the oracle's graphs,
cell by cell:

    NaN patterns identical,  op 0: |dev - ref| <= 1e-9 * refabs + 1e-300,  op 1: bit for bit

(refabs: the same recursion with |seed|; 1e-9 is the bound tests/test_gpu_weighted_uca.py uses for re-associated sums on this
graph; the floor covers subnormal products; a max rounds nothing).  The tiles are the smallest that reach every path: (70, 45)
is 3 x 2 blocks of 32 x 32, both ragged; (96, 80) 3 x 3; (160, 130) 5 x 5 with a 2-column sliver and some 600 pit edges.
Then: the duality with the device's own uca, the schedules, what the call must leave alone, run-to-run identity, memory."""
import warnings

import numpy as np
import pytest

from flowgraph_kit import (_same_snapshot, _snapshot, assert_bound, assert_same_bits, circular_case, deep_pair, fractal_pair as make,
                           nan_speck_pair, random_weights, run_child, shared_fractal_pair as fractal_pair)
from test_rev_accum_ref import OUTLETS, rev_accum_ref

pytestmark = pytest.mark.gpu

BOUND = 1e-9
FLOOR = 1e-300
CELL = 900.0            # dX * dY of the fractal tiles
TILES = [(shape, seed) for shape, seed, _ in OUTLETS]


def compare(dev, o, op, what, seed=None, absorb=None, absorb_value=1.0):
    ref, final, depth = rev_accum_ref(o, op, seed, absorb, absorb_value)
    if op == 1:
        assert_same_bits(dev, ref, what)
    else:
        assert_bound(dev, ref, rev_accum_ref(o, op, seed, absorb, absorb_value, absolute=True)[0], what, BOUND, FLOOR)
    return ref, final, depth


# ---- 1. dependence on stream targets
def check_dependence(o, dp, cells):
    shape = tuple(dp.shape)
    target = np.asarray(dp.uca) >= cells * CELL
    dep = dp.calc_up_dependence(target)
    assert dep is dp.up_dependence and dep.dtype == np.float64 and dep.shape == shape
    _, final, depth = compare(dep, o, 0, 'dependence %r %d cells' % (shape, cells), absorb=target)
    st = dp.up_dependence_stats
    assert st['n_unresolved'] == (~final).sum() == 0 and st['levels'] >= 2 and st['ms'] > 0
    inside, partial = np.mean(dep > 0), np.mean((dep > 0) & (dep < 1))
    print("%r %d cells: %.1f %% targets, %.1f %% with dep > 0, %.1f %% partial, depth %d, levels %d"
          % (shape, cells, 100 * target.mean(), 100 * inside, 100 * partial, depth, st['levels']))
    assert inside >= 0.8 and partial >= 0.02
    assert np.nanmax(dep) <= 1.0 + 1e-12 and np.nanmin(dep) >= 0.0 and (dep[target] == 1.0).all()
    return target, st['levels'], depth


@pytest.mark.parametrize('cells', [20, 100])
@pytest.mark.parametrize('shape,seed', TILES)
def test_dependence_on_stream_targets(shape, seed, cells):
    o, dp = fractal_pair(shape, seed)
    check_dependence(o, dp, cells)


# ---- 2. duality with the device's own forward sweep
@pytest.mark.parametrize('shape,seed,outlet', OUTLETS)
def test_dependence_is_dual_to_the_devices_uca(shape, seed, outlet):
    o, dp = fractal_pair(shape, seed)
    ws = dp.calc_watershed([outlet])
    dep = dp.up_dependence
    assert ws is dp.watershed and ws.dtype == bool and ws.shape == shape
    assert np.array_equal(ws, dep > 0) and ws[outlet] and dep[outlet] == 1.0
    total = float(np.nansum(dep * (dp.dX2 * dp.dY2)[:, None]))
    want = float(np.asarray(dp.uca)[outlet])
    print("%r outlet %r: sum of area x dep %.17g, uca %.17g, relative difference %.3g" % (shape, outlet, total, want, abs(total - want) / want))
    assert not np.isnan(dep).any() and abs(total - want) <= 1e-9 * want
    absorb = np.zeros(shape, bool)
    absorb[outlet] = True
    ref, _, _ = compare(dep, o, 0, 'one outlet %r' % (shape,), absorb=absorb)
    assert ws.sum() == (ref > 0).sum() >= 300
    # a mask of the same cell is the same call, and a fraction thins the watershed
    again = dp.calc_watershed(absorb, min_fraction=0.5)
    assert np.array_equal(again, dep > 0.5) and again[outlet] and again.sum() < ws.sum()
    assert dp.up_dependence.tobytes() == dep.tobytes()


# ---- 3. reverse accumulation of random loads
@pytest.mark.parametrize('shape,seed', TILES)
def test_rev_accum_random_weights(shape, seed):
    o, dp = fractal_pair(shape, seed)
    w1, w2 = random_weights(shape, seed), random_weights(shape, seed + 1)
    r1, m1 = dp.calc_rev_accum(w1)
    assert r1 is dp.rev_accum and m1 is dp.rev_accum_max and r1.shape == m1.shape == shape
    assert set(dp.rev_accum_stats) == {'sum', 'max'} and all(s['n_unresolved'] == 0 and s['levels'] >= 2 for s in dp.rev_accum_stats.values())
    _, final, _ = compare(r1, o, 0, 'racc %r' % (shape,), seed=w1)
    compare(m1, o, 1, 'dmax %r' % (shape,), seed=w1)
    assert final.all() and (m1 >= w1).all()
    r2, _ = dp.calc_rev_accum(w2)
    r12, m12 = dp.calc_rev_accum(w1 + w2)
    compare(m12, o, 1, 'dmax of the sum %r' % (shape,), seed=w1 + w2)
    assert_bound(r12, r1 + r2, rev_accum_ref(o, 0, seed=np.abs(w1) + np.abs(w2))[0], 'linearity %r' % (shape,), BOUND, FLOOR)
    r0, m0 = dp.calc_rev_accum(0.0)
    assert (r0 == 0.0).all() and (m0 == 0.0).all()


# ---- 4. deep chain
def check_deep():
    o, dp = deep_pair((200, 48))
    target = np.zeros(dp.shape, bool)
    target[-2:] = True
    dep = dp.calc_up_dependence(target)
    _, final, depth = compare(dep, o, 0, 'deep ramp', absorb=target)
    st = dp.up_dependence_stats
    print("deep ramp: depth %d, levels %d" % (depth, st['levels']))
    assert final.all() and depth >= 200 and st['levels'] >= 20 and st['n_unresolved'] == 0
    racc, dmax = dp.calc_rev_accum(np.arange(dep.size, dtype=np.float64).reshape(dep.shape) % 7 - 2.0)
    compare(racc, o, 0, 'deep ramp racc', seed=np.arange(dep.size, dtype=np.float64).reshape(dep.shape) % 7 - 2.0)
    compare(dmax, o, 1, 'deep ramp dmax', seed=np.arange(dep.size, dtype=np.float64).reshape(dep.shape) % 7 - 2.0)
    return dp, target, st['levels'], depth


def test_deep_chain():
    check_deep()


# ---- 5. circular drainage
def check_circular(loop):
    o, dp = circular_case(loop)
    n, m = dp.shape
    absorb = np.zeros((n, m), bool)
    absorb[n - 1, m - 1] = True
    with pytest.warns(UserWarning, match='circular drainage'):
        dep = dp.calc_up_dependence(absorb)
    _, final, _ = compare(dep, o, 0, loop + ' dependence', absorb=absorb)
    assert (~final).sum() > 0 and dp.up_dependence_stats['n_unresolved'] == (~final).sum()
    assert np.isnan(dep[~final]).all() and dep[n - 1, m - 1] == 1.0
    w = np.linspace(-1.0, 2.0, n * m).reshape(n, m)
    with pytest.warns(UserWarning, match='circular drainage'):
        racc, dmax = dp.calc_rev_accum(w)
    _, final, _ = compare(racc, o, 0, loop + ' racc', seed=w)
    compare(dmax, o, 1, loop + ' dmax', seed=w)
    assert all(s['n_unresolved'] == (~final).sum() > 0 for s in dp.rev_accum_stats.values())
    # the low-level call with another absorb value: the cell keeps it
    out, _, _, left = dp._tile.rev_accum('max', w, absorb, 3.5)
    compare(out, o, 1, loop + ' max with an absorbing cell', seed=w, absorb=absorb, absorb_value=3.5)
    assert out[n - 1, m - 1] == 3.5 and left == (~rev_accum_ref(o, 1, w, absorb, 3.5)[1]).sum()


@pytest.mark.parametrize('loop', ['two_cells', 'three_cells', 'two_loops'])
def test_circular_drainage_is_nan_and_counted(loop):
    check_circular(loop)


# ---- 6. NaN specks
def test_nan_specks():
    n, m = 96, 80
    z, o, dp, rng = nan_speck_pair((n, m), 12, [(0, 5), (95, 30), (20, 0)])
    uca = np.array(dp.uca)
    nodata = np.isnan(z)
    assert 13 <= nodata.sum() <= 15
    target = uca >= 50 * CELL
    dep = dp.calc_up_dependence(target)
    _, final, _ = compare(dep, o, 0, 'NaN specks dependence', absorb=target)
    assert final.all() and np.array_equal(np.isnan(dep), nodata)
    w = rng.uniform(-1.0, 2.0, (n, m))
    racc, dmax = dp.calc_rev_accum(w)
    compare(racc, o, 0, 'NaN specks racc', seed=w)
    compare(dmax, o, 1, 'NaN specks dmax', seed=w)
    assert np.array_equal(np.isnan(racc), nodata) and np.array_equal(np.isnan(dmax), nodata)
    # an absorbing mask over a no-data cell does not revive it
    out, _, _, _ = dp._tile.rev_accum('sum', None, np.ones((n, m), bool), 1.0)
    assert np.array_equal(np.isnan(out), nodata) and (out[~nodata] == 1.0).all()


# ---- 7. schedules
def check_schedules():
    """(child process) the cases that differ in what the tile passes and the queue each get to do; for the fractal tile and the
    deep chain: (levels of the dependence call, levels of pydem_dist_down h/ave with the same mask, depth of the reference)"""
    o, dp = fractal_pair(*TILES[0])
    target, levels, depth = check_dependence(o, dp, 20)
    dp.calc_dist_down(target=target)
    out = [(levels, dp.dist_down_stats['levels'], depth)]
    dp, target, levels, depth = check_deep()
    dp.calc_dist_down(target=target)
    out.append((levels, dp.dist_down_stats['levels'], depth))
    check_circular('two_loops')
    return out


@pytest.mark.parametrize('env', [{'PYDEM_DIST_PASSES': '0'}, {'PYDEM_DIST_MIN_PER_VISIT': '0'}, {'PYDEM_DIST_PASSES': '2'}])
def test_schedules(env):
    """the queue alone, tile passes to the end, two passes then the queue (the switches are read once per process)"""
    r = run_child("from test_gpu_rev_accum import check_schedules\nprint('LEVELS', check_schedules())\nprint('CHILD-OK')", env=env, timeout=300)
    (lv, lv_down, depth), (deep, deep_down, deep_depth) = eval(r.stdout.split('LEVELS', 1)[1].splitlines()[0])
    print(env, (lv, lv_down, depth), (deep, deep_down, deep_depth))
    if env.get('PYDEM_DIST_PASSES') == '0':
        # the same open set, the same edges, the same queue: the levels of the distance, which are the reference's
        assert lv == lv_down == depth and deep == deep_down == deep_depth
    if 'PYDEM_DIST_MIN_PER_VISIT' in env:
        assert deep < deep_depth                        # a pass finishes whole chains inside a tile, not one cell of each


# ---- 8. state integrity
def test_state_integrity():
    from test_gpu_dist_down import compare as compare_dist
    shape, seed = TILES[0]
    o, dp = make(shape, seed)                           # (a pair of this test's own: it adds fields to the tile)
    n, m = shape
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp.run_twi()
        dp.calc_weighted_uca(np.linspace(0.0, 2.0, n * m).reshape(n, m))
        uca = np.array(dp.uca)
        target = uca >= 20 * CELL
        before = _snapshot(dp)
        assert len(before[0]) == 11                     # all twelve but the weights, which the weighted call consumed
        dep = dp.calc_up_dependence(target)
        racc, dmax = dp.calc_rev_accum(random_weights(shape, 3))
        assert np.isfinite(dep).any() and not np.array_equal(dep, racc, equal_nan=True) and not np.array_equal(racc, dmax, equal_nan=True)
        _same_snapshot(before, _snapshot(dp))
        assert_same_bits(dp.calc_weighted_uca(1.0), uca, 'w = 1 after the reverse accumulation')
        # the calls share their planes: each still matches its reference after the other
        compare_dist(dp.calc_dist_down(target=target), o, target, 'h', 'ave', 'dist_down after up_dependence')
        compare(dp.calc_up_dependence(target), o, 0, 'up_dependence after dist_down', absorb=target)
        compare_dist(dp.calc_dist_down(uca_threshold=20 * CELL, kind='s', stat='max'), o, target, 's', 'max', 'dist_down after up_dependence, threshold')
        up = dp.calc_dist_up(edge_nan=False)
        compare(dp.calc_rev_accum(1.0)[1], o, 1, 'dmax after dist_up', seed=np.ones(shape))
        assert np.array_equal(dp.calc_dist_up(edge_nan=False), up, equal_nan=True)


# ---- 9. repeatability and memory
def test_identical_calls_and_no_growth():
    from pydem_amd import _ffi
    shape, seed = TILES[1]
    o, dp = fractal_pair(shape, seed)
    target = np.asarray(dp.uca) >= 100 * CELL
    w = random_weights(shape, 9)
    first = dp.calc_up_dependence(target), dp.calc_rev_accum(w)     # (warm-up: the call's planes, the seed's included, exist from here on)
    free0 = _ffi.device_memory(0)[0]
    for _ in range(20):
        assert dp.calc_up_dependence(target).tobytes() == first[0].tobytes()
        racc, dmax = dp.calc_rev_accum(w)
        assert racc.tobytes() == first[1][0].tobytes() and dmax.tobytes() == first[1][1].tobytes()
    assert _ffi.device_memory(0)[0] >= free0


# ---- 10. errors
def test_errors():
    from pydem_amd import DEMProcessor, _ffi, synth
    z = synth.fractal(64, 80, seed=2, top_shift=5, n_octaves=5)
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    everything = np.ones((64, 80), bool)
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.rev_accum('sum', None, everything)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d = dp.calc_up_dependence(everything)                             # runs calc_uca first
    assert (d == 1.0).all() and dp._has('uca')
    with pytest.raises(_ffi.HipError, match='error -2'):
        dp._tile.rev_accum('max', None, everything)                       # op 1 without a seed
    with pytest.raises(_ffi.HipError, match='error -2'):
        dp._tile.rev_accum(2, np.zeros((64, 80)))
    for bad in (np.nan, np.inf):
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp._tile.rev_accum('sum', None, everything, bad)
    assert dp.calc_up_dependence(everything).tobytes() == d.tobytes()     # the refused calls left the state alone
    dp._tile.upload(_ffi.ELEV, z + 1.0)                                   # the elevation changed: the graph is gone
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.rev_accum('sum', None, everything)
