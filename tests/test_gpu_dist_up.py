"""Upslope flow-path distance on the device (DEMProcessor.calc_dist_up, pydem_dist_up) against the forward Kahn reference of
tests/test_dist_up_ref.py on the oracle's graphs, cell by cell:

    NaN patterns identical, |dev - ref| <= 1e-9 * refabs   (refabs: the same recursion with |cost| for kind 'v'),

the bound and the form of tests/test_gpu_dist_down.py.  Then the schedules (bit-identical), what the call must leave alone,
run-to-run identity and the memory it holds."""
import functools
import warnings

import numpy as np
import pytest

from flowgraph_kit import (_same_snapshot, _snapshot, bits, circular_case, nan_speck_pair, pair, run_child, shared_deep_pair as deep_pair,
                           shared_fractal_pair as fractal_pair)
from test_dist_down_ref import KINDS, STATS
from test_dist_up_ref import dist_up_ref, edge_nan_cells

pytestmark = pytest.mark.gpu

BOUND = 1e-9


def compare(dev, o, kind, stat, edge_nan, what, min_finite=None):
    ref, final, depth = dist_up_ref(o, kind, stat, edge_nan)
    refabs = dist_up_ref(o, kind, stat, edge_nan, absolute=True)[0] if kind == 'v' else ref
    dev = np.asarray(dev, np.float64)
    nan_ref = np.isnan(ref)
    finite = 1.0 - nan_ref.mean()
    err = np.abs(dev[~nan_ref] - ref[~nan_ref])
    lim = BOUND * np.abs(refabs[~nan_ref])
    with np.errstate(invalid='ignore'):
        worst = float(np.nanmax(np.r_[0.0, err / np.maximum(np.abs(refabs[~nan_ref]), 1e-300)]))
    print("%s: %.1f %% finite, depth %d, %d cells not final, max %.4g, worst |dev - ref| / refabs %.3g"
          % (what, 100 * finite, depth, (~final).sum(), np.nanmax(ref) if finite else np.nan, worst))
    if min_finite is not None:
        assert finite >= min_finite, "%s: only %.1f %% of the reference is finite" % (what, 100 * finite)
    assert np.array_equal(np.isnan(dev), nan_ref), "%s: NaN patterns differ (%d device, %d reference)" % (what, np.isnan(dev).sum(), nan_ref.sum())
    assert (err <= lim).all(), "%s: %d cells off, worst %.3g of the scale" % (what, (err > lim).sum(), worst)
    return ref, final, depth


FRACTALS = [((300, 260), 5), ((700, 520), 41), ((1024, 1024), 42)]


@pytest.mark.parametrize('edge_nan', [True, False])
@pytest.mark.parametrize('shape,seed', FRACTALS)
def test_fractal_tiles_longest_flow_path(shape, seed, edge_nan):
    o, dp = fractal_pair(shape, seed)
    d = dp.calc_dist_up(edge_nan=edge_nan)                # h / max
    assert d is dp.dist_up and d.dtype == np.float64 and d.shape == shape
    _, final, depth = compare(d, o, 'h', 'max', edge_nan, 'h/max %r edge_nan=%r' % (shape, edge_nan), min_finite=0.90 if edge_nan else 1.0)
    if not edge_nan:
        assert np.array_equal(np.isfinite(d), np.isfinite(o.elev))
    st = dp.dist_up_stats
    assert st['n_unresolved'] == (~final).sum() == 0 and 2 <= st['levels'] <= depth and st['ms'] > 0
    assert (st['kind'], st['stat'], st['edge_nan']) == ('h', 'max', edge_nan)
    assert not (d < 0).any() and np.nanmax(d) > 30.0 * 20


@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('kind', KINDS)
def test_every_kind_and_statistic(kind, stat):
    o, dp = fractal_pair(*FRACTALS[1])
    d = dp.calc_dist_up(kind=kind, stat=stat, edge_nan=True)
    compare(d, o, kind, stat, True, '%s/%s' % (kind, stat), min_finite=0.90)


@functools.lru_cache(maxsize=None)
def deep_ramp_depth():
    return dist_up_ref(deep_pair()[0], 'h', 'max', False)[2]


@pytest.mark.parametrize('stat', STATS)
def test_deep_ramp(stat):
    """a 900-row ramp: the forward depth is the tile's length, not a hillslope's"""
    o, dp = deep_pair()
    d = dp.calc_dist_up(stat=stat, edge_nan=False)
    _, final, depth = compare(d, o, 'h', stat, False, 'deep ramp h/%s' % stat, min_finite=1.0)
    assert final.all() and depth >= 900
    st = dp.dist_up_stats
    assert 100 <= st['levels'] <= depth and st['n_unresolved'] == 0


@pytest.mark.parametrize('loop', ['two_cells', 'three_cells', 'two_loops'])
def test_circular_drainage_is_nan_and_counted(loop):
    o, dp = circular_case(loop)
    indptr, indices, _ = o.A
    src = np.repeat(np.arange(dp.shape[0] * dp.shape[1]), np.diff(indptr))
    for kind, stat, edge_nan in (('h', 'max', False), ('s', 'ave', False), ('v', 'min', True), ('h', 'max', True)):
        with pytest.warns(UserWarning, match='circular drainage'):
            d = dp.calc_dist_up(kind=kind, stat=stat, edge_nan=edge_nan)
        _, final, _ = compare(d, o, kind, stat, edge_nan, '%s %s/%s edge_nan=%r' % (loop, kind, stat, edge_nan))
        assert (~final).sum() >= 2 and dp.dist_up_stats['n_unresolved'] == (~final).sum()
        assert np.isnan(d[~final]).all()
        # the loop cells and everything downstream: NaN flows along every edge
        assert np.isnan(d.ravel()[indices[np.isnan(d.ravel()[src])]]).all()
        if not edge_nan:
            assert np.isfinite(d[final]).all()


def test_nan_specks():
    z, o, dp, _ = nan_speck_pair((640, 700), 40, [(0, 5), (639, 300), (200, 0)])
    assert np.isnan(np.asarray(dp.uca)).any()
    for edge_nan in (False, True):
        for kind, stat in (('h', 'max'), ('v', 'ave')):
            d = dp.calc_dist_up(kind=kind, stat=stat, edge_nan=edge_nan)
            compare(d, o, kind, stat, edge_nan, 'NaN specks %s/%s edge_nan=%r' % (kind, stat, edge_nan), min_finite=0.5)
            assert np.isnan(d[np.isnan(z)]).all()
            if edge_nan:
                assert np.isnan(d[edge_nan_cells(z)]).all()
            else:
                assert np.array_equal(np.isnan(d), np.isnan(z))


@pytest.mark.parametrize('shape', [(3, 7), (7, 3), (31, 33), (33, 65)])
def test_small_ramps(shape):
    """tiles smaller than one 32 x 32 block, and one cell more than a block in each direction"""
    n, m = shape
    z = -np.tile(np.arange(m, dtype=np.float64), (n, 1)) + 0.01 * np.arange(n, dtype=np.float64)[:, None]
    o, dp = pair(z, dX=2.0, dY=3.0)
    for kind, stat in (('h', 'max'), ('s', 'ave'), ('v', 'min')):
        for edge_nan in (False, True):
            d = dp.calc_dist_up(kind=kind, stat=stat, edge_nan=edge_nan)
            _, final, depth = compare(d, o, kind, stat, edge_nan, 'ramp %r %s/%s edge_nan=%r' % (shape, kind, stat, edge_nan))
            assert final.all() and dp.dist_up_stats['n_unresolved'] == 0 and 1 <= dp.dist_up_stats['levels'] <= depth
            if edge_nan:
                assert np.isnan(d[0]).all() and np.isnan(d[-1]).all() and np.isnan(d[:, 0]).all() and np.isnan(d[:, -1]).all()
            else:
                assert np.isfinite(d).all() and d.max() > 0


def test_row_varying_spacing():
    import capacity_terrain as CT
    from pydem_amd import synth
    n, m = 200, 150
    z = synth.fractal(n, m, seed=19, top_shift=7, n_octaves=7)
    dX, dY = CT.spacing(n, seed=4)
    sp = dict(dX=dX, dY=dY, dX2=np.r_[dX, dX[-1]] + 0.003, dY2=np.r_[dY[0], dY] - 0.007)
    o, dp = pair(z, **sp)
    for kind, stat, edge_nan in (('h', 'max', True), ('s', 'ave', True), ('h', 'ave', False), ('s', 'max', False), ('v', 'min', False)):
        d = dp.calc_dist_up(kind=kind, stat=stat, edge_nan=edge_nan)
        compare(d, o, kind, stat, edge_nan, 'row-varying spacing %s/%s edge_nan=%r' % (kind, stat, edge_nan), min_finite=0.7)


SCHEDULE_CASES = (('h', 'max', True), ('s', 'ave', False), ('v', 'min', True))


def schedule_results():
    """what the three schedules must agree on, bit for bit: (sha256 of the result, levels, unresolved) per call"""
    import sys
    out = []
    for name, dp in (('fractal', fractal_pair(*FRACTALS[0])[1]), ('deep ramp', deep_pair()[1]), ('two_loops', circular_case('two_loops')[1])):
        for kind, stat, edge_nan in SCHEDULE_CASES:
            if name == 'deep ramp':
                edge_nan = False
            sys.stderr.write('--- %s %s/%s\n' % (name, kind, stat))
            sys.stderr.flush()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                d = dp.calc_dist_up(kind=kind, stat=stat, edge_nan=edge_nan)
            out.append((name, bits(d), dp.dist_up_stats['levels'], dp.dist_up_stats['n_unresolved']))
    return out


@pytest.mark.parametrize('env', [{'PYDEM_DIST_PASSES': '0'}, {'PYDEM_DIST_MIN_PER_VISIT': '0'}, {}])
def test_schedules(env):
    """the queue alone, tile passes to the end, the default (the switches are read once per process: a fresh child each), held
    to this process's results, which the other tests hold to the reference: identical bits across the three"""
    import re
    here = schedule_results()
    assert here[-1][3] > 0 and here[0][3] == 0
    r = run_child("from test_gpu_dist_up import schedule_results\nprint('RESULTS', schedule_results())\nprint('CHILD-OK')",
                  env=dict(env, PYDEM_DIST_DEBUG='1'), timeout=300)
    there = eval(r.stdout.split('RESULTS', 1)[1].splitlines()[0])
    assert [(a[0], a[1], a[3]) for a in there] == [(a[0], a[1], a[3]) for a in here]
    # what each schedule got to do: "dist_up: <open> open cells, <visits> tile visits finished <cells>, queue: <levels> levels, ..."
    log = {}
    for block in r.stderr.split('--- ')[1:]:
        mt = re.search(r'dist_up: (\d+) open cells, (\d+) tile visits finished (\d+), queue: (\d+) levels, (\d+) cells', block)
        log.setdefault(block.split(' ', 1)[0], []).append(tuple(int(x) for x in mt.groups()))
    deep_depth = deep_ramp_depth()
    for name, rows in log.items():
        for (n_open, visits, by_passes, qlevels, qcells), res in zip(rows, [a for a in there if a[0].split(' ')[0] == name]):
            if env.get('PYDEM_DIST_PASSES') == '0':
                assert visits == 0 and by_passes == 0 and qcells == n_open - res[3]       # the queue alone gives the complete result
                if name == 'deep':
                    assert res[2] == deep_depth                                          # ... in the reference's levels
            elif 'PYDEM_DIST_MIN_PER_VISIT' in env:
                assert by_passes == n_open - res[3] or qlevels > 0                       # (cycles: the queue confirms that nothing is ready)
                if name == 'deep':
                    assert res[2] < deep_depth                     # a pass finishes whole chains inside a block, not one cell of each
            elif name == 'deep':
                assert visits > 0 and qlevels > 0 and qcells > 0                         # the deep ramp reaches the queue by default


def test_state_integrity():
    """the call writes nothing but its own state: fields, graph words, pit lists and timings are bit-equal around it; the
    downslope distance, whose planes it shares, gives the same bits before and after it"""
    from pydem_amd import DEMProcessor, synth
    z = synth.fractal(520, 700, seed=11, top_shift=7, n_octaves=7)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
        dp.run_slopes_directions(); dp.run_uca(); dp.run_twi()
        down0 = dp.calc_dist_down(uca_threshold=300 * 900.0, kind='s', stat='ave')
        before = _snapshot(dp)
        assert len(before[0]) >= 10
        named = {k: np.array(getattr(dp, k)) for k in ('uca', 'section', 'proportion', 'edge_todo', 'mag', 'flats')}
        a = dp.calc_dist_up(kind='s', stat='ave')
        b = dp.calc_dist_up(kind='h', stat='max', edge_nan=False)
        assert np.isfinite(a).any() and np.isfinite(b).all() and not np.array_equal(a, b, equal_nan=True)
        _same_snapshot(before, _snapshot(dp))
        for k, v in named.items():
            assert np.array(getattr(dp, k)).tobytes() == v.tobytes(), k
        assert bits(a) != bits(down0)
        down1 = dp.calc_dist_down(uca_threshold=300 * 900.0, kind='s', stat='ave')
        assert down1.tobytes() == down0.tobytes()
        again = dp.calc_dist_up(kind='s', stat='ave')
        assert again.tobytes() == a.tobytes() and again is not a
        _same_snapshot(before, _snapshot(dp))


def test_edge_rounds_of_a_mosaic_after_the_call(tmp_path):
    """the 2 x 2 mosaic of the directory flow with a calc_dist_up after every calc_uca, edge rounds included: the reference's
    per-tile and stitched results, as without the calls"""
    from conftest import load_golden
    from pydem_amd import DEMProcessor
    from test_gpu_process_manager import _close
    from test_process_manager_cpu import compare_with_golden, run_pm
    calls = []

    class WithDistUp(DEMProcessor):
        def run_uca(self, *a, **kw):
            DEMProcessor.run_uca(self, *a, **kw)
            d = self.calc_dist_up(stat='ave', edge_nan=False)
            calls.append((bool(kw.get('edge_init_data')), np.isfinite(d).mean()))

    g = load_golden('pm_fractal_2x2_ov2')
    pm, compact, order = run_pm(g, str(tmp_path), processor_cls=WithDistUp)
    compare_with_golden(pm, compact, order, g, _close)
    assert pm.edge_rounds >= 1
    assert sum(1 for e, _ in calls if not e) >= 4 and sum(1 for e, _ in calls if e) >= 1 and all(f > 0 for _, f in calls)


def test_memory():
    """the state is the downslope distance's result plane and int32 plane, 12 B per cell, and four words per 32 x 32 block
    behind 16 counter words: taken by the first call, nothing by the second, nothing more by a downslope call with a threshold"""
    from pydem_amd import DEMProcessor, _ffi, synth
    n, m = 333, 450
    z = synth.fractal(n, m, seed=23, top_shift=7, n_octaves=7)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
        dp.run_slopes_directions(); dp.run_uca()
        b0 = dp._tile.device_bytes()
        first = dp.calc_dist_up()
        b1 = dp._tile.device_bytes()
        blocks = -(-n // 32) * -(-m // 32)
        assert 0 < b1 - b0 <= 12 * n * m + 4 * (16 + 4 * blocks), (b0, b1)
        free1 = _ffi.device_memory(0)[0]
        for _ in range(5):
            assert dp.calc_dist_up().tobytes() == first.tobytes()
        assert dp._tile.device_bytes() == b1 and _ffi.device_memory(0)[0] >= free1
        dp.calc_dist_down(uca_threshold=200 * 900.0)
        assert dp._tile.device_bytes() == b1


def test_no_graph_is_an_error():
    from pydem_amd import DEMProcessor, _ffi, synth
    z = synth.fractal(64, 80, seed=2, top_shift=5, n_octaves=5)
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.dist_up('h', 'max')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d = dp.calc_dist_up(edge_nan=False)                                # runs calc_uca first
    assert np.isfinite(d).all() and dp._has('uca')
    dp._tile.upload(_ffi.ELEV, z + 1.0)                                    # the elevation changed: the graph is gone
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.dist_up('h', 'max')
