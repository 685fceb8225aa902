"""The stream network on the device (DEMProcessor.calc_flow_receiver / calc_stream_network, pydem_stream_network) against the
Kahn reference of tests/test_stream_network_ref.py, cell by cell.  The reference is fed the DEVICE's own edge list (rebuilt from
the graph words, the proportion and the kept pit edges, as assert_edge_set_equals_oracle of tests/test_gpu_parity.py rebuilds it)
and the device's own stream set: oracle and device weights agree only to a tolerance, and a receiver is an argmax.  On identical
inputs every output is an integer: np.array_equal everywhere, no tolerance anywhere.

The tiles: (300, 260) is 10 x 9 blocks of 32 x 32, both ragged -- the tile tests/test_stream_network_ref.py sizes the coverage
on --, (96, 80) is 3 x 3.  Then properties that do not go through the reference, the designed fields of tests/flow_fields.py,
circular drainage, no-data cells, the schedules, what the call must leave alone, run-to-run identity, memory, the error codes."""
import functools
import warnings

import numpy as np
import pytest

from flowgraph_kit import _same_snapshot, _snapshot, circular_case, deep_pair, fractal_pair as make, nan_speck_pair, run_child
from test_stream_network_ref import coverage, stream_network_ref, top_fraction

pytestmark = pytest.mark.gpu

TILES = [((300, 260), 5), ((96, 80), 5)]
PLANES = ('receiver', 'order', 'link', 'basin')


def device_edges(dp, z):
    """(src, dst, w, is_pit) of the flow graph on the tile: the regular edges of the graph words with weights p and 1 - p, the
    pit edges that pass the keep-filter"""
    n, m = dp.shape
    words = dp._tile.graph_words().ravel()
    prop = np.asarray(dp.proportion, np.float64).ravel()
    sec = ((words >> 12) & 7).astype(int)
    e1r = np.array([0, -1, -1, 0, 0, 1, 1, 0]); e1c = np.array([1, 0, 0, -1, -1, 0, 0, 1])
    e2r = np.array([-1, -1, -1, -1, 1, 1, 1, 1]); e2c = np.array([1, 1, -1, -1, -1, -1, 1, 1])
    cells = np.arange(n * m)
    parts = []
    for bit, dr, dc, w in ((8, e1r, e1c, prop), (9, e2r, e2c, 1 - prop)):
        has = ((words >> bit) & 1).astype(bool)
        src = cells[has]
        parts.append((src, src + dr[sec[has]] * m + dc[sec[has]], w[has], np.zeros(src.size, bool)))
    ps, pd, pw = dp._tile.pit_edges()
    zz = np.asarray(z, np.float64).ravel()
    keep = ~np.isnan(pw) & (pw > 1e-8) & (zz[pd] <= zz[ps])
    parts.append((ps[keep].astype(np.int64), pd[keep].astype(np.int64), pw[keep], np.ones(int(keep.sum()), bool)))
    return tuple(np.concatenate(x) for x in zip(*parts))


def stream_set(dp, thr):
    with np.errstate(invalid='ignore'):
        return np.asarray(dp.uca) >= thr


def assert_network(dp, z, edges, S, what, thr=None, basins=True):
    """one calc_stream_network call (by threshold if `thr` is given, else with S as a mask) and one raw call against the
    reference; returns (the StreamNetwork, the reference)"""
    from pydem_amd import streamnet
    ref = stream_network_ref(edges, tuple(dp.shape), z, S)
    kw = dict(uca_threshold=thr) if thr is not None else dict(streams=S)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        net = dp.calc_stream_network(basins=basins, **kw)
        raw, ms, levels, left = dp._tile.stream_network(None if thr is not None else S, thr, basin=basins)
    st = dp.stream_network_stats
    for name in PLANES[:3] + (('basin',) if basins else ()):
        bad = raw[name] != getattr(ref, name)
        assert not bad.any(), "%s: raw %s differs at %d cells, first %r" % (what, name, bad.sum(), np.argwhere(bad)[0].tolist())
    want = streamnet.compact_network(ref.receiver, ref.order, ref.link, ref.basin if basins else None)
    assert net is dp.stream_network and dp.flow_receiver is net.receiver
    for name in PLANES:
        a, b = getattr(net, name), getattr(want, name)
        if b is None:
            assert a is None and raw[name] is None
        else:
            assert a.dtype == np.int32 and np.array_equal(a, b), "%s: %s" % (what, name)
    assert np.array_equal(net.links, want.links)
    assert set(st) == {'ms', 'levels', 'n_unresolved', 'n_links', 'max_order'}
    expect_left = ref.n_unresolved if basins else (ref.n_unresolved[0], 0)
    assert st['n_unresolved'] == left == expect_left, (what, st['n_unresolved'], left, expect_left)
    assert st['n_links'] == want.links.size and st['max_order'] == int(ref.order.max())
    assert len(st['ms']) == 3 and st['ms'][0] > 0 and st['ms'][1] > 0 and (st['ms'][2] > 0) == basins
    assert len(st['levels']) == 2 and st['levels'][0] >= 1 and (st['levels'][1] >= 1) == basins
    return net, ref


@functools.lru_cache(maxsize=None)
def fractal_case(shape, seed):
    """(elevation, device processor after calc_uca, its edge list)"""
    o, dp = make(shape, seed)
    z = np.asarray(o.elev, np.float64)
    return z, dp, device_edges(dp, z)


# ---- 1. fractal tiles
def check_fractal(shape, seed, frac):
    z, dp, edges = fractal_case(shape, seed)
    thr = top_fraction(dp.uca, frac)
    S = stream_set(dp, thr)
    what = '%r top %g' % (shape, frac)
    net, ref = assert_network(dp, z, edges, S, what + ' by threshold', thr=thr)
    masked, _ = assert_network(dp, z, edges, S, what + ' by mask')
    assert all(np.array_equal(getattr(net, k), getattr(masked, k)) for k in PLANES) and np.array_equal(net.links, masked.links)
    cov = coverage(ref, edges, shape, S)
    print(what, cov, dp.stream_network_stats)
    return net, ref, cov


@pytest.mark.parametrize('frac', [0.05, 0.10])
@pytest.mark.parametrize('shape,seed', TILES)
def test_fractal_tiles(shape, seed, frac):
    net, ref, cov = check_fractal(shape, seed, frac)
    assert ref.n_unresolved == (0, 0) and cov['links'] >= 20
    if shape == (300, 260) and frac == 0.05:
        assert cov['max_order'] >= 4 and cov['links'] >= 1000 and cov['many'] >= 50 and cov['pit_recv'] >= 300
        assert cov['cross'] >= 200 and cov['leaves'] >= 100
    z, dp, edges = fractal_case(shape, seed)
    recv = dp.calc_flow_receiver()                                        # the receivers alone: no stream set
    assert recv is dp.flow_receiver and recv.dtype == np.int32 and np.array_equal(recv, ref.receiver)
    without, _ = assert_network(dp, z, edges, stream_set(dp, top_fraction(dp.uca, frac)), 'no basins', basins=False)
    assert without.basin is None and np.array_equal(without.link, net.link)


# ---- 2. properties, not through the reference
def test_properties_of_the_network():
    shape, seed = TILES[0]
    z, dp, edges = fractal_case(shape, seed)
    thr = top_fraction(dp.uca, 0.05)
    S = stream_set(dp, thr)
    net = dp.calc_stream_network(uca_threshold=thr)
    links = net.links
    K = links.size
    rf, of, lf, bf = (x.ravel().astype(np.int64) for x in (net.receiver, net.order, net.link, net.basin))
    Sf = S.ravel()
    assert dp.stream_network_stats['n_unresolved'] == (0, 0) and np.array_equal(lf > 0, Sf) and np.array_equal(of > 0, Sf)
    # the order is constant on every link
    on = np.flatnonzero(Sf)
    assert np.array_equal(of[on], links['order'][lf[on] - 1])
    # following the receivers from the head reaches the tail in n_cells - 1 steps inside the link
    cur, steps = links['head'].copy(), links['n_cells'] - 1
    for s in range(int(steps.max())):
        go = steps > s
        cur[go] = rf[cur[go]]
        assert (lf[cur[go]] == links['id'][go]).all()
    assert np.array_equal(cur, links['tail'])
    # the head orders follow the Strahler rule, recomputed from `down`
    feeds = links[links['down'] > 0]
    hi = np.zeros(K + 1, np.int64)
    np.maximum.at(hi, feeds['down'], feeds['order'])
    k = np.bincount(feeds['down'][feeds['order'] == hi[feeds['down']]], minlength=K + 1)
    n_in = np.bincount(feeds['down'], minlength=K + 1)
    want = np.where(n_in == 0, 1, np.where(k >= 2, hi + 1, hi))[1:]
    assert (n_in[1:] != 1).all() and np.array_equal(links['order'], want) and links['order'].max() >= 4
    # basins
    assert np.array_equal(bf[on], lf[on])
    off = np.flatnonzero(~Sf)
    has = rf[off] >= 0
    assert np.array_equal(bf[off[has]], bf[rf[off[has]]]) and (bf[off[~has]] == 0).all()
    # against the dependence: each receiver edge has weight >= the cell's other out-edges' and > 1e-8, so all of basin L
    # has a positive share of its flow reaching link L
    sizes = np.bincount(bf[bf > 0], minlength=K + 1)
    for order in (1, 2, 3):
        cand = links['id'][links['order'] == order]
        L = int(cand[np.argmax(sizes[cand])])
        dep = dp.calc_up_dependence(net.link == L)
        inside = net.basin == L
        print("order %d: link %d, %d cells, basin %d cells, %d cells with dep > 0" % (order, L, (net.link == L).sum(), inside.sum(), (dep > 0).sum()))
        assert inside.sum() > (net.link == L).sum() and (dep[inside] > 0).all()


# ---- 3. designed fields
FIELD_NAMES = ['row_snake', 'tile_snake', 'fan0', 'fan1', 'fan2', 'fan3', 'fan4', 'fan5', 'fan6', 'fan7', 'far_pit', 'near_pit',
               'tall', 'wide']


@pytest.mark.parametrize('name', FIELD_NAMES)
def test_designed_fields(name):
    from test_gpu_flow_fields import FIELDS, pair
    field = FIELDS[name]()
    o, dp = pair(name)
    z = np.asarray(field.elev, np.float64)
    edges = device_edges(dp, z)
    thr = 2.0 * float(dp.dX2[0] * dp.dY2[0])
    S = stream_set(dp, thr)
    net, ref = assert_network(dp, z, edges, S, name, thr=thr)
    assert ref.n_unresolved == (0, 0) and S.any()
    print(name, coverage(ref, edges, z.shape, S), dp.stream_network_stats)
    if 'paths' in field.facts:
        # one path through many tiles comes out as one order-1 link
        assert net.links.size == len(field.facts['paths']) and (net.links['order'] == 1).all()
        assert net.links['n_cells'].sum() == S.sum() and net.links['n_cells'].max() >= len(field.facts['path']) - 2
    if name.endswith('_pit'):
        pit = field.facts['pit']
        assert ref.code[pit] == 8 and net.receiver[pit] == ref.receiver[pit] >= 0      # a receiver that is a pit edge


# ---- 4. the deep chain and circular drainage
def check_deep():
    o, dp = deep_pair((200, 48))
    z = np.asarray(o.elev, np.float64)
    edges = device_edges(dp, z)
    thr = top_fraction(dp.uca, 0.10)
    net, ref = assert_network(dp, z, edges, stream_set(dp, thr), 'deep ramp', thr=thr)
    assert ref.n_unresolved == (0, 0) and net.links.size >= 20
    # every cell a stream: every cell with an in-edge is open, and the flow paths run the 200 rows of the ramp -- 7 row blocks,
    # of which a pass finishes at most one per path, and a level of the queue one cell
    net, ref = assert_network(dp, z, edges, np.ones(z.shape, bool), 'deep ramp, every cell a stream')
    st = dp.stream_network_stats
    print("deep ramp: levels %r, %d links, max order %d" % (st['levels'], st['n_links'], st['max_order']))
    assert ref.n_unresolved == (0, 0) and st['levels'][0] >= 7 and np.array_equal(net.basin, net.link)
    return dp


def test_deep_chain():
    check_deep()


def check_circular(loop):
    o, dp = circular_case(loop)
    n, m = dp.shape
    z = np.asarray(o.elev, np.float64)
    edges = device_edges(dp, z)
    # every cell a stream: the loops and what lies downstream of them are unresolved in the forward sweep
    S = np.ones((n, m), bool)
    with pytest.warns(UserWarning, match='circular drainage'):
        net = dp.calc_stream_network(streams=S)
    _, ref = assert_network(dp, z, edges, S, loop + ' all streams')
    assert ref.n_unresolved[0] > 0 and ref.n_unresolved[1] == ref.n_unresolved[0]
    assert np.array_equal(net.order == -1, ref.order == -1) and np.array_equal(net.link == -1, ref.order == -1)
    assert (net.links['down'] == -1).any()
    # only the last row: the loops are off the streams, they and what lies upstream of them are unresolved in the reverse sweep
    S = np.zeros((n, m), bool)
    S[-1] = True
    with pytest.warns(UserWarning, match='circular drainage'):
        net = dp.calc_stream_network(streams=S)
    _, ref = assert_network(dp, z, edges, S, loop + ' last row')
    assert ref.n_unresolved[0] == 0 and ref.n_unresolved[1] > 0 and np.array_equal(net.basin == -1, ref.basin == -1)
    assert (net.order >= 0).all() and (net.link >= 0).all()


@pytest.mark.parametrize('loop', ['two_cells', 'three_cells', 'two_loops'])
def test_circular_drainage_is_minus_one_and_counted(loop):
    check_circular(loop)


# ---- 5. NaN specks
def test_nan_specks():
    n, m = 96, 80
    z, _, dp, _ = nan_speck_pair((n, m), 12, [(0, 5), (95, 30), (20, 0)])
    nodata = np.isnan(z)
    assert 13 <= nodata.sum() <= 15
    edges = device_edges(dp, z)
    thr = 50 * 900.0
    net, ref = assert_network(dp, z, edges, stream_set(dp, thr), 'NaN specks', thr=thr)
    for plane, value in ((net.receiver, -1), (net.order, 0), (net.link, 0), (net.basin, 0)):
        assert (plane[nodata] == value).all()
    assert ref.n_unresolved == (0, 0) and (net.order > 0).sum() >= 20
    # a mask over the no-data cells does not revive them
    everything = np.ones((n, m), bool)
    net, ref = assert_network(dp, z, edges, everything, 'NaN specks, every cell a stream')
    assert (net.order[nodata] == 0).all() and (net.link[nodata] == 0).all() and (net.basin[nodata] == 0).all()
    assert (net.order[~nodata] != 0).all() and np.array_equal(net.basin, net.link)


# ---- 6. schedules
def check_schedules():
    """(child process) the cases that differ in what the tile passes and the queue each get to do: each is compared with the
    reference, whose planes do not know about schedules"""
    from test_gpu_flow_fields import FIELDS, pair
    check_fractal(TILES[1][0], TILES[1][1], 0.05)
    check_fractal(TILES[1][0], TILES[1][1], 0.10)
    check_deep()
    check_circular('two_loops')
    for name in ('row_snake', 'far_pit'):
        field = FIELDS[name]()
        o, dp = pair(name)
        z = np.asarray(field.elev, np.float64)
        assert_network(dp, z, device_edges(dp, z), stream_set(dp, 12.0), name, thr=12.0)
    return dp.stream_network_stats['levels']


@pytest.mark.parametrize('env', [{'PYDEM_DIST_PASSES': '0'}, {'PYDEM_DIST_MIN_PER_VISIT': '0'}, {'PYDEM_DIST_PASSES': '2'}])
def test_schedules(env):
    """the queue alone, tile passes to the end, two passes then the queue (the switches are read once per process)"""
    r = run_child("from test_gpu_stream_network import check_schedules\nprint('LEVELS', check_schedules())\nprint('CHILD-OK')", env=env, timeout=300)
    print(env, r.stdout.split('LEVELS', 1)[1].splitlines()[0])


# ---- 7. state integrity
def test_state_integrity():
    shape, seed = TILES[1]
    o, dp = make(shape, seed)                           # (a pair of this test's own)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        uca = np.array(dp.uca)
        up = dp.calc_dist_up(edge_nan=False)
        before = _snapshot(dp)
        thr = top_fraction(uca, 0.10)
        net = dp.calc_stream_network(uca_threshold=thr)
        dp.calc_flow_receiver()
        dp.calc_stream_network(streams=uca >= thr, basins=False)
        assert net.links.size >= 20
        _same_snapshot(before, _snapshot(dp))
        assert np.array(dp.uca).tobytes() == uca.tobytes()
        assert dp.calc_dist_up(edge_nan=False).tobytes() == up.tobytes()
        dep = dp.calc_up_dependence(net.link == 1)
        again = dp.calc_stream_network(uca_threshold=thr)
        assert all(np.array_equal(getattr(net, k), getattr(again, k)) for k in PLANES)
        assert dp.calc_up_dependence(net.link == 1).tobytes() == dep.tobytes()


# ---- 8. repeatability and memory
def test_identical_calls_and_no_growth():
    from pydem_amd import _ffi
    shape, seed = TILES[1]
    z, dp, edges = fractal_case(shape, seed)
    thr = top_fraction(dp.uca, 0.10)
    first = dp.calc_stream_network(uca_threshold=thr)   # (warm-up: the call's planes exist from here on)
    dp.calc_stream_network(streams=stream_set(dp, thr))
    free0 = _ffi.device_memory(0)[0]
    for k in range(20):
        net = dp.calc_stream_network(uca_threshold=thr) if k % 2 == 0 else dp.calc_stream_network(streams=stream_set(dp, thr))
        assert all(getattr(net, name).tobytes() == getattr(first, name).tobytes() for name in PLANES)
        assert net.links.tobytes() == first.links.tobytes()
    assert _ffi.device_memory(0)[0] >= free0


# ---- 9. errors
def test_errors():
    from pydem_amd import DEMProcessor, _ffi, synth
    z = synth.fractal(64, 80, seed=2, top_shift=5, n_octaves=5)
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    everything = np.ones((64, 80), bool)
    for kw in (dict(streams=everything), dict(uca_threshold=900.0), dict(order=False, link=False, basin=False)):
        with pytest.raises(_ffi.HipError, match='no flow graph'):
            dp._tile.stream_network(**kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        net = dp.calc_stream_network(streams=everything)                  # runs calc_uca first
    assert dp._has('uca') and (net.order != 0).all()
    for bad in (np.nan, np.inf, -1.0):
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp._tile.stream_network(None, bad)
    with pytest.raises(ValueError):
        dp._tile.stream_network()                                         # a sweep without a stream set
    with pytest.raises(ValueError):
        dp._tile.stream_network(np.ones((64, 79), bool))
    # the receivers alone need no stream set, whatever the threshold says
    planes, ms, levels, left = dp._tile.stream_network(order=False, link=False, basin=False)
    assert np.array_equal(planes['receiver'], net.receiver) and planes['order'] is None and ms[0] > 0 and ms[1:] == (0.0, 0.0)
    assert levels == (0, 0) and left == (0, 0)
    again = dp.calc_stream_network(streams=everything)                    # the refused calls left the state alone
    assert all(np.array_equal(getattr(net, k), getattr(again, k)) for k in PLANES)
    dp._tile.upload(_ffi.ELEV, z + 1.0)                                   # the elevation changed: the graph is gone
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.stream_network(everything)
