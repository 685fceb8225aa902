"""The receiver-tree accumulation on the device (DEMProcessor.calc_tree_accum / calc_reach_attributes, pydem_tree_accum) against
the Kahn reference of tests/test_tree_accum_ref.py, cell by cell.  The reference is fed the DEVICE's own edge list, stream set and
load (device_edges / stream_set of tests/test_gpu_stream_network.py) and does the device's operations in the device's order: every
comparison is tobytes() equality, no tolerance anywhere -- except where a property is held against numpy's own sums, whose order
differs; the bound is stated there.

The tiles are those of tests/test_gpu_stream_network.py: (300, 260) is 10 x 9 blocks of 32 x 32, both ragged, (96, 80) is 3 x 3.
Then properties that do not go through the reference, the designed fields of tests/flow_fields.py, the deep ramp, circular
drainage, no-data cells, the schedules, what the call must leave alone, run-to-run identity, memory, the error codes, and the
table of calc_reach_attributes."""
import functools
import warnings

import numpy as np
import pytest

from flowgraph_kit import _same_snapshot, _snapshot, circular_case, deep_pair, fractal_pair as make, nan_speck_pair, run_child
from test_gpu_stream_network import TILES, device_edges, fractal_case, stream_set
from test_stream_network_ref import stream_network_ref, top_fraction
from test_tree_accum_ref import OPS, finite_below_nan, reach_table_ref, tree_accum_ref

pytestmark = pytest.mark.gpu


def random_load(shape, seed):
    """a load with negative values and exact zeros"""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 3.0, shape)
    w[rng.random(shape) < 0.1] = 0.0
    assert (w < 0).mean() > 0.3
    return w


def assert_accum(dp, z, edges, load, op, S, edge_nan, what, thr=None, net=None, at=None):
    """one raw call (cut by threshold if `thr` is given, by the mask S if S is given, else the whole tree) against the
    reference: the plane, the gathered values, the unresolved count; returns (plane, reference's count)"""
    shape = tuple(dp.shape)
    ref, left_ref = tree_accum_ref(edges, shape, z, load, op, S, edge_nan, net=net)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out, vals, ms, levels, left = dp._tile.tree_accum(load, op, None if thr is not None else S, thr, edge_nan, at)
    bad = out.view(np.uint64) != ref.view(np.uint64)
    assert not bad.any(), "%s: %d cells differ, first %r: device %r, reference %r" % (
        what, bad.sum(), np.argwhere(bad)[0].tolist(), out[bad][0], ref[bad][0])
    assert out.tobytes() == ref.tobytes() and left == left_ref and ms > 0 and levels >= 1, (what, left, left_ref, ms, levels)
    if at is not None:
        assert vals.dtype == np.float64 and vals.tobytes() == out.ravel()[np.asarray(at)].tobytes(), what + ': gathered values'
    else:
        assert vals is None
    return out, left_ref


@functools.lru_cache(maxsize=None)
def fractal_set(shape, seed, frac):
    """(threshold, device stream set, reference network on the device's edges, the compacted network) of a fractal tile"""
    from pydem_amd import streamnet
    z, dp, edges = fractal_case(shape, seed)
    thr = top_fraction(dp.uca, frac)
    S = stream_set(dp, thr)
    ref = stream_network_ref(edges, shape, z, S)
    return thr, S, ref, streamnet.compact_network(ref.receiver, ref.order, ref.link, ref.basin)


# ---- 1. fractal tiles
def check_fractal(shape, seed, frac, op):
    z, dp, edges = fractal_case(shape, seed)
    thr, S, ref, net = fractal_set(shape, seed, frac)
    load = random_load(shape, 17)
    tails = net.links['tail']
    what = '%r top %g %s' % (shape, frac, op)
    for edge_nan in (True, False):
        cut, left = assert_accum(dp, z, edges, load, op, S, edge_nan, what + ' cut by mask, edge_nan %r' % edge_nan, net=ref, at=tails)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            by_thr, vals, _, _, _ = dp._tile.tree_accum(load, op, None, thr, edge_nan, tails[::-1])
        assert by_thr.tobytes() == cut.tobytes() and vals.tobytes() == cut.ravel()[tails[::-1]].tobytes()    # by threshold: the same set
        whole, left_w = assert_accum(dp, z, edges, load, op, None, edge_nan, what + ' whole tree, edge_nan %r' % edge_nan, at=tails[:5])
        assert left == 0 and left_w == 0 and whole.tobytes() != cut.tobytes()
        assert np.isfinite(cut).all() == (not edge_nan) and np.isfinite(cut).sum() >= 0.5 * cut.size
    return net


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('frac', [0.05, 0.10])
@pytest.mark.parametrize('shape,seed', TILES)
def test_fractal_tiles(shape, seed, frac, op):
    net = check_fractal(shape, seed, frac, op)
    assert net.links.size >= 20


def test_public_call_and_default_weights():
    shape, seed = TILES[1]
    z, dp, edges = fractal_case(shape, seed)
    thr, S, ref, net = fractal_set(shape, seed, 0.10)
    area = np.full(shape, 900.0)
    for kw, Sref in ((dict(), None), (dict(uca_threshold=thr), S), (dict(streams=S), S)):
        out = dp.calc_tree_accum(**kw)                                     # weights None: the cell area, edge_nan on
        want, _ = tree_accum_ref(edges, shape, z, area, 'sum', Sref, True)
        assert out is dp.tree_accum and out.dtype == np.float64 and out.tobytes() == want.tobytes()
        st = dp.tree_accum_stats
        assert set(st) == {'ms', 'levels', 'n_unresolved', 'edge_nan', 'cut'} and st['cut'] == (Sref is not None)
        assert st['edge_nan'] is True and st['n_unresolved'] == 0 and st['ms'] > 0 and st['levels'] >= 1
    w = random_load(shape, 3)
    out = dp.calc_tree_accum(np.ma.masked_array(w, mask=w > 4.0), op='max', edge_nan=False)
    want, _ = tree_accum_ref(edges, shape, z, np.where(w > 4.0, 0.0, w), 'max', None, False)
    assert out.tobytes() == want.tobytes() and dp.tree_accum_stats['edge_nan'] is False
    assert dp.calc_tree_accum(2.5, edge_nan=False).tobytes() == tree_accum_ref(edges, shape, z, np.full(shape, 2.5), 'sum', None, False)[0].tobytes()


# ---- 2. properties, not through the reference
def basin_sum_bound(count, abs_sum):
    """two sums of `count` terms in different orders differ by at most 2 (count - 1) u sum|terms| + O(u^2), u = 2^-53: each is
    within (count - 1) u sum|terms| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); the
    test uses 2 count u sum|terms|"""
    return 2.0 * count * 2.0 ** -53 * abs_sum


def test_properties_of_the_reach_table():
    shape, seed = TILES[0]
    z, dp, edges = fractal_case(shape, seed)
    thr = top_fraction(dp.uca, 0.05)
    values = np.array(dp.mag, np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        net = dp.calc_stream_network(uca_threshold=thr)
        basin, links = net.basin.ravel().astype(np.int64), net.links
        plain = dp.calc_reach_attributes(uca_threshold=thr, values=values, edge_nan=False)
        st_plain = dp.reach_attributes_stats
        whole = dp.calc_tree_accum(edge_nan=False)
        above = dp.calc_tree_accum(stream_set(dp, thr).astype(np.float64), edge_nan=False)
        table = dp.calc_reach_attributes(uca_threshold=thr, values=values, edge_nan=True)
    K = links.size
    assert np.array_equal(dp.stream_network.links, links) and dp.stream_network.basin is None and table is dp.reach_attributes
    assert plain.size == K >= 1000 and np.array_equal(plain['id'], links['id'])
    assert set(st_plain) == {'ms', 'sweeps', 'edge_nan', 'n_links'} and st_plain['n_links'] == K and st_plain['edge_nan'] is False
    assert set(st_plain['sweeps']) == {'local_cells', 'local_area', 'total_area', 'magnitude', 'v_sum', 'v_min', 'v_max'}
    assert all(s['n_unresolved'] == 0 and s['ms'] > 0 for s in st_plain['sweeps'].values())
    # the cut count is the basin's size, exactly; the cut area its area within the bound of two sums of n_L positive terms
    count = np.bincount(basin[basin > 0], minlength=K + 1)[1:]
    assert plain['complete'].all() and np.array_equal(plain['local_cells'], count)
    area = np.broadcast_to((dp.dX2 * dp.dY2)[:, None], shape).ravel()
    want = np.bincount(basin[basin > 0], weights=area[basin > 0], minlength=K + 1)[1:]
    err = np.abs(plain['local_area'] - want)
    print("local_area: max error %.3g, bound there %.3g" % (err.max(), basin_sum_bound(count, want)[np.argmax(err)]))
    assert (err <= basin_sum_bound(count, want)).all()
    # the whole tree ends at the cells without a receiver: together they hold the tile's area
    nodata = np.isnan(z)
    ends = (net.receiver < 0) & ~nodata
    total, n_cells = area[~nodata.ravel()].sum(), int((~nodata).sum())
    print("whole tree: %d ends hold %.17g of %.17g" % (ends.sum(), whole[ends].sum(), total))
    assert abs(whole[ends].sum() - total) <= basin_sum_bound(n_cells, total)
    assert (plain['total_area'] >= plain['local_area']).all() and (plain['total_area'] > plain['local_area']).any()
    assert np.array_equal(plain['total_area'], whole.ravel()[links['tail']])
    # magnitude: the sources above the tail -- 1 where no stream cell but the link's own lies above it (a link of order 1 may
    # hold more: a stream that left the stream set can come back in), at least 2 below a junction
    top = above.ravel()[links['tail']] == links['n_cells']
    assert top.sum() >= 500 and (plain['magnitude'][top] == 1).all() and (links['order'][top] == 1).all()
    assert (plain['magnitude'] >= 1).all() and (plain['magnitude'][links['order'] > 1] >= 2).all()
    # the edge rule: the cut stops the contamination at the link boundaries
    below = finite_below_nan(links, table['local_area'])
    print("%d links, %d complete, %d complete below an incomplete one; total_area finite for %d"
          % (K, table['complete'].sum(), below, np.isfinite(table['total_area']).sum()))
    assert below >= 10 and table['complete'].sum() > np.isfinite(table['total_area']).sum()
    ok = table['complete']
    for k in ('local_cells', 'local_area', 'v_sum', 'v_min', 'v_max', 'v_mean'):
        assert table[k][ok].tobytes() == plain[k][ok].tobytes() and np.isnan(table[k][~ok]).all(), k
    # the value columns against numpy's reductions per basin: min and max exactly, the sum within the bound scaled by sum |v|
    vf = values.ravel()
    print("values: %d NaN" % np.isnan(vf).sum())
    lo, hi = np.full(K + 1, np.inf), np.full(K + 1, -np.inf)
    np.minimum.at(lo, basin[basin > 0], vf[basin > 0])
    np.maximum.at(hi, basin[basin > 0], vf[basin > 0])
    assert np.array_equal(plain['v_min'], lo[1:], equal_nan=True) and np.array_equal(plain['v_max'], hi[1:], equal_nan=True)
    vsum = np.bincount(basin[basin > 0], weights=vf[basin > 0], minlength=K + 1)[1:]
    vabs = np.bincount(basin[basin > 0], weights=np.abs(vf[basin > 0]), minlength=K + 1)[1:]
    fin = np.isfinite(vsum)
    assert np.array_equal(fin, np.isfinite(plain['v_sum'])) and fin.sum() >= K // 2
    assert (np.abs(plain['v_sum'] - vsum)[fin] <= basin_sum_bound(count, vabs)[fin]).all()
    assert np.array_equal(plain['v_mean'], plain['v_sum'] / plain['local_cells'], equal_nan=True)
    assert (plain['v_min'][fin] <= plain['v_mean'][fin]).all() and (plain['v_mean'][fin] <= plain['v_max'][fin]).all()


# ---- 3. the table against the reference's
@pytest.mark.parametrize('edge_nan', [True, False])
@pytest.mark.parametrize('shape,seed', TILES)
def test_reach_attributes_bit_for_bit(shape, seed, edge_nan):
    from pydem_amd import streamnet
    z, dp, edges = fractal_case(shape, seed)
    thr = top_fraction(dp.uca, 0.10 if shape == (96, 80) else 0.05)
    S = stream_set(dp, thr)
    values = np.array(dp.mag, np.float64)
    want, net = reach_table_ref(edges, shape, z, S, dp.dX2, dp.dY2, values, edge_nan)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        table = dp.calc_reach_attributes(uca_threshold=thr, values=values, edge_nan=edge_nan)
        masked = dp.calc_reach_attributes(streams=S, values=values, edge_nan=edge_nan)
        short = dp.calc_reach_attributes(streams=S, edge_nan=edge_nan)
    links = dp.stream_network.links
    assert table.dtype == streamnet.REACH_VALUES_DTYPE and np.array_equal(links, net.links) and table.size == links.size >= 20
    for k in table.dtype.names:
        assert table[k].tobytes() == want[k].tobytes(), k
    assert masked.tobytes() == table.tobytes()
    assert short.dtype == streamnet.REACH_DTYPE and all(short[k].tobytes() == table[k].tobytes() for k in short.dtype.names)
    # length and drop from the host formula, recomputed here
    n, m = shape
    lf, rf = dp.stream_network.link.ravel(), dp.stream_network.receiver.ravel().astype(np.int64)
    length = np.zeros(links.size + 1)
    for c in np.flatnonzero(lf > 0).tolist():
        r = rf[c]
        if r >= 0 and lf[r] == lf[c]:
            length[lf[c]] += np.hypot((r % m - c % m) * dp.dX2[c // m], (r // m - c // m) * dp.dY2[c // m])
    # (a sum of n_cells <= 400 positive terms, each a hypot within an ulp, in the same order: (n_cells + 1) 2^-53 < 1e-13)
    assert links['n_cells'].max() <= 400 and np.allclose(table['length'], length[1:], rtol=1e-13, atol=0) and np.array_equal(table['length'] == 0, links['n_cells'] == 1)
    assert np.array_equal(table['drop'], z.ravel()[links['head']] - z.ravel()[links['tail']])
    assert (table['straight'] <= table['length'] * (1 + 1e-12)).all()                          # (uniform spacing)
    assert np.array_equal(table['complete'], np.isfinite(table['local_area'])) and table['complete'].all() == (not edge_nan)


# ---- 4. designed fields
FIELD_NAMES = ['row_snake', 'tile_snake', 'fan0', 'fan1', 'fan2', 'fan3', 'fan4', 'fan5', 'fan6', 'fan7', 'far_pit', 'near_pit',
               'tall', 'wide']


def check_field(name, thr=None):
    from test_gpu_flow_fields import FIELDS, pair
    from pydem_amd import streamnet
    field = FIELDS[name]()
    o, dp = pair(name)
    z = np.asarray(field.elev, np.float64)
    shape = z.shape
    edges = device_edges(dp, z)
    thr = 2.0 * float(dp.dX2[0] * dp.dY2[0]) if thr is None else thr      # (streams as in test_gpu_stream_network.test_designed_fields)
    S = stream_set(dp, thr)
    ref = stream_network_ref(edges, shape, z, S)
    net = streamnet.compact_network(ref.receiver, ref.order, ref.link, ref.basin)
    ones = np.ones(shape)
    tails = net.links['tail']
    cut, left = assert_accum(dp, z, edges, ones, 'sum', S, False, name + ' cut', thr=thr, net=ref, at=tails)
    whole, _ = assert_accum(dp, z, edges, ones, 'sum', None, False, name + ' whole tree')
    assert_accum(dp, z, edges, random_load(shape, 5), 'min', S, True, name + ' min, cut, edge_nan', net=ref)
    assert left == 0 and S.any()
    assert np.array_equal(cut.ravel()[tails], np.bincount(net.basin.ravel(), minlength=tails.size + 1)[1:])
    return field, ref, net, cut, whole


@pytest.mark.parametrize('name', FIELD_NAMES)
def test_designed_fields(name):
    field, ref, net, cut, whole = check_field(name)
    tails = net.links['tail']
    if 'paths' in field.facts:
        # one path through many tiles is one link: its tail carries the count of the whole path
        assert net.links.size == len(field.facts['paths'])
        assert cut.ravel()[tails].max() >= len(field.facts['path']) - 2 and cut.ravel()[tails].max() >= net.links['n_cells'].max()
    if name.endswith('_pit'):
        pit = field.facts['pit']
        r = ref.receiver[pit]
        assert ref.code[pit] == 8 and r >= 0                                  # the pit's value arrives through a pit receiver edge
        sources = np.flatnonzero(ref.receiver.ravel() == r)
        assert whole.ravel()[r] == 1 + whole.ravel()[sources].sum() and whole[pit] >= 1 and np.ravel_multi_index(pit, whole.shape) in sources


# ---- 5. the deep ramp, circular drainage, NaN specks
def check_deep():
    o, dp = deep_pair((200, 48))
    z = np.asarray(o.elev, np.float64)
    edges = device_edges(dp, z)
    every = np.ones(z.shape, bool)
    load = random_load(z.shape, 9)
    # every cell a stream: every cell with an in-edge is open, and the flow paths run the 200 rows of the ramp -- 7 row blocks
    ref = stream_network_ref(edges, z.shape, z, every)
    for op in OPS:
        _, left = assert_accum(dp, z, edges, load, op, every, False, 'deep ramp, every cell a stream, ' + op, net=ref)
        assert left == 0
    _, _, _, levels, _ = dp._tile.tree_accum(load, 'sum', every, None, False, download=False)
    assert levels >= 7
    _, left = assert_accum(dp, z, edges, load, 'sum', None, True, 'deep ramp, whole tree, edge_nan')
    assert left == 0
    return levels


def test_deep_chain():
    print("deep ramp: levels", check_deep())


def check_circular(loop):
    o, dp = circular_case(loop)
    z = np.asarray(o.elev, np.float64)
    edges = device_edges(dp, z)
    shape = z.shape
    load = random_load(shape, 2)
    last_row = np.zeros(shape, bool)
    last_row[-1] = True
    total = 0
    for S in (None, np.ones(shape, bool), last_row):
        for op in OPS:
            out, left = assert_accum(dp, z, edges, load, op, S, False, '%s %s' % (loop, op))
            assert left > 0 and np.isnan(out).sum() == left            # (no NaN elevation, no edge rule: the NaN are the unresolved)
            total += left
    with pytest.warns(UserWarning, match='circular drainage'):
        out = dp.calc_tree_accum(load, edge_nan=False)
    assert dp.tree_accum_stats['n_unresolved'] == np.isnan(out).sum() > 0
    return total


@pytest.mark.parametrize('loop', ['two_cells', 'three_cells', 'two_loops'])
def test_circular_drainage_is_nan_and_counted(loop):
    check_circular(loop)


def test_nan_specks():
    n, m = 96, 80
    z, _, dp, _ = nan_speck_pair((n, m), 12, [(0, 5), (95, 30), (20, 0)])
    nodata = np.isnan(z)
    edges = device_edges(dp, z)
    thr = 50 * 900.0
    S = stream_set(dp, thr)
    load = random_load((n, m), 6)
    for op in OPS:
        for edge_nan in (False, True):
            out, left = assert_accum(dp, z, edges, load, op, S, edge_nan, 'NaN specks %s' % op, thr=thr)
            assert left == 0 and np.isnan(out[nodata]).all() and (np.isnan(out).sum() == nodata.sum()) == (not edge_nan)
    # a mask over the no-data cells does not revive them
    out, _ = assert_accum(dp, z, edges, load, 'sum', np.ones((n, m), bool), False, 'NaN specks, every cell a stream')
    assert np.array_equal(np.isnan(out), nodata)


# ---- 6. schedules
def check_schedules():
    """(child process) the cases that differ in what the tile passes and the queue each get to do: each is compared with the
    reference, whose planes do not know about schedules -- so the bits are the same at every switch point"""
    shape, seed = TILES[1]
    for frac in (0.05, 0.10):
        for op in OPS:
            check_fractal(shape, seed, frac, op)
    levels = check_deep()
    check_circular('two_loops')
    for name in ('row_snake', 'far_pit'):
        check_field(name, thr=12.0)
    return levels


@pytest.mark.parametrize('env', [{'PYDEM_DIST_PASSES': '0'}, {'PYDEM_DIST_MIN_PER_VISIT': '0'}, {'PYDEM_DIST_PASSES': '2'}])
def test_schedules(env):
    """the queue alone, tile passes to the end, two passes then the queue (the switches are read once per process)"""
    r = run_child("from test_gpu_tree_accum import check_schedules\nprint('LEVELS', check_schedules())\nprint('CHILD-OK')", env=env, timeout=300)
    print(env, r.stdout.split('LEVELS', 1)[1].splitlines()[0])


# ---- 7. state integrity
def test_state_integrity():
    shape, seed = TILES[1]
    o, dp = make(shape, seed)                           # (a pair of this test's own)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        uca = np.array(dp.uca)
        thr = top_fraction(uca, 0.10)
        up = dp.calc_dist_up(edge_nan=False)
        net = dp.calc_stream_network(uca_threshold=thr)
        dep = dp.calc_up_dependence(net.link == 1)
        before = _snapshot(dp)
        a = dp.calc_tree_accum(random_load(shape, 1), op='min', uca_threshold=thr)
        b = dp.calc_tree_accum()
        table = dp.calc_reach_attributes(streams=uca >= thr, values=uca)
        assert np.isfinite(a).any() and np.isfinite(b).any() and table.size == net.links.size
        _same_snapshot(before, _snapshot(dp))
        assert np.array(dp.uca).tobytes() == uca.tobytes()
        assert dp.calc_dist_up(edge_nan=False).tobytes() == up.tobytes()
        dp.calc_tree_accum()
        again = dp.calc_stream_network(uca_threshold=thr)
        assert all(getattr(net, k).tobytes() == getattr(again, k).tobytes() for k in ('receiver', 'order', 'link', 'basin'))
        assert again.links.tobytes() == net.links.tobytes()
        dp.calc_tree_accum(uca_threshold=thr)
        assert dp.calc_up_dependence(net.link == 1).tobytes() == dep.tobytes()
        assert dp.calc_tree_accum().tobytes() == b.tobytes()
        _same_snapshot(before, _snapshot(dp))


# ---- 8. repeatability and memory
def test_identical_calls_and_no_growth():
    from pydem_amd import _ffi
    shape, seed = TILES[1]
    z, dp, edges = fractal_case(shape, seed)
    thr, S, ref, net = fractal_set(shape, seed, 0.10)
    load = random_load(shape, 8)
    tails = net.links['tail']
    cut = dp._tile.tree_accum(load, 'sum', None, thr, True, tails)      # (warm-up: the call's planes exist from here on)
    whole = dp._tile.tree_accum(load, 'max', None, None, False, tails)
    dp._tile.tree_accum(load, 'sum', S, None, True, tails)
    bytes0, free0 = dp._tile.device_bytes(), _ffi.device_memory(0)[0]
    for k in range(20):
        if k % 2:
            got, first = dp._tile.tree_accum(load, 'max', None, None, False, tails), whole
        elif k % 4:
            got, first = dp._tile.tree_accum(load, 'sum', None, thr, True, tails), cut
        else:
            got, first = dp._tile.tree_accum(load, 'sum', S, None, True, tails), cut
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes() and got[4] == first[4] == 0
    assert dp._tile.device_bytes() == bytes0 and _ffi.device_memory(0)[0] >= free0


# ---- 9. errors
def test_errors():
    from pydem_amd import DEMProcessor, _ffi, synth
    z = synth.fractal(64, 80, seed=2, top_shift=5, n_octaves=5)
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
    dp.run_slopes_directions()
    ones = np.ones((64, 80))
    everything = np.ones((64, 80), bool)
    for kw in (dict(), dict(streams=everything), dict(uca_threshold=900.0)):
        with pytest.raises(_ffi.HipError, match='no flow graph'):
            dp._tile.tree_accum(ones, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        v = dp.calc_tree_accum(1.0, edge_nan=False)                        # runs calc_uca first
    assert dp._has('uca') and np.isfinite(v).all() and (v >= 1.0).all() and v.sum() > v.size
    for bad in (np.nan, np.inf, -1.0):
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp._tile.tree_accum(ones, 'sum', None, bad)
    for op in (3, -1):
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp._tile.tree_accum(ones, op)
    for at in ([64 * 80], [-1], [0, 5, 64 * 80 + 7]):
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp._tile.tree_accum(ones, at=np.array(at))
    with pytest.raises(_ffi.HipError, match='error -2'):                   # no load
        _ffi.check(dp._tile.lib.pydem_tree_accum(dp._tile._h, 0, None, 0, None, 0.0, 1, None, None, 0, None, None, None, None))
    with pytest.raises(ValueError):
        dp._tile.tree_accum(np.ones((64, 79)))
    with pytest.raises(ValueError):
        dp._tile.tree_accum(ones, streams=np.ones((64, 79), bool))
    with pytest.raises(ValueError):
        dp._tile.tree_accum(ones, at=np.array([2 ** 31]))
    # the threshold is not read without a cut; an empty list gathers nothing; the last cell can be gathered
    out, vals, _, _, left = dp._tile.tree_accum(ones, 'sum', None, None, False, at=np.array([], np.int64))
    assert out.tobytes() == v.tobytes() and vals.size == 0 and left == 0   # the refused calls left the state alone
    out, vals, _, _, _ = dp._tile.tree_accum(ones, 'sum', None, None, False, at=np.array([64 * 80 - 1, 0]), download=False)
    assert out is None and vals.tolist() == [v[63, 79], v[0, 0]]
    dp._tile.upload(_ffi.ELEV, z + 1.0)                                     # the elevation changed: the graph is gone
    with pytest.raises(_ffi.HipError, match='no flow graph'):
        dp._tile.tree_accum(ones)
