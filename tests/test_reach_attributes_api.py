"""CPU tier: the table builder of DEMProcessor.calc_reach_attributes (pydem_amd/streamnet.py) on reference planes, and the
argument checks of calc_tree_accum / calc_reach_attributes that need no device."""
import inspect

import numpy as np
import pytest

from test_stream_network_ref import stream_network_ref
from test_tree_accum_ref import fractal_net, reach_table_ref, tree_accum_ref


def _dp(**kw):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=np.arange(25, dtype=float).reshape(5, 5) + 1.0, dX=2.0, dY=3.0, fill_flats=False,
                      drain_pits_path=False, **kw)
    dp.mag = np.ones((5, 5)); dp.direction = np.ones((5, 5)); dp.flats = np.zeros((5, 5), bool)   # skip the device stencil
    return dp


def _untouched(dp):
    return (dp._tile is None and dp.tree_accum is None and dp.tree_accum_stats is None and dp.reach_attributes is None
            and dp.reach_attributes_stats is None and dp.stream_network is None)


def hand_net(path, shape, pit=None):
    """(edges, network) of one stream on a grid of `shape`: path = [(row, col), ...], every cell a stream, each flowing into the next"""
    from pydem_amd import streamnet
    n, m = shape
    cells = [i * m + j for i, j in path]
    k = len(cells) - 1
    edges = (np.array(cells[:-1]), np.array(cells[1:]), np.ones(k), np.zeros(k, bool) if pit is None else np.asarray(pit, bool))
    S = np.zeros(shape, bool)
    S.ravel()[cells] = True
    ref = stream_network_ref(edges, shape, np.zeros(shape), S)
    return edges, S, streamnet.compact_network(ref.receiver, ref.order, ref.link, None)


def test_length_of_a_straight_and_a_diagonal_link():
    from pydem_amd import streamnet
    shape = (6, 7)
    elev = np.arange(42, 0, -1, dtype=np.float64).reshape(shape)
    uniform = (np.full(6, 2.0), np.full(6, 3.0))
    varying = (np.array([2.0, 2.5, 3.0, 3.5, 4.0, 4.5]), np.array([3.0, 3.1, 3.2, 3.3, 3.4, 3.5]))
    # along a row: 4 steps east in row 2
    _, _, net = hand_net([(2, j) for j in range(1, 6)], shape)
    assert net.links.size == 1 and net.links['n_cells'][0] == 5
    for (dX2, dY2), want in ((uniform, 4 * 2.0), (varying, 4 * 3.0)):
        length, drop, slope, straight = streamnet.channel_attributes(net, elev, dX2, dY2)
        assert length.tolist() == [want] and straight.tolist() == [want]
        assert drop.tolist() == [4.0] and slope.tolist() == [4.0 / want]
    # down a column: 3 steps south from row 1, each with the spacing of the row it leaves
    _, _, net = hand_net([(i, 3) for i in range(1, 5)], shape)
    for (dX2, dY2), want in ((uniform, 9.0), (varying, 3.1 + 3.2 + 3.3)):
        length, drop, slope, straight = streamnet.channel_attributes(net, elev, dX2, dY2)
        assert length.tolist() == [want] and np.allclose(straight, want, rtol=1e-15) and drop.tolist() == [21.0]
    # a diagonal: 3 steps south-east from (1, 1)
    _, _, net = hand_net([(1 + k, 1 + k) for k in range(4)], shape)
    length, _, _, straight = streamnet.channel_attributes(net, elev, *uniform)
    assert length.tolist() == [3 * np.hypot(2.0, 3.0)] and np.allclose(straight, length, rtol=1e-15)
    length, _, _, straight = streamnet.channel_attributes(net, elev, *varying)
    assert length.tolist() == [np.hypot(2.5, 3.1) + np.hypot(3.0, 3.2) + np.hypot(3.5, 3.3)]
    # (the stated formula: the mean width of rows 1..4 times the columns, the heights of rows 1..3)
    assert np.allclose(straight, np.hypot(3 * np.mean([2.5, 3.0, 3.5, 4.0]), 3.1 + 3.2 + 3.3), rtol=1e-15)
    # a bend is longer than it is straight; a pit step of any offset counts with its offset
    _, _, net = hand_net([(0, 0), (0, 1), (1, 1), (1, 5)], shape, pit=[False, False, True])
    length, _, _, straight = streamnet.channel_attributes(net, elev, *uniform)
    assert length.tolist() == [2.0 + 3.0 + 4 * 2.0] and straight.tolist() == [np.hypot(5 * 2.0, 3.0)]


def test_one_cell_links_have_no_slope_and_sources_have_magnitude_one():
    from pydem_amd import streamnet
    # 0, 1 -> 2 -> 3 on a 1 x 4 grid: the sources 0 and 1 are one-cell links, {2, 3} is the link below them
    shape = (1, 4)
    edges = (np.array([0, 1, 2]), np.array([2, 2, 3]), np.ones(3), np.zeros(3, bool))
    elev = np.array([[9.0, 8.0, 5.0, 1.0]])
    table, net = reach_table_ref(edges, shape, elev, np.ones(shape, bool), np.array([2.0]), np.array([3.0]), edge_nan=False)
    assert table.dtype == streamnet.REACH_DTYPE and table['id'].tolist() == [1, 2, 3] and net.links['head'].tolist() == [0, 1, 2]
    assert table['length'].tolist() == [0.0, 0.0, 2.0] and table['drop'].tolist() == [0.0, 0.0, 4.0]
    assert np.isnan(table['slope'][:2]).all() and table['slope'][2] == 2.0 and table['straight'].tolist() == [0.0, 0.0, 2.0]
    assert table['magnitude'].tolist() == [1.0, 1.0, 2.0] and table['local_cells'].tolist() == [1.0, 1.0, 2.0]
    assert table['local_area'].tolist() == [6.0, 6.0, 12.0] and table['total_area'].tolist() == [6.0, 6.0, 24.0]
    assert table['complete'].all()
    load = streamnet.magnitude_load(net)
    assert load.tolist() == [[1.0, 1.0, 0.0, 0.0]]


def test_the_table_on_a_fractal_tile():
    from pydem_amd import streamnet
    shape = (96, 80)
    o, edges, S, ref, net = fractal_net(shape, 5, 0.10)
    dX2, dY2 = np.linspace(28.0, 31.0, 96), np.full(96, 30.0)
    values = np.random.default_rng(4).normal(size=shape)
    table, net2 = reach_table_ref(edges, shape, o.elev, S, dX2, dY2, values, edge_nan=True)
    links = net.links
    assert table.dtype == streamnet.REACH_VALUES_DTYPE and np.array_equal(net2.links, links) and np.array_equal(table['id'], links['id'])
    # links with nothing above -- no stream cell but their own upstream of the tail along the tree -- have magnitude 1 (wherever
    # the edge rule leaves it known); "no link above through `down`" is weaker: a stream that left the stream set may come back in
    plain, _ = reach_table_ref(edges, shape, o.elev, S, dX2, dY2, None, edge_nan=False)
    above, _ = tree_accum_ref(edges, shape, o.elev, S.astype(np.float64), 'sum', None, False)
    top = above.ravel()[links['tail']] == links['n_cells']
    known = np.isfinite(table['magnitude'])
    assert top.sum() >= 20 and (plain['magnitude'][top] == 1).all() and (table['magnitude'][top & known] == 1).all()
    assert (links['order'][top] == 1).all() and (top & known).sum() >= 10
    # a link holds at least the magnitudes that enter its head through `down`, and at least 2 where any does
    total = np.zeros(links.size + 1)
    feeds = links['down'] > 0
    np.add.at(total, links['down'][feeds], plain['magnitude'][feeds])
    fed = total[1:] > 0
    assert plain['complete'].all() and (plain['magnitude'] >= total[1:]).all() and (total[1:][fed] >= 2).all() and not (fed & top).any()
    assert np.array_equal(plain['local_cells'], np.bincount(net.basin.ravel(), minlength=links.size + 1)[1:])
    # columns hang together
    one = links['n_cells'] == 1
    assert one.any() and np.isnan(table['slope'][one]).all() and (table['length'][one] == 0).all()
    with np.errstate(invalid='ignore'):
        assert (table['length'][~one] > 0).all() and np.array_equal(table['slope'][~one], (table['drop'] / table['length'])[~one])
    zf = np.asarray(o.elev, np.float64).ravel()
    assert np.array_equal(table['drop'], zf[links['head']] - zf[links['tail']])
    assert np.array_equal(table['complete'], np.isfinite(table['local_area'])) and 0 < table['complete'].sum() < links.size
    ok = table['complete']
    assert np.array_equal(table['v_mean'][ok], (table['v_sum'] / table['local_cells'])[ok])
    assert (table['v_min'][ok] <= table['v_mean'][ok]).all() and (table['v_mean'][ok] <= table['v_max'][ok]).all()
    assert (plain['total_area'] >= plain['local_area']).all()


def test_reach_table_refuses_incomplete_input():
    from pydem_amd import streamnet
    _, _, net = hand_net([(0, 0), (0, 1)], (2, 3))
    cols = {k: np.ones(1) for k in streamnet.DEVICE_COLUMNS}
    assert streamnet.reach_table(net, np.zeros((2, 3)), np.ones(2), np.ones(2), cols).size == 1
    with pytest.raises(ValueError):
        streamnet.reach_table(net, np.zeros((2, 3)), np.ones(2), np.ones(2), {k: v for k, v in cols.items() if k != 'magnitude'})
    with pytest.raises(ValueError):
        streamnet.reach_table(net, np.zeros((2, 3)), np.ones(2), np.ones(2), dict(cols, v_sum=np.ones(1)))
    with pytest.raises(ValueError):
        streamnet.reach_table(net, np.zeros((2, 3)), np.ones(2), np.ones(2), dict(cols, magnitude=np.ones(2)))


def test_methods_and_attributes_exist():
    from pydem_amd import DEMProcessor, _ffi
    sigs = {'calc_tree_accum': [('weights', None), ('op', 'sum'), ('streams', None), ('uca_threshold', None), ('edge_nan', True)],
            'calc_reach_attributes': [('uca_threshold', None), ('streams', None), ('values', None), ('edge_nan', True)]}
    for name, want in sigs.items():
        assert callable(getattr(DEMProcessor, name, None)), name
        sig = inspect.signature(getattr(DEMProcessor, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == want
    assert 'pydem_tree_accum' in _ffi.SYMBOLS and callable(_ffi.Tile.tree_accum)
    assert _untouched(_dp())


@pytest.mark.parametrize('kw', [dict(op='mean'), dict(op=0), dict(uca_threshold=10.0, streams=np.ones((5, 5), bool)),
                                dict(streams=np.ones((5, 4), bool)), dict(streams=True), dict(uca_threshold=-1.0),
                                dict(uca_threshold=np.nan), dict(uca_threshold=np.inf), dict(uca_threshold='x'),
                                dict(weights=np.ones((5, 4))), dict(weights=np.nan), dict(weights=np.full((5, 5), np.inf))])
def test_tree_accum_refuses_bad_arguments_before_device_work(kw):
    dp = _dp()
    kw = dict(kw)
    with pytest.raises(ValueError):
        dp.calc_tree_accum(kw.pop('weights', 1.0), **kw)
    assert _untouched(dp)


@pytest.mark.parametrize('kw', [dict(), dict(uca_threshold=10.0, streams=np.ones((5, 5), bool)), dict(streams=np.ones((5, 4), bool)),
                                dict(uca_threshold=-1.0), dict(uca_threshold=np.nan), dict(uca_threshold='x'),
                                dict(uca_threshold=12.0, values=np.ones((5, 4))), dict(uca_threshold=12.0, values='x')])
def test_reach_attributes_refuses_bad_arguments_before_device_work(kw):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_reach_attributes(**kw)
    assert _untouched(dp)


@pytest.mark.parametrize('kw', [dict(drain_flats=True), dict(drain_pits_spill=True)])
def test_unimplemented_drainage_alternatives_fail_loudly(kw):
    dp = _dp(drain_pits=False, **kw)
    with pytest.raises(NotImplementedError):
        dp.calc_tree_accum(1.0)
    with pytest.raises(NotImplementedError):
        dp.calc_reach_attributes(uca_threshold=12.0)
    with pytest.raises(ValueError):                                     # the argument checks still come first
        dp.calc_reach_attributes()
    assert _untouched(dp)


def test_no_cpu_fallback():
    """HipError where no GPU is visible; where one is, the calls compute the flow graph first and are served by the device."""
    from pydem_amd import _ffi, streamnet
    try:
        n = _ffi.device_count()
    except _ffi.HipError:
        n = 0
    dp = _dp()
    if n == 0:
        with pytest.raises(_ffi.HipError):
            dp.calc_tree_accum()
        with pytest.raises(_ffi.HipError):
            dp.calc_reach_attributes(uca_threshold=12.0)
        assert dp.tree_accum is None and dp.reach_attributes is None
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            acc = dp.calc_tree_accum(edge_nan=False)
            table = dp.calc_reach_attributes(uca_threshold=12.0)
        assert dp._has('uca') and acc.shape == (5, 5) and acc.dtype == np.float64 and acc is dp.tree_accum
        assert set(dp.tree_accum_stats) == {'ms', 'levels', 'n_unresolved', 'edge_nan', 'cut'} and not dp.tree_accum_stats['cut']
        assert table is dp.reach_attributes and table.dtype == streamnet.REACH_DTYPE and table.size == dp.stream_network.links.size
        assert set(dp.reach_attributes_stats) == {'ms', 'sweeps', 'edge_nan', 'n_links'}
