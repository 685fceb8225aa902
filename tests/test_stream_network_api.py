"""CPU tier: the stream network (DEMProcessor.calc_flow_receiver / calc_stream_network, pydem_stream_network) is part of the
public surface and of the C-ABI, refuses bad input before any device work, and its host side -- the compaction of the raw
labels to link ids and the table of links (pydem_amd/streamnet.py) -- is right on planes produced by the reference."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_stream_network_ref import fractal_oracle, line, oracle_edges, stream_network_ref, top_fraction


def _dp(**kw):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=np.arange(25, dtype=float).reshape(5, 5) + 1.0, dX=2.0, dY=3.0, fill_flats=False,
                      drain_pits_path=False, **kw)
    dp.mag = np.ones((5, 5)); dp.direction = np.ones((5, 5)); dp.flats = np.zeros((5, 5), bool)   # skip the device stencil
    return dp


def _untouched(dp):
    return dp._tile is None and dp.flow_receiver is None and dp.stream_network is None and dp.stream_network_stats is None


def test_methods_and_attributes_exist():
    from pydem_amd import DEMProcessor
    sigs = {'calc_flow_receiver': [],
            'calc_stream_network': [('uca_threshold', None), ('streams', None), ('basins', True)]}
    for name, want in sigs.items():
        assert callable(getattr(DEMProcessor, name, None)), name
        sig = inspect.signature(getattr(DEMProcessor, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == want
    assert _untouched(_dp())


@pytest.mark.parametrize('kw', [dict(), dict(uca_threshold=10.0, streams=np.ones((5, 5), bool)), dict(streams=np.ones((5, 4), bool)),
                                dict(streams=np.ones(25, bool)), dict(streams=True), dict(uca_threshold=-1.0),
                                dict(uca_threshold=np.nan), dict(uca_threshold=np.inf), dict(uca_threshold='x')])
def test_bad_arguments_are_refused_before_device_work(kw):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_stream_network(**kw)
    assert _untouched(dp)


@pytest.mark.parametrize('kw', [dict(drain_flats=True), dict(drain_pits_spill=True)])
def test_unimplemented_drainage_alternatives_fail_loudly(kw):
    dp = _dp(drain_pits=False, **kw)
    with pytest.raises(NotImplementedError):
        dp.calc_flow_receiver()
    with pytest.raises(NotImplementedError):
        dp.calc_stream_network(uca_threshold=12.0)
    with pytest.raises(ValueError):                                     # the argument checks still come first
        dp.calc_stream_network()
    assert _untouched(dp)


def test_implicit_run_uca_and_no_cpu_fallback():
    """HipError where no GPU is visible; where one is, the calls compute the flow graph first and are served by the device."""
    from pydem_amd import _ffi, streamnet
    try:
        n = _ffi.device_count()
    except _ffi.HipError:
        n = 0
    dp = _dp()
    if n == 0:
        with pytest.raises(_ffi.HipError):
            dp.calc_flow_receiver()
        with pytest.raises(_ffi.HipError):
            dp.calc_stream_network(uca_threshold=12.0)
        assert dp.flow_receiver is None and dp.stream_network is None and dp.stream_network_stats is None
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            recv = dp.calc_flow_receiver()
            net = dp.calc_stream_network(uca_threshold=12.0)
        assert dp._has('uca')                                              # the implicit run_uca()
        assert recv.dtype == np.int32 and recv.shape == (5, 5) and np.array_equal(recv, net.receiver)
        assert isinstance(net, streamnet.StreamNetwork) and net is dp.stream_network and dp.flow_receiver is net.receiver
        assert set(dp.stream_network_stats) == {'ms', 'levels', 'n_unresolved', 'n_links', 'max_order'}


def test_header_declares_the_export():
    text = open(os.path.join(ROOT, 'include', 'pydem_hip.h')).read()
    assert re.search(r'int\s+pydem_stream_network\s*\(\s*pydem_tile\s*\*\s*t\s*,\s*const\s+uint8_t\s*\*\s*streams[^;]*double\s+uca_threshold'
                     r'[^;]*int32_t\s*\*\s*receiver\s*,\s*int32_t\s*\*\s*order\s*,\s*int32_t\s*\*\s*link\s*,\s*int32_t\s*\*\s*basin[^;]*double\s*\*\s*ms'
                     r'[^;]*int64_t\s+levels\[2\][^;]*int64_t\s+n_unresolved\[2\][^;]*\)\s*;', text)
    assert re.search(r'^ \*   pydem_stream_network\s', text, re.M)          # the list at the top of the header
    from pydem_amd import _ffi
    assert 'pydem_stream_network' in _ffi.SYMBOLS
    assert len(_ffi.SYMBOLS['pydem_stream_network'][1]) == 10
    sig = inspect.signature(_ffi.Tile.stream_network)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ('streams', None), ('uca_threshold', None), ('receiver', True), ('order', True), ('link', True), ('basin', True)]


def test_library_exports_the_symbol():
    from pydem_amd import _ffi
    assert hasattr(_ffi.load(), 'pydem_stream_network')


# ---- the host side, on planes of the reference
def check_network(net, ref, S):
    """a StreamNetwork against the raw planes `ref` it was compacted from"""
    links = net.links
    K = links.size
    heads = np.unique(ref.link[ref.link > 0]) - 1
    assert K == heads.size and np.array_equal(links['id'], np.arange(1, K + 1)) and np.array_equal(links['head'], heads)
    assert (np.diff(links['head']) > 0).all()
    lf, rf, of = net.link.ravel(), net.receiver.ravel(), net.order.ravel()
    # the ids name the same partition as the raw labels; 0 and -1 stay
    assert np.array_equal(net.link > 0, ref.link > 0) and np.array_equal(net.link == -1, ref.link == -1)
    assert np.array_equal(links['head'][lf[lf > 0] - 1] + 1, ref.link.ravel()[lf > 0])
    assert np.array_equal(lf[links['head']], links['id']) and np.array_equal(lf[links['tail']], links['id'])
    assert np.array_equal(links['n_cells'], np.bincount(lf[lf > 0], minlength=K + 1)[1:]) and links['n_cells'].sum() == (lf > 0).sum()
    assert np.array_equal(links['order'], of[links['head']])
    if net.basin is not None:
        bf = net.basin.ravel()
        assert np.array_equal(net.basin > 0, ref.basin > 0) and np.array_equal(net.basin == -1, ref.basin == -1)
        assert np.array_equal(links['head'][bf[bf > 0] - 1] + 1, ref.basin.ravel()[bf > 0])
    # the tail's receiver leaves the link; down names where it lands
    rt = rf[links['tail']]
    want = np.where(rt >= 0, lf[np.maximum(rt, 0)], 0)
    assert np.array_equal(links['down'], want) and (links['down'] != links['id']).all()
    return links


def test_compaction_and_links_table_on_a_fractal_tile():
    from pydem_amd import streamnet
    shape = (96, 80)
    o = fractal_oracle(shape, 5)
    S = np.asarray(o.uca) >= top_fraction(o.uca, 0.10)
    ref = stream_network_ref(oracle_edges(o), shape, o.elev, S)
    net = streamnet.compact_network(ref.receiver, ref.order, ref.link, ref.basin)
    assert all(x.dtype == np.int32 and x.shape == shape for x in (net.receiver, net.order, net.link, net.basin))
    links = check_network(net, ref, S)
    assert links.dtype.names == ('id', 'head', 'tail', 'order', 'n_cells', 'down') and links.size >= 50
    assert (links['n_cells'] > 1).any() and (links['down'] > 0).any() and (links['down'] == 0).any()
    # walking the receivers from the head reaches the tail in n_cells - 1 steps, inside the link
    rf, lf = net.receiver.ravel(), net.link.ravel()
    for row in links[:: max(1, links.size // 25)]:
        c = int(row['head'])
        for _ in range(int(row['n_cells']) - 1):
            c = int(rf[c])
            assert lf[c] == row['id']
        assert c == row['tail']
    without = streamnet.compact_network(ref.receiver, ref.order, ref.link, None)
    assert without.basin is None and np.array_equal(without.link, net.link) and np.array_equal(without.links, links)


def test_compaction_keeps_unresolved_cells_and_names_what_flows_into_them():
    from pydem_amd import streamnet
    # 0 -> 1 -> 2 <-> 3 (loop), 4 -> 5: the link of 0 ends at 1, whose receiver is unresolved
    ref = line([(0, 1), (1, 2), (2, 3), (3, 2), (4, 5)], 6)
    assert ref.link[0].tolist() == [1, 1, -1, -1, 5, 5]
    net = streamnet.compact_network(ref.receiver, ref.order, ref.link, ref.basin)
    assert net.link[0].tolist() == [1, 1, -1, -1, 2, 2] and net.basin[0].tolist() == [1, 1, -1, -1, 2, 2]
    assert net.links.tolist() == [(1, 0, 1, 1, 2, -1), (2, 4, 5, 1, 2, 0)]
    check_network(net, ref, np.ones((1, 6), bool))
    # no streams at all: an empty table
    ref = line([(0, 1)], 2, S=np.zeros((1, 2), bool))
    net = streamnet.compact_network(ref.receiver, ref.order, ref.link, ref.basin)
    assert net.links.size == 0 and not net.link.any() and not net.basin.any()
