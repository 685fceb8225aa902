"""CPU tier: the reference of the receiver-tree accumulation (DEMProcessor.calc_tree_accum / calc_reach_attributes,
pydem_tree_accum), pinned by itself.  tests/test_gpu_tree_accum.py holds the device against it.

tree_accum_ref(edges, shape, elev, load, op, S, edge_nan) is the contract of include/pydem_hip.h as a plain Kahn sweep over an
edge list edges = (src, dst, w, is_pit), on the receivers and the inflow counts of stream_network_ref:
    the tree in-neighbours of c: the u with recv[u] == c, each once, in ascending u;
    S (None: empty, the whole tree) without the NaN elevations; c continues a link when it is in S and has exactly one stream inflow;
    c takes the tree edge u -> c unless u is in S and c does not continue a link;
    V = NaN on NaN elevations and, with edge_nan, on the border and beside a NaN elevation: final from the start; V = load where
    no graph edge enters; every other cell waits for ALL its graph in-neighbours, then
        sum: acc = 0.0; acc += V[u] in ascending u; V = load + acc      max / min: a = load; a = V[u] if V[u] > a (< a) else a
    NaN if any operand is NaN; cells that never become ready are NaN and counted.
The operations and their order are the device's, so the device tests compare bytes."""
import collections
import functools

import numpy as np
import pytest

from test_dist_up_ref import edge_nan_cells
from test_stream_network_ref import fractal_oracle, hand_graph, line, oracle_edges, stream_network_ref, top_fraction

OPS = ('sum', 'max', 'min')


def tree_accum_ref(edges, shape, elev, load, op='sum', S=None, edge_nan=False, net=None):
    """(V [n, m] float64, n_unresolved).  net: the stream_network_ref of the same edges, elevation and S, if the caller has it."""
    n, m = shape
    NN = n * m
    elev = np.asarray(elev, np.float64).reshape(n, m)
    if S is None:
        S = np.zeros(shape, bool)
    if net is None:
        net = stream_network_ref(edges, shape, elev, S)
    nodata = np.isnan(elev).ravel()
    Sf = (np.asarray(S, bool).ravel() & ~nodata).tolist()
    recv = net.receiver.ravel().astype(np.int64)
    cont = (np.asarray(Sf) & (net.n_inflow.ravel() == 1)).tolist()
    tree_in = [[] for _ in range(NN)]
    for u in np.flatnonzero(recv >= 0).tolist():                          # (ascending u)
        tree_in[recv[u]].append(u)
    src, dst = np.asarray(edges[0], np.int64), np.asarray(edges[1], np.int64)
    outs = [[] for _ in range(NN)]
    for a, b in zip(src.tolist(), dst.tolist()):
        outs[a].append(b)
    cnt = np.bincount(dst, minlength=NN).astype(np.int64)
    ld = np.asarray(load, np.float64).ravel().tolist()
    nan_start = (edge_nan_cells(elev) if edge_nan else np.isnan(elev)).ravel()
    V = np.full(NN, np.nan)
    final = nan_start | (cnt == 0)
    start = np.flatnonzero(final & ~nan_start)
    V[start] = np.asarray(ld)[start]
    V = V.tolist()
    final = final.tolist()
    nan = float('nan')
    queue = collections.deque(np.flatnonzero(np.asarray(final)).tolist())
    while queue:
        v = queue.popleft()
        for c in outs[v]:
            cnt[c] -= 1
            if cnt[c] == 0 and not final[c]:
                taken = [V[u] for u in tree_in[c] if cont[c] or not Sf[u]]
                assert all(final[u] for u in tree_in[c])
                if op == 'sum':
                    acc = 0.0
                    for x in taken:
                        acc += x
                    r = ld[c] + acc
                else:
                    r = ld[c]
                    bad = r != r
                    for x in taken:
                        bad = bad or x != x
                        if op == 'max':
                            r = x if x > r else r
                        else:
                            r = x if x < r else r
                    if bad:
                        r = nan
                V[c] = r
                final[c] = True
                queue.append(c)
    V = np.array(V, np.float64)
    left = ~np.asarray(final)
    V[left] = np.nan
    V[np.isnan(V)] = np.nan                                                # (one NaN pattern: numpy's, which is the device's)
    return V.reshape(n, m), int(left.sum())


def reach_table_ref(edges, shape, elev, S, dX2, dY2, values=None, edge_nan=True):
    """(the table calc_reach_attributes has to return, the compacted reference network): the catchment columns from
    tree_accum_ref at the link tails, put together by the product's own streamnet.reach_table"""
    from pydem_amd import streamnet
    ref = stream_network_ref(edges, shape, elev, S)
    net = streamnet.compact_network(ref.receiver, ref.order, ref.link, None)
    tails = net.links['tail']
    area = np.broadcast_to((np.asarray(dX2, np.float64) * np.asarray(dY2, np.float64))[:, None], shape)
    sweeps = [('local_cells', np.ones(shape), 'sum', S), ('local_area', area, 'sum', S), ('total_area', area, 'sum', None),
              ('magnitude', streamnet.magnitude_load(net), 'sum', None)]
    if values is not None:
        sweeps += [('v_sum', values, 'sum', S), ('v_min', values, 'min', S), ('v_max', values, 'max', S)]
    at = {}
    for name, load, op, cut in sweeps:
        V, _ = tree_accum_ref(edges, shape, elev, load, op, cut, edge_nan, net=ref if cut is not None else None)
        at[name] = V.ravel()[tails]
    return streamnet.reach_table(net, elev, dX2, dY2, at), net


def line_accum(edges, n_cells, load=None, op='sum', S=None, w=None, pit=None, elev=None):
    """tree_accum_ref on the hand graph of test_stream_network_ref.line: a 1 x n_cells grid, edges = [(src, dst), ...]"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.ones(len(e)) if w is None else np.asarray(w, np.float64)
    pit = np.zeros(len(e), bool) if pit is None else np.asarray(pit, bool)
    elev = np.zeros((1, n_cells)) if elev is None else elev
    load = np.ones((1, n_cells)) if load is None else np.asarray(load, np.float64).reshape(1, n_cells)
    V, left = tree_accum_ref((e[:, 0], e[:, 1], w, pit), (1, n_cells), elev, load, op, S, False)
    return V[0].tolist(), left


ALL = lambda k: np.ones((1, k), bool)


def test_perfect_binary_tree():
    """node k flows into (k - 1) // 2.  Whole tree: the size of the subtree.  Every node a stream: every node is a junction or a
    source, so every link is one cell and holds only itself."""
    edges = [(k, (k - 1) // 2) for k in range(1, 15)]
    V, left = line_accum(edges, 15)
    depth = np.floor(np.log2(np.arange(15) + 1)).astype(int)
    assert V == (2.0 ** (4 - depth) - 1).tolist() and left == 0
    assert line_accum(edges, 15, S=ALL(15)) == ([1.0] * 15, 0)
    # only the leaves off the streams: a leaf is taken by its parent, a stream node by nobody (every stream node has 0 or 2 inflows)
    S = (np.arange(15) < 7)[None, :]
    V, _ = line_accum(edges, 15, S=S)
    assert V == [1.0, 1.0, 1.0, 3.0, 3.0, 3.0, 3.0] + [1.0] * 8
    # max and min of the load k over the subtree
    load = np.arange(15.0)
    assert line_accum(edges, 15, load, 'min')[0] == load.tolist()
    assert line_accum(edges, 15, load, 'max')[0] == [14.0, 10.0, 14.0, 8.0, 10.0, 12.0, 14.0] + load[7:].tolist()


def test_a_chain_joining_a_trunk_and_three_inflows():
    # 0, 1 -> 2 -> 3 <- 4 <- 5 ; 3 -> 6.  Links (every cell a stream): {0}, {1}, {2}, {3, 6}, {5, 4}
    edges = [(0, 2), (1, 2), (2, 3), (5, 4), (4, 3), (3, 6)]
    assert line_accum(edges, 7)[0] == [1.0, 1.0, 3.0, 6.0, 2.0, 1.0, 7.0]
    assert line_accum(edges, 7, S=ALL(7))[0] == [1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 2.0]    # the chain 5 -> 4 and 3 -> 6 go on; junctions cut
    # negative loads, and the order of the sum: ascending source
    load = [0.1, -0.7, 0.3, 1e16, -1e16, 2.0, 0.5]
    V, _ = line_accum(edges, 7, load)
    assert V[2] == 0.3 + ((0.0 + 0.1) + -0.7) and V[4] == -1e16 + (0.0 + 2.0)
    assert V[3] == 1e16 + ((0.0 + V[2]) + V[4]) and V[6] == 0.5 + (0.0 + V[3])
    assert line_accum(edges, 7, load, 'max')[0] == [0.1, -0.7, 0.3, 1e16, 2.0, 2.0, 1e16]
    assert line_accum(edges, 7, load, 'min')[0] == [0.1, -0.7, -0.7, -1e16, -1e16, 2.0, -1e16]
    assert line_accum(edges, 7, load, 'min', S=ALL(7))[0] == [0.1, -0.7, 0.3, 1e16, -1e16, 2.0, 0.5]
    # three inflows into one cell: nothing is taken under the cut, everything without
    edges = [(0, 3), (1, 3), (2, 3)]
    assert line_accum(edges, 4)[0] == [1.0, 1.0, 1.0, 4.0] and line_accum(edges, 4, S=ALL(4))[0] == [1.0] * 4
    # one of the three off the streams: it is taken, the two stream inflows are not
    assert line_accum(edges, 4, S=np.array([[True, False, True, True]]))[0] == [1.0, 1.0, 1.0, 2.0]


def test_a_stream_that_leaves_S_and_reenters_it():
    # 0 -> 1 -> 2 -> 3 -> 4 -> 5 with S = {1, 2, 5}: link {1, 2} ends where 3 is off S; 3, 4 drain to link {5}
    edges = [(k, k + 1) for k in range(5)]
    S = np.array([[False, True, True, False, False, True]])
    assert line_accum(edges, 6, S=S)[0] == [1.0, 2.0, 3.0, 1.0, 2.0, 3.0]
    assert line_accum(edges, 6)[0] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    net = line(edges, 6, S=S)
    assert np.array_equal(np.bincount(net.basin[0])[[2, 6]], [3, 3])                    # the tails hold the basins' cell counts


def test_tie_cases():
    # equal weights: the lower destination is the receiver, the other edge is a graph edge only -- cell 2 still waits for 1
    V, _ = line_accum([(1, 2), (1, 0)], 3, w=[0.5, 0.5])
    assert V == [2.0, 1.0, 1.0]
    V, _ = line_accum([(1, 2), (1, 0)], 3, w=[0.5 + 1e-12, 0.5])
    assert V == [1.0, 1.0, 2.0]
    # two entries from one source to one cell: the source counts once, whichever edge is the receiver
    assert line_accum([(0, 1), (0, 1)], 2, w=[0.5, 0.5], pit=[True, False])[0] == [1.0, 2.0]
    assert line_accum([(0, 1), (0, 1)], 2, w=[0.5 + 1e-12, 0.5], pit=[True, False])[0] == [1.0, 2.0]
    assert line_accum([(0, 1), (0, 1)], 2, w=[0.5, 0.5], pit=[True, True], S=ALL(2))[0] == [1.0, 2.0]
    # the tree is not the graph: 0 -> 1 (heavier) and 0 -> 2; 1 -> 2.  2 takes 1 (which holds 0) but not 0 again
    assert line_accum([(0, 1), (0, 2), (1, 2)], 3, w=[0.6, 0.4, 1.0])[0] == [1.0, 2.0, 3.0]
    assert line_accum([(0, 1), (0, 2), (1, 2)], 3, w=[0.4, 0.6, 1.0])[0] == [1.0, 1.0, 3.0]


def test_cycles_are_nan_and_counted():
    o = hand_graph()                                                      # 0 -> 1 <-> 2 (loop);  3 -> 4 -> 5
    V, left = tree_accum_ref(oracle_edges(o), (1, 6), o.elev, np.ones((1, 6)), 'sum', None, False)
    assert np.array_equal(np.isnan(V[0]), [False, True, True, False, False, False]) and left == 2
    assert V[0, [0, 3, 4, 5]].tolist() == [1.0, 1.0, 2.0, 3.0]
    # what lies downstream of the loop: 0 -> 1 <-> 2, 2 -> 3 -> 4 with the smaller weight
    for op in OPS:
        V, left = line_accum([(0, 1), (1, 2), (2, 1), (2, 3), (3, 4)], 5, op=op, w=[1, 1, 0.6, 0.4, 1])
        assert np.array_equal(np.isnan(V), [False, True, True, True, True]) and left == 4
    # readiness is the graph's, not the tree's: 3 -> 4 is no receiver edge (3 -> 2 is heavier), but 4 waits for 3, which waits
    # for the loop
    V, left = line_accum([(0, 1), (1, 2), (2, 1), (2, 3), (3, 2), (3, 4)], 5, w=[1, 1, 0.6, 0.4, 0.7, 0.3])
    assert np.isnan(V[4]) and left == 4


def test_nan_cells_and_the_cut_that_stops_them():
    elev = np.zeros((1, 5)); elev[0, 1] = np.nan
    # 0 -> 1(NaN) -> 2 -> 3 -> 4: the NaN cell has no receiver, so it reaches nobody along the tree, but 2 waited for it
    e = ([0, 1, 2, 3], [1, 2, 3, 4], [1.0] * 4, [False] * 4)
    V, left = tree_accum_ref(e, (1, 5), elev, np.ones((1, 5)), 'sum', None, False)
    assert np.isnan(V[0, 1]) and V[0, [0, 2, 3, 4]].tolist() == [1.0, 1.0, 2.0, 3.0] and left == 0
    # a NaN value upstream, carried by a taken edge: everything below is NaN without a cut; with every cell a stream the
    # junction at 3 cuts it off
    edges = [(0, 1), (1, 3), (2, 3), (3, 4)]
    load = [np.nan, 1.0, 1.0, 1.0, 1.0]
    for op in OPS:
        V, _ = line_accum(edges, 5, load, op)
        assert np.array_equal(np.isnan(V), [True, True, False, True, True])
        V, _ = line_accum(edges, 5, load, op, S=ALL(5))
        assert np.array_equal(np.isnan(V), [True, True, False, False, False])
    # a mask over a NaN elevation does not make it a stream: 0 is 2's only stream inflow, so 2 continues 0's link
    elev = np.zeros((1, 4)); elev[0, 1] = np.nan
    e = ([0, 1, 2], [2, 2, 3], [1.0] * 3, [False] * 3)
    V, _ = tree_accum_ref(e, (1, 4), elev, np.ones((1, 4)), 'sum', np.ones((1, 4), bool), False)
    assert V[0, [0, 2, 3]].tolist() == [1.0, 2.0, 3.0] and np.isnan(V[0, 1])


# ---- the oracle's fractal tiles
@functools.lru_cache(maxsize=None)
def fractal_net(shape, seed, frac):
    o = fractal_oracle(shape, seed)
    edges = oracle_edges(o)
    S = np.asarray(o.uca) >= top_fraction(o.uca, frac)
    from pydem_amd import streamnet
    ref = stream_network_ref(edges, shape, o.elev, S)
    return o, edges, S, ref, streamnet.compact_network(ref.receiver, ref.order, ref.link, ref.basin)


def finite_below_nan(links, at_tails):
    """links whose value is finite though a link directly above them (through `down`) is NaN"""
    K = links.size
    bad_above = np.zeros(K + 1, bool)
    feeds = links[links['down'] > 0]
    bad_above[feeds['down'][np.isnan(at_tails[feeds['id'] - 1])]] = True
    return int((np.isfinite(at_tails) & bad_above[1:]).sum())


def test_fractal_tile_cut_counts_are_the_basins():
    shape = (300, 260)
    o, edges, S, ref, net = fractal_net(shape, 5, 0.05)
    tails = net.links['tail']
    ones = np.ones(shape)
    cut, left = tree_accum_ref(edges, shape, o.elev, ones, 'sum', S, False, net=ref)
    assert left == 0 and net.links.size >= 1000
    assert np.array_equal(cut.ravel()[tails], np.bincount(net.basin.ravel(), minlength=net.links.size + 1)[1:])
    whole, left = tree_accum_ref(edges, shape, o.elev, ones, 'sum', None, False)
    nodata = np.isnan(np.asarray(o.elev, np.float64))
    assert left == 0 and whole[(ref.receiver < 0) & ~nodata].sum() == (~nodata).sum()
    assert (whole.ravel()[tails] >= cut.ravel()[tails]).all()
    # the edge rule: the cut stops the contamination at the link boundaries
    cut_e, _ = tree_accum_ref(edges, shape, o.elev, ones, 'sum', S, True, net=ref)
    whole_e, _ = tree_accum_ref(edges, shape, o.elev, ones, 'sum', None, True)
    a, b = cut_e.ravel()[tails], whole_e.ravel()[tails]
    below = finite_below_nan(net.links, a)
    print("links %d, finite under the cut %d, finite on the whole tree %d, finite below a NaN link %d"
          % (tails.size, np.isfinite(a).sum(), np.isfinite(b).sum(), below))
    assert below >= 10 and np.isfinite(a).sum() > np.isfinite(b).sum()
    fin = np.isfinite(a)
    assert np.array_equal(a[fin], cut.ravel()[tails][fin])                # where it is finite it is the whole sub-basin


def test_small_fractal_tile_finite_below_nan():
    shape = (96, 80)
    o, edges, S, ref, net = fractal_net(shape, 5, 0.10)
    cut_e, _ = tree_accum_ref(edges, shape, o.elev, np.ones(shape), 'sum', S, True, net=ref)
    below = finite_below_nan(net.links, cut_e.ravel()[net.links['tail']])
    print("links %d, finite below a NaN link %d" % (net.links.size, below))
    assert below >= 5


@pytest.mark.parametrize('op', ['max', 'min'])
def test_fractal_tile_extremes_against_the_basins(op):
    shape = (96, 80)
    o, edges, S, ref, net = fractal_net(shape, 5, 0.10)
    load = np.random.default_rng(11).normal(size=shape)
    V, _ = tree_accum_ref(edges, shape, o.elev, load, op, S, False, net=ref)
    want = np.full(net.links.size + 1, -np.inf if op == 'max' else np.inf)
    (np.maximum if op == 'max' else np.minimum).at(want, net.basin.ravel(), load.ravel())
    assert np.array_equal(V.ravel()[net.links['tail']], want[1:])
