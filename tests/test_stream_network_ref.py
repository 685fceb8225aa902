"""CPU tier: the reference of the stream network (DEMProcessor.calc_flow_receiver / calc_stream_network, pydem_stream_network),
pinned by itself.  tests/test_gpu_stream_network.py holds the device against it.

stream_network_ref(edges, shape, elev, S) is the definitions of include/pydem_hip.h as plain Kahn sweeps over an edge list
edges = (src, dst, w, is_pit):
    the out-edges of a cell in ascending destination order, a regular edge before a pit edge to the same cell;
    recv = the destination of the first out-edge of greatest weight in that order, -1 without an out-edge or on a NaN elevation;
    S without the NaN elevations; the stream inflows of c in S: the u in S with recv[u] == c, each once;
    forward (a cell of S waits for ALL its in-neighbours; the cells off S are final from the start): order 1 and its own link
    without a stream inflow; with exactly one, that inflow's order and link; otherwise M + 1 if two or more inflows have the
    greatest order M, else M, and its own link (raw label: head cell + 1); cells that never become ready hold -1 and are counted;
    reverse (a cell off S waits for ALL its out-neighbours; the cells of S, the NaN elevations and the cells without an
    out-edge are final from the start): basin = link on S, 0 without a receiver, basin[recv] otherwise; -1 where a cell never
    becomes ready; the cells whose basin is -1 are counted."""
import collections

import numpy as np

from test_rev_accum_ref import fractal_oracle, hand_graph

Net = collections.namedtuple('Net', 'receiver code order link basin n_inflow n_unresolved')
NB = {(-1, -1): 0, (-1, 0): 1, (-1, 1): 2, (0, -1): 3, (0, 1): 4, (1, -1): 5, (1, 0): 6, (1, 1): 7}


def stream_network_ref(edges, shape, elev, S):
    """Net of planes of `shape`: receiver (flat cell or -1), code (0..7 the neighbour direction NW N NE W E SW S SE, 8 a pit
    edge, 255 none), order, link and basin (raw labels), n_inflow (stream inflows of the cells of S), and n_unresolved =
    (forward, reverse)."""
    n, m = shape
    NN = n * m
    src, dst, w, is_pit = (np.asarray(x) for x in edges)
    src, dst, is_pit = src.astype(np.int64), dst.astype(np.int64), is_pit.astype(bool)
    k = np.lexsort((is_pit, dst, src))
    src, dst, w, is_pit = src[k], dst[k], np.asarray(w, np.float64)[k], is_pit[k]
    nodata = np.isnan(np.asarray(elev, np.float64)).ravel()
    S = np.asarray(S, bool).ravel() & ~nodata
    # the first out-edge of greatest weight per source
    k = np.lexsort((np.arange(src.size), -w, src))
    first = k[np.r_[True, src[k][1:] != src[k][:-1]]] if src.size else k
    first = first[~nodata[src[first]]]
    recv = np.full(NN, -1, np.int64)
    code = np.full(NN, 255, np.int64)
    recv[src[first]] = dst[first]
    di, dj = dst[first] // m - src[first] // m, dst[first] % m - src[first] % m
    # (hand graphs: an edge between two cells that are not neighbours reads as a pit edge)
    code[src[first]] = [8 if p else NB.get((a, b), 8) for p, a, b in zip(is_pit[first].tolist(), di.tolist(), dj.tolist())]
    outs, ins = [[] for _ in range(NN)], [[] for _ in range(NN)]
    for a, b in zip(src.tolist(), dst.tolist()):
        outs[a].append(b)
        ins[b].append(a)
    inflows = [[] for _ in range(NN)]
    for u in np.flatnonzero(S & (recv >= 0)).tolist():
        if S[recv[u]]:
            inflows[recv[u]].append(u)
    # forward
    order, link = np.zeros(NN, np.int64), np.zeros(NN, np.int64)
    cnt = np.array([len(x) for x in ins], np.int64)
    final = ~S | (cnt == 0)
    heads = np.flatnonzero(S & (cnt == 0))
    order[heads], link[heads] = 1, heads + 1
    queue = collections.deque(np.flatnonzero(final).tolist())
    while queue:
        v = queue.popleft()
        for c in outs[v]:
            cnt[c] -= 1
            if cnt[c] == 0 and not final[c]:
                ords = [order[u] for u in inflows[c]]
                assert all(final[u] for u in inflows[c])
                if len(ords) == 1:
                    order[c], link[c] = ords[0], link[inflows[c][0]]
                else:
                    hi = max(ords) if ords else 0
                    order[c], link[c] = (hi + 1 if ords.count(hi) >= 2 else hi) if ords else 1, c + 1
                final[c] = True
                queue.append(c)
    order[~final], link[~final] = -1, -1
    left_fwd = int((~final).sum())
    # reverse
    basin = np.where(S, link, 0)
    cnt = np.array([len(x) for x in outs], np.int64)
    final = S | nodata | (cnt == 0)
    queue = collections.deque(np.flatnonzero(final).tolist())
    while queue:
        v = queue.popleft()
        for c in ins[v]:
            cnt[c] -= 1
            if cnt[c] == 0 and not final[c]:
                basin[c] = basin[recv[c]]
                final[c] = True
                queue.append(c)
    basin[~final] = -1
    n_inflow = np.array([len(x) for x in inflows], np.int64)
    shaped = [x.reshape(n, m).astype(np.int32) for x in (recv, code, order, link, basin, n_inflow)]
    return Net(*shaped, n_unresolved=(left_fwd, int((basin == -1).sum())))


def oracle_edges(o):
    """the edge list of the oracle's adjacency matrix o.A (CSC: columns are sources): a drained pit loses its facet edges, so
    every out-edge it has is a pit edge"""
    indptr, indices, data = o.A
    src = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    pits = np.unique(np.asarray(getattr(o, 'pit_i', []), np.int64))
    return src, np.asarray(indices, np.int64), np.asarray(data, np.float64), np.isin(src, pits)


def coverage(net, edges, shape, S):
    """what a tile exercises: (max order, links, cells with >= 3 stream inflows, stream receiver edges that are pit edges, that
    cross a 32-cell block boundary, stream cells whose receiver is off S)"""
    n, m = shape
    S = np.asarray(S, bool) & (net.order != 0)
    cells = np.flatnonzero(S.ravel() & (net.receiver.ravel() >= 0))
    r = net.receiver.ravel()[cells]
    on = S.ravel()[r]
    cross = (cells // m // 32 != r // m // 32) | (cells % m // 32 != r % m // 32)
    return dict(max_order=int(net.order.max()), links=int(np.unique(net.link[net.link > 0]).size), many=int((net.n_inflow >= 3).sum()),
                pit_recv=int((net.code.ravel()[cells][on] == 8).sum()), cross=int((cross & on).sum()), leaves=int((~on).sum()))


def line(edges, n_cells, S=None, w=None, pit=None):
    """a hand graph on a 1 x n_cells grid: edges = [(src, dst), ...]"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.ones(len(e)) if w is None else np.asarray(w, np.float64)
    pit = np.zeros(len(e), bool) if pit is None else np.asarray(pit, bool)
    return stream_network_ref((e[:, 0], e[:, 1], w, pit), (1, n_cells), np.zeros((1, n_cells)),
                              np.ones((1, n_cells), bool) if S is None else S)


def test_perfect_binary_tree():
    """node k flows into (k - 1) // 2: 8 sources of order 1, then 2, 3, and the root of order 4; every node is a link head"""
    net = line([(k, (k - 1) // 2) for k in range(1, 15)], 15)
    depth = np.floor(np.log2(np.arange(15) + 1)).astype(int)
    assert np.array_equal(net.order[0], 4 - depth) and sorted(set(net.order[0].tolist())) == [1, 2, 3, 4]
    assert np.array_equal(net.link[0], np.arange(15) + 1) and np.unique(net.link).size == 15
    assert np.array_equal(net.basin, net.link) and net.n_unresolved == (0, 0)
    assert net.receiver[0, 0] == -1 and np.array_equal(net.receiver[0, 1:], (np.arange(1, 15) - 1) // 2)


def test_a_chain_joining_a_trunk_and_three_inflows():
    # 0, 1 -> 2 (order 2) -> 3 <- 4 <- 5 (a chain of order 1) ; 3 -> 6
    net = line([(0, 2), (1, 2), (2, 3), (5, 4), (4, 3), (3, 6)], 7)
    assert net.order[0].tolist() == [1, 1, 2, 2, 1, 1, 2]
    assert net.link[0].tolist() == [1, 2, 3, 4, 6, 6, 4]                 # 5 -> 4 is one link; 3 is a junction, 6 goes on in its link
    assert net.n_inflow[0].tolist() == [0, 0, 2, 2, 1, 0, 1]
    # three order-1 inflows into one cell: order 2, not 3
    net = line([(0, 3), (1, 3), (2, 3)], 4)
    assert net.order[0].tolist() == [1, 1, 1, 2] and net.link[0].tolist() == [1, 2, 3, 4]
    # off the streams: the order is 0, a stream cell below starts again at 1, and the basins follow the receivers
    S = np.array([[False, True, True, False, False, True]])
    net = line([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], 6, S=S)
    assert net.order[0].tolist() == [0, 1, 1, 0, 0, 1] and net.link[0].tolist() == [0, 2, 2, 0, 0, 6]
    assert net.basin[0].tolist() == [2, 2, 2, 6, 6, 6]
    # a cell without a receiver reaches nothing
    net = line([(0, 1)], 3, S=np.array([[False, False, True]]))
    assert net.basin[0].tolist() == [0, 0, 3] and net.receiver[0].tolist() == [1, -1, -1]


def test_cycles_are_unresolved_and_counted():
    o = hand_graph()                                                      # 0 -> 1 <-> 2 (loop);  3 -> 4 -> 5
    net = stream_network_ref(oracle_edges(o), (1, 6), o.elev, np.ones((1, 6), bool))
    assert net.order[0].tolist() == [1, -1, -1, 1, 1, 1] and net.link[0].tolist() == [1, -1, -1, 4, 4, 4]
    assert net.basin[0].tolist() == [1, -1, -1, 4, 4, 4] and net.n_unresolved == (2, 2)
    # what lies downstream of the loop: 0 -> 1 <-> 2, 2 -> 3 -> 4 with the smaller weight
    net = line([(0, 1), (1, 2), (2, 1), (2, 3), (3, 4)], 5, w=[1, 1, 0.6, 0.4, 1])
    assert net.order[0].tolist() == [1, -1, -1, -1, -1] and net.n_unresolved == (4, 4)
    # off the streams the loop is upstream of nothing that is final: the basins of the loop and above it are -1
    net = line([(0, 1), (1, 2), (2, 1), (3, 4)], 5, S=np.array([[False, False, False, False, True]]))
    assert net.order[0].tolist() == [0, 0, 0, 0, 1] and net.basin[0].tolist() == [-1, -1, -1, 5, 5] and net.n_unresolved == (0, 3)
    # a NaN elevation is never a stream and has no receiver
    elev = np.zeros((1, 3)); elev[0, 1] = np.nan
    net = stream_network_ref(([0, 1], [1, 2], [1.0, 1.0], [False, False]), (1, 3), elev, np.ones((1, 3), bool))
    assert net.receiver[0].tolist() == [1, -1, -1] and net.order[0].tolist() == [1, 0, 1] and net.basin[0].tolist() == [1, 0, 3]


def test_the_tie_rule():
    net = line([(1, 2), (1, 0)], 3, w=[0.5, 0.5])
    assert net.receiver[0, 1] == 0 and net.code[0, 1] == 3               # equal weights: the lower destination (west)
    net = line([(1, 2), (1, 0)], 3, w=[0.5 + 1e-12, 0.5])
    assert net.receiver[0, 1] == 2 and net.code[0, 1] == 4
    net = line([(0, 1), (0, 1)], 2, w=[0.5, 0.5], pit=[True, False])
    assert net.receiver[0, 0] == 1 and net.code[0, 0] == 4               # a regular edge wins over a pit edge to the same cell
    net = line([(0, 1), (0, 1)], 2, w=[0.5 + 1e-12, 0.5], pit=[True, False])
    assert net.code[0, 0] == 8 and net.n_inflow[0, 1] == 1               # (and the source counts once)
    net = line([(0, 2), (0, 1)], 3, w=[0.5, 0.5], pit=[True, False])
    assert net.receiver[0, 0] == 1 and net.code[0, 0] == 4


def top_fraction(uca, frac):
    """the threshold that leaves the top `frac` of the finite areas"""
    return float(np.nanquantile(np.asarray(uca, np.float64), 1.0 - frac))


def test_fractal_tile_coverage():
    """the tile the device tests are sized on: what the top 5 % of uca exercises"""
    shape = (300, 260)
    o = fractal_oracle(shape, 5)
    edges = oracle_edges(o)
    S = np.asarray(o.uca) >= top_fraction(o.uca, 0.05)
    net = stream_network_ref(edges, shape, o.elev, S)
    cov = coverage(net, edges, shape, S)
    w = np.asarray(edges[2])
    srt = np.lexsort((-w, edges[0]))
    same = edges[0][srt][1:] == edges[0][srt][:-1]
    close = np.abs(w[srt][1:] - w[srt][:-1])[same] <= 1e-12 * w[srt][:-1][same]
    print(cov, net.n_unresolved, 'near ties', int(close.sum()))
    assert cov['max_order'] >= 4 and cov['links'] >= 1000 and cov['many'] >= 50 and cov['pit_recv'] >= 300
    assert cov['cross'] >= 200 and cov['leaves'] >= 100 and net.n_unresolved == (0, 0)
    assert np.array_equal(net.basin[S], net.link[S]) and (net.order[~S] == 0).all() and (net.order[S] >= 1).all()
