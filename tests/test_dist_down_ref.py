"""CPU tier: the reference of the downslope distance (DEMProcessor.calc_dist_down / calc_hand, pydem_dist_down), pinned by
itself.  tests/test_gpu_dist_down.py holds the device against it.

dist_down_ref(o, target, kind, stat) is the semantics of include/pydem_hip.h as a reverse Kahn sweep over the oracle's
adjacency matrix o.A (OracleDEM.build_graph(): CSC, columns are sources, `indices` destinations):
    D = 0 on targets; NaN where a cell has no out-edge; otherwise, once every out-neighbour is final,
    t_e = D[v_e] + cost(c, v_e):  'ave' sum(w_e t_e) / sum(w_e),  'min' / 'max' of t_e (NaN if any t_e is NaN);
    cost 'h' = hypot((j' - j) dX2[r], (r' - r) dY2[r]),  'v' = elev[c] - elev[v],  's' = hypot(h, v);
cells that never become ready (on or upstream of a drainage cycle) stay NaN and are not final."""
import warnings

import numpy as np

KINDS = ('h', 'v', 's')
STATS = ('ave', 'min', 'max')


def _ranges(start, count):
    """concatenation of arange(start[k], start[k] + count[k]) (count > 0)"""
    tot = int(count.sum())
    if tot == 0:
        return np.zeros(0, np.int64)
    first = np.cumsum(count) - count
    return np.repeat(start - first, count) + np.arange(tot, dtype=np.int64)


def edge_cost(o, src, dst, kind, absolute=False):
    n, m = o.elev.shape
    r, j = src // m, src % m
    r2, j2 = dst // m, dst % m
    h = np.hypot((j2 - j) * o.dX2[r], (r2 - r) * o.dY2[r])
    if kind == 'h':
        return h
    z = o.elev.ravel()
    v = z[src] - z[dst]
    if kind == 'v':
        return np.abs(v) if absolute else v
    return np.hypot(h, v)


def dist_down_ref(o, target, kind='h', stat='ave', absolute=False):
    """(values [n, m], final mask [n, m], depth).  `absolute`: the same recursion with |cost| (the scale of the error bound)."""
    assert kind in KINDS and stat in STATS
    indptr, indices, data = o.A
    n, m = o.elev.shape
    NN = n * m
    indptr = indptr.astype(np.int64)
    dst_all = indices.astype(np.int64)
    outdeg = np.diff(indptr)
    # in-edges: edge ids grouped by destination
    by_dst = np.argsort(dst_all, kind='stable')
    in_ptr = np.zeros(NN + 1, np.int64)
    np.cumsum(np.bincount(dst_all, minlength=NN), out=in_ptr[1:])
    src_by_dst = (np.searchsorted(indptr, by_dst, side='right') - 1).astype(np.int64)      # source of edge by_dst[k]
    del by_dst
    tg = np.asarray(target, bool).ravel()
    D = np.full(NN, np.nan)
    D[tg] = 0.0
    final = tg | (outdeg == 0)
    cnt = outdeg.copy()
    frontier = np.flatnonzero(final)
    depth = 0
    while frontier.size:
        depth += 1
        k = in_ptr[frontier + 1] - in_ptr[frontier]
        up = src_by_dst[_ranges(in_ptr[frontier][k > 0], k[k > 0])]
        up = up[~final[up]]
        if up.size == 0:
            break
        u, c = np.unique(up, return_counts=True)
        cnt[u] -= c
        ready = u[cnt[u] == 0]
        if ready.size == 0:
            break
        deg = outdeg[ready]
        e = _ranges(indptr[ready], deg)
        src = np.repeat(ready, deg)
        # (a column's destinations in ascending order: the order in which the device adds)
        order = np.lexsort((dst_all[e], src))
        e = e[order]
        t = D[dst_all[e]] + edge_cost(o, src, dst_all[e], kind, absolute)
        seg = np.cumsum(deg) - deg
        if stat == 'ave':
            w = data[e]
            val = np.add.reduceat(w * t, seg) / np.add.reduceat(w, seg)
        elif stat == 'min':
            val = np.minimum.reduceat(t, seg)            # (np.minimum / np.maximum propagate NaN)
        else:
            val = np.maximum.reduceat(t, seg)
        D[ready] = val
        final[ready] = True
        frontier = ready
    D[~final] = np.nan
    return D.reshape(n, m), final.reshape(n, m), depth


def ramp_oracle(n=12, m=17):
    """planar ramp falling along the columns, z = -j, dX = 2, dY = 3 (oracle with its graph built)"""
    from oracle import oracle as O
    z = -np.tile(np.arange(m, dtype=np.float64), (n, 1))
    o = O.OracleDEM(z, dX=2.0, dY=3.0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_slopes_directions()
        o.build_graph()
    return o


def test_ramp_distance_is_the_column_distance():
    o = ramp_oracle()
    n, m = o.elev.shape
    target = np.zeros((n, m), bool)
    target[:, -1] = True
    want = (m - 1 - np.arange(m)) * o.dX2[:, None]
    seen = 0
    for stat in STATS:
        D, final, depth = dist_down_ref(o, target, 'h', stat)
        ok = np.isfinite(D)
        assert final.all() and ok.sum() >= (n - 2) * m
        assert np.allclose(D[ok], np.broadcast_to(want, (n, m))[ok], rtol=1e-12, atol=0)
        assert depth >= m - 1
        seen += ok.sum()
    assert seen
    # the drop along the same paths is the column difference, and 's' is hypot of the two per step
    V, _, _ = dist_down_ref(o, target, 'v', 'ave')
    ok = np.isfinite(V)
    assert np.allclose(V[ok], np.broadcast_to((m - 1 - np.arange(m)) * 1.0, (n, m))[ok], rtol=1e-12, atol=0)
    S, _, _ = dist_down_ref(o, target, 's', 'ave')
    assert np.allclose(S[ok], np.broadcast_to((m - 1 - np.arange(m)) * np.hypot(2.0, 1.0), (n, m))[ok], rtol=1e-12, atol=0)


def test_min_equals_dijkstra_to_the_nearest_target():
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    from oracle import oracle as O
    from pydem_amd import synth
    z = synth.fractal(90, 70, seed=5, top_shift=5, n_octaves=5)
    o = O.OracleDEM(z, dX=30.0, dY=20.0, drain_pits=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    n, m = z.shape
    NN = n * m
    target = o.uca >= 40 * 600.0
    assert 0 < target.sum() < NN // 4
    D, final, depth = dist_down_ref(o, target, 'h', 'min')
    ok = np.isfinite(D)
    assert final.all() and ok.mean() > 0.5 and depth > 5
    indptr, indices, data = o.A
    src = np.repeat(np.arange(NN), np.diff(indptr))
    dst = indices.astype(np.int64)
    cost = edge_cost(o, src, dst, 'h')
    # the same edges and costs, plus a zero-cost edge from every target to one sink (explicit zeros are edges)
    sink = NN
    tcells = np.flatnonzero(target.ravel())
    keep = ~target.ravel()[src]                      # a target's own out-edges do not matter: it is at distance 0
    G = sp.csr_matrix((np.r_[cost[keep], np.full(tcells.size, 1e-300)], (np.r_[src[keep], tcells], np.r_[dst[keep], np.full(tcells.size, sink)])),
                      shape=(NN + 1, NN + 1))
    dj = dijkstra(G.T.tocsr(), directed=True, indices=sink)[:NN].reshape(n, m)
    assert np.allclose(D[ok], dj[ok], rtol=1e-12, atol=1e-290)
    assert (D[target] == 0).all()


def test_cycles_and_dead_ends_are_nan():
    """a two-cell loop: the loop and everything upstream of it is not final; a cell without an out-edge is final and NaN"""
    class G(object):
        pass
    o = G()
    n, m = 1, 6
    o.elev = np.arange(6, 0, -1, dtype=np.float64).reshape(n, m)
    o.dX2 = np.array([2.0]); o.dY2 = np.array([3.0])
    # 0 -> 1 <-> 2 (loop);  3 -> 4 -> 5 (target);  columns are sources
    src = np.array([0, 1, 2, 3, 4]); dst = np.array([1, 2, 1, 4, 5])
    indptr = np.zeros(7, np.int32)
    np.cumsum(np.bincount(src, minlength=6), out=indptr[1:])
    o.A = (indptr, dst.astype(np.int32), np.ones(5))
    target = np.zeros((n, m), bool); target[0, 5] = True
    D, final, depth = dist_down_ref(o, target, 'h', 'ave')
    assert list(final.ravel()) == [False, False, False, True, True, True]
    assert np.isnan(D[0, :3]).all() and list(D[0, 3:]) == [4.0, 2.0, 0.0] and depth == 3
    target[0, 5] = False
    D, final, _ = dist_down_ref(o, target, 'h', 'max')
    assert np.isnan(D).all() and list(final.ravel()) == [False, False, False, True, True, True]
