"""CPU tier: the reference of the upslope flow-path distance (DEMProcessor.calc_dist_up, pydem_dist_up), pinned by itself.
tests/test_gpu_dist_up.py holds the device against it.

dist_up_ref(o, kind, stat, edge_nan) is the semantics of include/pydem_hip.h as a forward Kahn sweep over the oracle's
adjacency matrix o.A (OracleDEM.build_graph(): CSC, columns are sources, `indices` destinations):
    U = NaN where the elevation is NaN and, with edge_nan, on the tile's border and beside a NaN elevation; 0 where a cell has
    no in-edge; otherwise, once every in-neighbour is final,
    t_e = U[u_e] + cost(u_e, c):  'ave' sum(w_e t_e) / sum(w_e),  'min' / 'max' of t_e (NaN if any t_e is NaN), the in-edges
    in ascending source order; the cost is edge_cost of tests/test_dist_down_ref.py (the source row's cell size);
cells that never become ready (on or downstream of a drainage cycle) stay NaN and are not final."""
import warnings

import numpy as np

from test_dist_down_ref import KINDS, STATS, _ranges, edge_cost, ramp_oracle


def edge_nan_cells(elev):
    """the cells TauDEM's edge-contamination rule makes NaN: the border, no-data cells and their 8-neighbours"""
    nan = np.isnan(elev)
    out = nan.copy()
    out[0, :] = out[-1, :] = True
    out[:, 0] = out[:, -1] = True
    pad = np.pad(nan, 1, constant_values=False)
    n, m = elev.shape
    for a in range(3):
        for b in range(3):
            out |= pad[a:a + n, b:b + m]
    return out


def dist_up_ref(o, kind='h', stat='max', edge_nan=True, absolute=False):
    """(values [n, m], final mask [n, m], depth).  `absolute`: the same recursion with |cost| (the scale of the error bound)."""
    assert kind in KINDS and stat in STATS
    indptr, indices, data = o.A
    n, m = o.elev.shape
    NN = n * m
    indptr = indptr.astype(np.int64)
    dst_all = indices.astype(np.int64)
    outdeg = np.diff(indptr)
    src_all = np.repeat(np.arange(NN, dtype=np.int64), outdeg)
    # in-edges: edge ids grouped by destination, ascending source inside a group (the order in which the device adds)
    by_dst = np.argsort(dst_all, kind='stable')
    indeg = np.bincount(dst_all, minlength=NN)
    in_ptr = np.zeros(NN + 1, np.int64)
    np.cumsum(indeg, out=in_ptr[1:])
    elev = np.asarray(o.elev, np.float64)
    nanv = (edge_nan_cells(elev) if edge_nan else np.isnan(elev)).ravel()
    U = np.full(NN, np.nan)
    U[~nanv & (indeg == 0)] = 0.0
    final = nanv | (indeg == 0)
    cnt = indeg.copy()
    frontier = np.flatnonzero(final)
    depth = 0
    while frontier.size:
        depth += 1
        k = outdeg[frontier]
        down = dst_all[_ranges(indptr[frontier][k > 0], k[k > 0])]
        down = down[~final[down]]
        if down.size == 0:
            break
        u, c = np.unique(down, return_counts=True)
        cnt[u] -= c
        ready = u[cnt[u] == 0]
        if ready.size == 0:
            break
        deg = indeg[ready]
        e = by_dst[_ranges(in_ptr[ready], deg)]
        t = U[src_all[e]] + edge_cost(o, src_all[e], np.repeat(ready, deg), kind, absolute)
        seg = np.cumsum(deg) - deg
        if stat == 'ave':
            w = data[e]
            val = np.add.reduceat(w * t, seg) / np.add.reduceat(w, seg)
        elif stat == 'min':
            val = np.minimum.reduceat(t, seg)            # (np.minimum / np.maximum propagate NaN)
        else:
            val = np.maximum.reduceat(t, seg)
        U[ready] = val
        final[ready] = True
        frontier = ready
    U[~final] = np.nan
    return U.reshape(n, m), final.reshape(n, m), depth


def small_fractal_oracle():
    from oracle import oracle as O
    from pydem_amd import synth
    z = synth.fractal(90, 70, seed=5, top_shift=5, n_octaves=5)
    o = O.OracleDEM(z, dX=30.0, dY=20.0, drain_pits=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    return o


def test_ramp_distance_is_the_column_distance_from_the_top():
    o = ramp_oracle()
    n, m = o.elev.shape
    col = np.broadcast_to(np.arange(m, dtype=np.float64), (n, m))
    for stat in STATS:
        U, final, depth = dist_up_ref(o, 'h', stat, edge_nan=False)
        ok = np.isfinite(U)
        assert final.all() and ok.all() and depth >= m - 1
        # (the rows of the border need not flow along the ramp: the interior rows do, all the way from column 0)
        assert np.allclose(U[1:-1], (col * o.dX2[:, None])[1:-1], rtol=1e-12, atol=0)
    V, _, _ = dist_up_ref(o, 'v', 'ave', edge_nan=False)
    assert np.allclose(V[1:-1], col[1:-1], rtol=1e-12, atol=0)
    S, _, _ = dist_up_ref(o, 's', 'ave', edge_nan=False)
    assert np.allclose(S[1:-1], col[1:-1] * np.hypot(2.0, 1.0), rtol=1e-12, atol=0)


def test_min_equals_dijkstra_from_the_divides():
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    o = small_fractal_oracle()
    n, m = o.elev.shape
    NN = n * m
    U, final, depth = dist_up_ref(o, 'h', 'min', edge_nan=False)
    assert final.all() and np.isfinite(U).all() and depth > 5
    indptr, indices, data = o.A
    src = np.repeat(np.arange(NN), np.diff(indptr))
    dst = indices.astype(np.int64)
    cost = edge_cost(o, src, dst, 'h')
    # the same edges and costs, plus a (nearly) free edge from one super-source to every cell nothing flows into
    heads = np.flatnonzero(np.bincount(dst, minlength=NN) == 0)
    assert 0 < heads.size < NN
    G = sp.csr_matrix((np.r_[cost, np.full(heads.size, 1e-300)], (np.r_[src, np.full(heads.size, NN)], np.r_[dst, heads])),
                      shape=(NN + 1, NN + 1))
    dj = dijkstra(G, directed=True, indices=NN)[:NN].reshape(n, m)
    assert np.allclose(U, dj, rtol=1e-12, atol=1e-290)
    assert (U.ravel()[heads] == 0).all()


def test_min_ave_max_are_ordered():
    o = small_fractal_oracle()
    lo, ave, hi = (dist_up_ref(o, 'h', stat, edge_nan=False)[0] for stat in ('min', 'ave', 'max'))
    assert np.isfinite(lo).all() and np.isfinite(ave).all() and np.isfinite(hi).all()
    # (a rounded weighted mean may leave the interval of its operands by a few ulp)
    assert (lo <= ave * (1 + 1e-12)).all() and (ave <= hi * (1 + 1e-12)).all()
    assert (lo < hi).any() and hi.max() > 10 * 20.0


def test_cycles_and_what_they_feed_are_nan():
    """0 -> 1 <-> 2 -> 3, 4 -> 5: the loop and everything downstream of it is not final; heads are 0"""
    class G(object):
        pass
    o = G()
    n, m = 1, 6
    o.elev = np.arange(6, 0, -1, dtype=np.float64).reshape(n, m)
    o.dX2 = np.array([2.0]); o.dY2 = np.array([3.0])
    src = np.array([0, 1, 2, 2, 4]); dst = np.array([1, 2, 1, 3, 5])          # columns are sources
    indptr = np.zeros(7, np.int32)
    np.cumsum(np.bincount(src, minlength=6), out=indptr[1:])
    o.A = (indptr, dst.astype(np.int32), np.ones(5))
    for stat in STATS:
        U, final, depth = dist_up_ref(o, 'h', stat, edge_nan=False)
        assert list(final.ravel()) == [True, False, False, False, True, True]
        assert np.isnan(U[0, 1:4]).all() and U[0, 0] == 0.0 and U[0, 4] == 0.0 and U[0, 5] == 2.0 and depth == 2
    V, _, _ = dist_up_ref(o, 'v', 'max', edge_nan=False)
    assert V[0, 5] == 1.0
    # one row: every cell is on the border
    U, final, _ = dist_up_ref(o, 'h', 'max', edge_nan=True)
    assert np.isnan(U).all() and final.all()


def test_edge_nan_border_rule():
    o = ramp_oracle(5, 5)
    off, f_off, _ = dist_up_ref(o, 'h', 'max', edge_nan=False)
    on, f_on, _ = dist_up_ref(o, 'h', 'max', edge_nan=True)
    assert f_off.all() and f_on.all() and np.isfinite(off).all()
    border = np.ones((5, 5), bool)
    border[1:-1, 1:-1] = False
    assert np.isnan(on[border]).all()
    # every interior cell of a ramp has a flow path that enters through the border column at its top
    assert np.isnan(on).all()
    assert (off[1:-1, 1:] > 0).all() and (off[1:-1, 0] == 0).all()
    # on terrain with divides inside the tile: NaN is closed downstream, and the finite values are those of the other mode
    o = small_fractal_oracle()
    z = np.array(o.elev)
    for stat in STATS:
        off, _, _ = dist_up_ref(o, 'h', stat, edge_nan=False)
        on, final, _ = dist_up_ref(o, 'h', stat, edge_nan=True)
        ok = np.isfinite(on)
        assert final.all() and 0.2 < ok.mean() < 1.0
        assert np.isnan(on[edge_nan_cells(z)]).all()
        assert np.array_equal(on[ok], off[ok])
        indptr, indices, _ = o.A
        src = np.repeat(np.arange(z.size), np.diff(indptr))
        assert not ok.ravel()[indices[np.isnan(on.ravel()[src])]].any()
    # a no-data cell and its 8 neighbours
    z[40, 30] = np.nan
    rule = edge_nan_cells(z)
    assert rule[39:42, 29:32].all() and not rule[38, 30] and not rule[40, 32]
