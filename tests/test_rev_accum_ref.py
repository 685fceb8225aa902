"""CPU tier: the reference of the reverse accumulation (DEMProcessor.calc_up_dependence / calc_watershed / calc_rev_accum,
pydem_rev_accum), pinned by itself.  tests/test_gpu_rev_accum.py holds the device against it.

rev_accum_ref(o, op, seed, absorb, absorb_value) is the semantics of include/pydem_hip.h as a reverse Kahn sweep over the
oracle's adjacency matrix o.A (OracleDEM.build_graph(): CSC, columns are sources, `indices` destinations), in this order:
    V = NaN where the elevation is NaN;  V = absorb_value on the absorbing cells (final, whatever their out-edges);
    V = seed where a cell has no out-edge;  otherwise, once every out-neighbour is final, over the out-edges in ascending
    destination order:  op 0  acc = 0; acc += w_e V[v_e]; V = seed + acc  (not normalised),  op 1  V = max(seed, max_e V[v_e]),
    NaN if any operand is NaN;
cells that never become ready (on or upstream of a drainage cycle) stay NaN and are not final."""
import warnings

import numpy as np
import pytest

from test_dist_down_ref import _ranges, dist_down_ref, ramp_oracle

# (shape, seed of synth.fractal(top_shift=7, n_octaves=7), interior outlet): dX = dY = 30, drain_pits=True
OUTLETS = [((96, 80), 5, (60, 72)), ((160, 130), 41, (132, 100)), ((70, 45), 19, (58, 14))]


def rev_accum_ref(o, op, seed=None, absorb=None, absorb_value=1.0, absolute=False):
    """(values [n, m], final mask [n, m], depth).  op: 0 sum, 1 max.  `absolute`: the same recursion with |seed| and
    |absorb_value| (the scale of the error bound)."""
    assert op in (0, 1) and (op == 0 or seed is not None)
    indptr, indices, data = o.A
    n, m = o.elev.shape
    NN = n * m
    indptr = indptr.astype(np.int64)
    dst_all = indices.astype(np.int64)
    outdeg = np.diff(indptr)
    by_dst = np.argsort(dst_all, kind='stable')
    in_ptr = np.zeros(NN + 1, np.int64)
    np.cumsum(np.bincount(dst_all, minlength=NN), out=in_ptr[1:])
    src_by_dst = (np.searchsorted(indptr, by_dst, side='right') - 1).astype(np.int64)      # source of edge by_dst[k]
    del by_dst
    sd = np.zeros(NN) if seed is None else np.array(np.broadcast_to(np.asarray(seed, np.float64), (n, m))).ravel()
    av = float(absorb_value)
    if absolute:
        sd, av = np.abs(sd), abs(av)
    nodata = np.isnan(np.asarray(o.elev, np.float64)).ravel()
    ab = np.zeros(NN, bool) if absorb is None else np.asarray(absorb, bool).ravel() & ~nodata
    leaf = (outdeg == 0) & ~nodata & ~ab
    V = np.full(NN, np.nan)
    V[ab] = av
    V[leaf] = sd[leaf]
    final = nodata | ab | leaf
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
        e = e[np.lexsort((dst_all[e], src))]
        seg = np.cumsum(deg) - deg
        s0 = sd[ready]
        acc, hi, bad = np.zeros(ready.size), s0.copy(), np.isnan(s0)
        for r in range(int(deg.max())):                  # the r-th out-edge of every ready cell that has one
            sel = np.flatnonzero(deg > r)
            er = e[seg[sel] + r]
            t = V[dst_all[er]]
            if op == 0:
                acc[sel] += data[er] * t
            else:
                bad[sel] |= np.isnan(t)
                hi[sel] = np.where(t > hi[sel], t, hi[sel])
        with np.errstate(invalid='ignore'):
            val = s0 + acc if op == 0 else np.where(bad, np.nan, hi)
        val[np.isnan(val)] = np.nan                      # (one NaN)
        V[ready] = val
        final[ready] = True
        frontier = ready
    V[~final] = np.nan
    return V.reshape(n, m), final.reshape(n, m), depth


def fractal_oracle(shape, seed):
    from oracle import oracle as O
    from pydem_amd import synth
    z = synth.fractal(shape[0], shape[1], seed=seed, top_shift=7, n_octaves=7)
    o = O.OracleDEM(z, dX=30.0, dY=30.0, drain_pits=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    return o


def hand_graph():
    """the 1 x 6 graph of test_dist_down_ref.test_cycles_and_dead_ends_are_nan: 0 -> 1 <-> 2 (loop);  3 -> 4 -> 5"""
    class G(object):
        pass
    o = G()
    o.elev = np.arange(6, 0, -1, dtype=np.float64).reshape(1, 6)
    o.dX2 = np.array([2.0]); o.dY2 = np.array([3.0])
    src = np.array([0, 1, 2, 3, 4]); dst = np.array([1, 2, 1, 4, 5])
    indptr = np.zeros(7, np.int32)
    np.cumsum(np.bincount(src, minlength=6), out=indptr[1:])
    o.A = (indptr, dst.astype(np.int32), np.ones(5))
    return o


@pytest.mark.parametrize('shape,seed,outlet', OUTLETS)
def test_dependence_is_dual_to_the_oracles_uca(shape, seed, outlet):
    """sum over the cells of area x (share of the cell's flow that reaches the outlet) = the outlet's contributing area"""
    o = fractal_oracle(shape, seed)
    absorb = np.zeros(shape, bool)
    absorb[outlet] = True
    dep, final, depth = rev_accum_ref(o, 0, absorb=absorb, absorb_value=1.0)
    assert final.all() and not np.isnan(dep).any() and depth > 5
    assert dep[outlet] == 1.0 and dep.min() >= 0.0 and dep.max() <= 1.0 + 1e-12
    total = float((dep * (o.dX2 * o.dY2)[:, None]).sum())
    want = float(o.uca[outlet])
    print("%r outlet %r: relative difference %.3g, %d watershed cells, %d partial" %
          (shape, outlet, abs(total - want) / want, (dep > 0).sum(), ((dep > 0) & (dep < 1)).sum()))
    assert abs(total - want) <= 1e-12 * want
    assert (dep > 0).sum() >= 300 and ((dep > 0) & (dep < 1)).sum() >= 100


def test_ramp_dependence_and_counts():
    o = ramp_oracle()
    n, m = o.elev.shape
    target = np.zeros((n, m), bool)
    target[:, -1] = True
    ok = np.isfinite(dist_down_ref(o, target, 'h', 'ave')[0])
    assert ok.sum() >= (n - 2) * m
    dep, final, depth = rev_accum_ref(o, 0, absorb=target)
    assert final.all() and depth >= m - 1
    assert (dep[ok] == 1.0).all()
    racc, final, _ = rev_accum_ref(o, 0, seed=np.ones((n, m)))
    assert final.all()
    want = np.broadcast_to(1.0 + (m - 1 - np.arange(m)), (n, m))         # the cell itself + the cells downslope in its row
    assert np.array_equal(racc[ok], want[ok])


def test_cycles_dead_ends_and_the_running_maximum():
    o = hand_graph()
    seed = np.array([[5.0, 1.0, 2.0, 3.0, 7.0, 4.0]])
    for op in (0, 1):
        V, final, depth = rev_accum_ref(o, op, seed=seed)
        assert list(final.ravel()) == [False, False, False, True, True, True] and depth == 3
        assert np.isnan(V[0, :3]).all()
        assert V[0, 5] == 4.0                                              # the dead end carries its seed
    assert list(V[0, 3:]) == [7.0, 7.0, 4.0]                             # max along 3 -> 4 -> 5
    V, _, _ = rev_accum_ref(o, 0, seed=seed)
    assert list(V[0, 3:]) == [14.0, 11.0, 4.0]
    # an absorbing cell is final whatever its out-edges: cell 1 breaks the loop
    absorb = np.zeros((1, 6), bool); absorb[0, 1] = True
    V, final, _ = rev_accum_ref(o, 0, absorb=absorb, absorb_value=1.0)
    assert final.all() and list(V[0]) == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    # NaN elevation comes first
    o.elev[0, 5] = np.nan
    V, final, _ = rev_accum_ref(o, 1, seed=seed)
    assert np.isnan(V[0, 3:]).all() and final[0, 3:].all()


def test_max_dominates_the_seed_and_keeps_integers():
    shape, seed, _ = OUTLETS[2]
    o = fractal_oracle(shape, seed)
    w = np.random.default_rng(2).integers(-50, 50, shape).astype(np.float64)
    dmax, final, _ = rev_accum_ref(o, 1, seed=w)
    assert final.all() and not np.isnan(dmax).any()
    assert (dmax >= w).all() and (dmax > w).mean() > 0.5
    assert np.array_equal(dmax, np.rint(dmax)) and np.isin(dmax, w).all()
    # absolute: the recursion on |seed|
    both = rev_accum_ref(o, 0, seed=w, absolute=True)[0]
    assert np.array_equal(both, rev_accum_ref(o, 0, seed=np.abs(w))[0])
