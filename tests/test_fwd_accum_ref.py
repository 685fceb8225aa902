"""CPU tier: the reference of the forward accumulation with a per-cell rule (DEMProcessor.calc_decay_accum /
calc_trans_lim_accum, pydem_fwd_accum), pinned by itself.  tests/test_gpu_fwd_accum.py holds the device against it.

fwd_accum_ref(o, load, mult, cap, edge_nan) is the semantics of include/pydem_hip.h as a forward Kahn sweep over the oracle's
adjacency matrix o.A (OracleDEM.build_graph(): CSC, columns are sources, `indices` destinations):
    V = I = NaN where the elevation is NaN and, with edge_nan, on the tile's border and beside a NaN elevation;
    I = 0, tot = load where a cell has no in-edge; otherwise, once every in-neighbour is final, over the in-edges in ascending
    source order:  acc = 0; acc += w_e * (mult[u_e] * V[u_e]);  I = acc;  tot = load + acc;
    V = tot without a cap,  V = NaN if tot is NaN else min(tot, cap) with one;
cells that never become ready (on or downstream of a drainage cycle) stay NaN and are not final."""
import numpy as np
import pytest

from test_dist_down_ref import _ranges, ramp_oracle
from test_dist_up_ref import edge_nan_cells
from test_rev_accum_ref import OUTLETS, fractal_oracle, hand_graph, rev_accum_ref


def fwd_accum_ref(o, load, mult=None, cap=None, edge_nan=False, absolute=False):
    """(V [n, m], I [n, m], final mask [n, m], depth).  `absolute`: the same recursion with |load|, |mult| and no cap (the
    scale of the error bound)."""
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
    plane = lambda a: np.array(np.broadcast_to(np.asarray(a, np.float64), (n, m))).ravel()
    ld = plane(load)
    mu = None if mult is None else plane(mult)
    cp = None if cap is None else plane(cap)
    if absolute:
        ld, mu, cp = np.abs(ld), (None if mu is None else np.abs(mu)), None

    def value(tot, cells):
        with np.errstate(invalid='ignore'):
            v = tot if cp is None else np.where(np.isnan(tot), np.nan, np.minimum(tot, cp[cells]))
        v = np.array(v, np.float64)
        v[np.isnan(v)] = np.nan                          # (one NaN)
        return v

    elev = np.asarray(o.elev, np.float64)
    nanv = (edge_nan_cells(elev) if edge_nan else np.isnan(elev)).ravel()
    head = ~nanv & (indeg == 0)
    V = np.full(NN, np.nan)
    I = np.full(NN, np.nan)
    I[head] = 0.0
    V[head] = value(ld[head] + 0.0, np.flatnonzero(head))
    final = nanv | head
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
        seg = np.cumsum(deg) - deg
        acc = np.zeros(ready.size)
        with np.errstate(invalid='ignore'):
            for r in range(int(deg.max())):              # the r-th in-edge of every ready cell that has one
                sel = np.flatnonzero(deg > r)
                er = e[seg[sel] + r]
                src = src_all[er]
                acc[sel] += data[er] * (V[src] if mu is None else mu[src] * V[src])
            acc[np.isnan(acc)] = np.nan
            I[ready] = acc
            V[ready] = value(ld[ready] + acc, ready)
        final[ready] = True
        frontier = ready
    V[~final] = np.nan
    I[~final] = np.nan
    return V.reshape(n, m), I.reshape(n, m), final.reshape(n, m), depth


def out_weight_sum(o):
    """per cell, the sum of the weights of its out-edges (1 where all its flow stays on the graph)"""
    indptr, _, data = o.A
    n, m = o.elev.shape
    src = np.repeat(np.arange(n * m), np.diff(indptr))
    return np.bincount(src, weights=data, minlength=n * m).reshape(n, m)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module', params=OUTLETS, ids=lambda p: '%dx%d' % p[0])
def fractal(request):
    shape, seed, outlet = request.param
    return fractal_oracle(shape, seed), shape, outlet


def test_plain_sum_equals_the_oracles_uca(fractal):
    o, shape, _ = fractal
    area = np.broadcast_to((o.dX2 * o.dY2)[:, None], shape)
    V, I, final, depth = fwd_accum_ref(o, area)
    uca = np.asarray(o.uca, np.float64)
    ok = np.isfinite(uca)
    worst = float(np.max(np.abs(V[ok] - uca[ok]) / uca[ok]))
    print("%r: %d NaN cells in uca, worst relative difference %.3g, depth %d" % (shape, (~ok).sum(), worst, depth))
    assert final.all() and depth > 5 and (~ok).sum() <= 10
    assert np.isfinite(V).all() and worst <= 1e-12
    assert same_bits(V, area + I)


def test_duality_with_the_reverse_accumulation(fractal):
    o, shape, outlet = fractal
    absorb = np.zeros(shape, bool)
    absorb[outlet] = True
    dep = rev_accum_ref(o, 0, absorb=absorb)[0]
    w = np.random.default_rng(11).uniform(-1.0, 2.0, shape)
    V = fwd_accum_ref(o, w)[0]
    want, scale = float((dep * w).sum()), float(np.abs(dep * w).sum())
    print("%r outlet %r: |V - sum(dep w)| / sum|dep w| = %.3g" % (shape, outlet, abs(V[outlet] - want) / scale))
    assert abs(V[outlet] - want) <= 1e-12 * scale


def test_neutral_arguments_give_the_bits_of_none(fractal):
    o, shape, _ = fractal
    w = np.random.default_rng(12).uniform(-1.0, 2.0, shape)
    V, I, _, _ = fwd_accum_ref(o, w)
    for kw in (dict(mult=1.0), dict(cap=np.inf), dict(mult=np.ones(shape), cap=np.full(shape, np.inf))):
        V2, I2, _, _ = fwd_accum_ref(o, w, **kw)
        assert same_bits(V, V2) and same_bits(I, I2), kw
    # absolute: the recursion on |load| and |mult| without the cap
    assert same_bits(fwd_accum_ref(o, w, mult=-0.5, cap=1.0, absolute=True)[0], fwd_accum_ref(o, np.abs(w), mult=0.5)[0])


def test_constant_capacity(fractal):
    o, shape, _ = fractal
    T, I, final, _ = fwd_accum_ref(o, 1.0, cap=5.0)
    D = (1.0 + I) - T
    capped = float((D > 0).mean())
    print("%r: supply 1, cap 5: %.3f of the cells deposit" % (shape, capped))
    assert final.all() and np.isfinite(T).all()
    assert capped >= 0.15 and (D >= 0).all() and T.max() == 5.0
    assert (D[T < 5.0] == 0).all()                   # exactly 0 wherever the cap does not bind (tot == cap: D = 0 at T = cap)
    assert (T[D > 0] == 5.0).all()
    left = float((T * (1.0 - out_weight_sum(o))).sum())
    total = float(T.size)
    assert abs(total - (float(D.sum()) + left)) <= 1e-12 * total


def test_random_capacity(fractal):
    o, shape, _ = fractal
    free = fwd_accum_ref(o, 1.0)[0]
    cap = 2.0 * np.median(free) * np.random.default_rng(13).uniform(0.5, 1.5, shape)
    T, I, final, _ = fwd_accum_ref(o, 1.0, cap=cap)
    D = (1.0 + I) - T
    capped, passing = float((D > 0).mean()), float(((I > 0) & (D == 0)).mean())
    print("%r: random cap: %.3f capped, %.3f with inflow and no deposition" % (shape, capped, passing))
    assert final.all() and (D >= 0).all() and (T <= cap).all()
    assert capped >= 0.15 and passing >= 0.3
    assert (D[T < cap] == 0).all() and (T[D > 0] == cap[D > 0]).all()


def test_decay_shrinks_the_accumulation(fractal):
    o, shape, _ = fractal
    plain = fwd_accum_ref(o, 1.0)[0]
    mult = np.random.default_rng(14).uniform(0.5, 1.0, shape)
    V = fwd_accum_ref(o, 1.0, mult=mult)[0]
    print("%r: max %.4g with decay, %.4g without" % (shape, V.max(), plain.max()))
    assert (V <= plain).all() and (V >= 1.0).all()
    assert V.max() < plain.max() / 5


def test_edge_nan(fractal):
    o, shape, _ = fractal
    off = fwd_accum_ref(o, 1.0)[0]
    V, I, final, _ = fwd_accum_ref(o, 1.0, edge_nan=True)
    ok = np.isfinite(V)
    print("%r: %.3f finite under edge_nan" % (shape, ok.mean()))
    assert final.all() and 0.7 <= ok.mean() < 1.0
    assert np.isnan(V[edge_nan_cells(np.asarray(o.elev))]).all()
    assert np.array_equal(np.isnan(V), np.isnan(I))
    assert same_bits(V[ok], off[ok])
    # NaN is closed downstream
    indptr, indices, _ = o.A
    src = np.repeat(np.arange(V.size), np.diff(indptr))
    assert not ok.ravel()[indices[np.isnan(V.ravel()[src])]].any()


def test_hand_graph_loop_chain_and_nan_source():
    """0 -> 1 <-> 2 (loop);  3 -> 4 -> 5.  The loop is NaN and not final.  Cell 0 feeds the loop but nothing flows into it: in a
    FORWARD sweep it is final from the start with its own load (in the reverse sweep of test_rev_accum_ref.py it is the cell
    upstream of the loop that never becomes ready)."""
    o = hand_graph()
    load = np.array([[5.0, 1.0, 2.0, 3.0, 7.0, 4.0]])
    V, I, final, depth = fwd_accum_ref(o, load)
    assert list(final.ravel()) == [True, False, False, True, True, True] and depth == 3
    assert V[0, 0] == 5.0 and I[0, 0] == 0.0                                # (final: nothing flows into it)
    assert np.isnan(V[0, 1:3]).all() and np.isnan(I[0, 1:3]).all()
    assert list(V[0, 3:]) == [3.0, 10.0, 14.0] and list(I[0, 3:]) == [0.0, 3.0, 10.0]
    mult = np.array([[1.0, 1.0, 1.0, 0.5, 0.25, 9.0]])
    V, I, _, _ = fwd_accum_ref(o, load, mult=mult)
    assert list(V[0, 3:]) == [3.0, 8.5, 6.125] and list(I[0, 3:]) == [0.0, 1.5, 2.125]
    V, I, _, _ = fwd_accum_ref(o, load, cap=np.array([[9.0, 9.0, 9.0, 2.0, 8.0, 20.0]]))
    assert list(V[0, 3:]) == [2.0, 8.0, 12.0] and list(I[0, 3:]) == [0.0, 2.0, 8.0]
    # the loop with nothing flowing in is still a loop: cell 0 does not matter
    V, _, final, _ = fwd_accum_ref(o, load, mult=0.0, cap=1.0)
    assert np.isnan(V[0, 1:3]).all() and not final[0, 1:3].any()
    # a NaN source makes everything downstream NaN, a finite cap or not; the NaN elevation comes first
    bad = load.copy()
    bad[0, 3] = np.nan
    V, I, final, _ = fwd_accum_ref(o, bad, cap=1.0)
    assert np.isnan(V[0, 3:]).all() and final[0, 3:].all() and I[0, 3] == 0.0 and np.isnan(I[0, 4:]).all()
    o.elev[0, 3] = np.nan
    V, I, final, _ = fwd_accum_ref(o, load, cap=1.0)
    assert np.isnan(V[0, 3:]).all() and np.isnan(I[0, 3:]).all() and final[0, 3:].all()


def test_ramp_geometric_series_and_cap():
    o = ramp_oracle()
    n, m = o.elev.shape
    j = np.broadcast_to(np.arange(m, dtype=np.float64), (n, m))
    for k in (0.5, 0.9, 0.0):
        V, I, final, depth = fwd_accum_ref(o, 1.0, mult=k)
        want = (1.0 - k ** (j + 1.0)) / (1.0 - k)
        assert final.all() and depth >= m - 1
        # (the rows of the border need not flow along the ramp: the interior rows do, all the way from column 0)
        assert np.allclose(V[1:-1], want[1:-1], rtol=1e-12, atol=0)
    for cap in (4.0, 6.5, 100.0):
        V, I, _, _ = fwd_accum_ref(o, 1.0, cap=cap)
        assert np.array_equal(V[1:-1], np.minimum(j + 1.0, cap)[1:-1])
        assert np.array_equal(I[1:-1, 1:], V[1:-1, :-1])
