"""Terrain built to sit on the fixed capacities of the device kernels (tests/test_gpu_capacity_edges.py, and the unbounded-reach
fixtures of oracle/ref_harness/gen_golden.py).  Every constructor is seeded and deterministic and returns, next to the surface,
the host-side quantity that shows it reaches its target: the border / drain count of a pit search, the row spans of the
pit -> drain pairs, the in-degree-0 cells of a sweep tile, the inlets of a sweep tile.

Not product code: kept out of pydem_amd/synth.py on purpose."""
import numpy as np
from scipy import ndimage


def border_size(mask):
    """cells outside `mask` with an 8-neighbour in it, inside the tile (utils.get_border_index of the reference)"""
    return int((ndimage.binary_dilation(mask, structure=np.ones((3, 3), bool)) & ~mask).sum())


def basin(shape, floor, n_drains, pit=None, cone=True, dtype=np.float64, noise=0.0, seed=0):
    """A crater: floor cells (`floor`, a bool mask) enclosed by a rim (the 8-neighbour border of the floor) of which exactly
    `n_drains` cells are notched down below the floor, all to ONE elevation (tied drains); everything outside the rim falls
    away from it.  cone=True: the floor rises by Chebyshev rings from the single cell `pit`, so that cell is the only pit and
    its search adds one whole ring per iteration; cone=False: a flat floor, every floor cell a pit.
    The search of the pit (the centre one for a flat floor) ends when the region is the floor: the border is the whole rim and
    it holds `n_drains` drains.  noise > 0 perturbs the cells outside the floor and the rim by less than that (not the notches).
    Returns (elev, info) with info = {'pit', 'border', 'drains', 'iterations'}."""
    n, m = shape
    floor = np.asarray(floor, bool)
    assert floor.shape == shape
    d = ndimage.distance_transform_cdt(~floor, metric='chessboard')     # 0 on the floor, 1 on the rim
    rim = np.flatnonzero(d.ravel() == 1)
    ii, jj = np.indices(shape)
    if pit is None:
        fi, fj = np.nonzero(floor)
        pit = (int(np.rint(fi.mean())), int(np.rint(fj.mean())))
    assert floor[pit]
    rp = np.maximum(np.abs(ii - pit[0]), np.abs(jj - pit[1]))
    a = int(rp[floor].max())
    F = 1000.0
    step = 1.0 if np.issubdtype(np.dtype(dtype), np.integer) else 0.25
    top = F + step * a if cone else F
    R, D = top + 40.0, F - 20.0
    z = np.where(floor, F + step * rp if cone else F, D - 2.0 * d).astype(np.float64)
    zr = z.ravel()
    zr[rim] = R
    rng = np.random.default_rng(seed)
    # notches only where the rim touches the last ring of a cone floor: the search sees no drain before the whole floor is in
    cand = rim[rp.ravel()[rim] == rp.ravel()[rim].max()] if cone else rim
    assert n_drains <= cand.size, (n_drains, cand.size)
    notch = np.sort(rng.permutation(cand)[:n_drains])
    if noise:
        off = ~floor.ravel()
        zr[off] += rng.random(off.sum()) * noise
    zr[notch] = D
    # the tile's outer ring at 0: the cells where the slopes end are no pits (elev > 0 gates the search), so the only pit
    # searches are those of the floor
    z[0, :] = z[-1, :] = z[:, 0] = z[:, -1] = 0.0
    info = dict(pit=int(pit[0] * m + pit[1]), border=int(rim.size), drains=int(n_drains),
                iterations=(a + 1) if cone else None)
    return z.astype(dtype), info


def square_floor(shape, center, a):
    f = np.zeros(shape, bool)
    f[center[0] - a:center[0] + a + 1, center[1] - a:center[1] + a + 1] = True
    return f


def crater(a, n_drains, margin=4, dent=False, **kw):
    """basin() around a (2a+1)^2 floor in the middle of a square tile: rim of 8(a+1) cells.  dent=True: the middle cell of the
    floor's top row is left out (it joins the rim, the rim cell above it stays): 8(a+1) + 1 cells -- 33 for a = 3"""
    s = 2 * (a + 1 + margin) + 1
    c = s // 2
    f = square_floor((s, s), (c, c), a)
    if dent:
        f[c - a, c] = False
    return basin((s, s), f, n_drains, pit=(c, c), **kw)


def spacing(n, seed=0):
    """row-varying dX / dY (n - 1 values each, none of them short binary fractions: every sum rounds)"""
    rng = np.random.default_rng(seed)
    dX = 25.0 + 0.01 * np.arange(n - 1) + rng.random(n - 1) * 0.37
    dY = 31.0 - 0.004 * np.arange(n - 1) + rng.random(n - 1) * 0.29
    return dX, dY


def channel_plateau(length=320, width=9, n_rows=None, dtype=np.float64, noise=0.0, seed=0, pit_at_head=False):
    """A plane falling toward the last row, cut by one flat 1-cell channel of `length` rows in the middle column that opens
    at its lower end onto three lower cells.  Every channel cell but the last is a flat pit; the search of the pit k rows
    above the opening grows one channel cell per iteration and finds the three drains k + 1 rows away: with
    drain_pits_max_dist=None and drain_pits_max_iter=300 the row spans of the pit -> drain pairs run through 2..300
    (numpy's leaf sums, the 8-accumulator sums and the first levels of its pairwise split).
    pit_at_head: the top channel cell one unit lower (a strict local minimum for calc_pit_drain_paths, whose outlet search
    then walks the whole channel).  Returns (elev, info) with info['channel'] = (first row, last row, column)."""
    n = n_rows or length + 12
    m = width
    c = m // 2
    r1 = n - 4                       # last channel row
    r0 = r1 - length + 1
    assert r0 >= 2
    ii, jj = np.indices((n, m))
    z = 10.0 * (n - 1 - ii) + 0.5 * np.abs(jj - c) + 50.0
    if noise:
        z += np.random.default_rng(seed).random((n, m)) * noise
    h = 10.0 * (n - 1 - (r1 + 1)) + 50.0 + 5.0          # between the opening row (below) and the walls (above)
    z[r0:r1 + 1, c] = h
    if pit_at_head:
        z[r0, c] = h - 1.0
    return z.astype(dtype), dict(channel=(r0, r1, c))


def twin_outlets(L=150, width=5, seed=25):
    """A strict minimum in the middle of a flat 1-cell channel that opens L rows above and L rows below onto two outlets of
    one elevation: calc_pit_drain_paths reaches both in the same iteration and carves toward the one of smaller reach, the
    upper one on a tie (:509-512).  Both reaches are pure dY sums over L > 128 rows (same column, no run), and the dY of the
    upper span is a shuffle of the lower one, so the two sums differ by an ulp or two at most and which one is smaller turns
    on numpy's summation order.  Returns (elev, dX, dY, info) with info = {'pit', 'rise_up', 'rise_down'} (numpy's sums)."""
    n, m = 2 * L + 3, width
    c = m // 2
    ip = L + 1
    z = np.full((n, m), 200.0)
    z[0, :] = z[-1, :] = 0.0                       # sea rows: the outlets drain there, and are no pits themselves
    h = 100.0
    z[2:2 * L + 1, c] = h
    z[ip, c] = h - 1.0
    z[1, c] = z[2 * L + 1, c] = 50.0
    rng = np.random.default_rng(seed)
    v = 31.0 + rng.random(L) * 0.29
    dY = np.full(n - 1, 30.0)
    dY[ip:ip + L] = v
    dY[ip - L:ip] = rng.permutation(v)
    dX = np.full(n - 1, 25.0)
    info = dict(pit=ip * m + c, rise_up=np.add.reduce(dY[ip - L:ip]), rise_down=np.add.reduce(dY[ip:ip + L]))
    return z, dX, dY, info


class SplitMutantSum(np.ndarray):
    """a float64 vector whose .sum() is np_sum_split_mutant: the host twin run with it shows what a kernel that lost numpy's
    split would carve"""
    def sum(self, *a, **k):
        return np_sum_split_mutant(np.asarray(self))


def row_spans(pit_i, pit_j, m):
    return np.abs(np.asarray(pit_i) // m - np.asarray(pit_j) // m)


def np_sum_split_mutant(a):
    """numpy's pairwise sum without the `n2 -= n2 % 8` of its split: what a kernel that lost it would compute"""
    n = len(a)
    if n <= 128:
        return np.add.reduce(np.asarray(a, np.float64))
    n2 = n // 2
    return np_sum_split_mutant(a[:n2]) + np_sum_split_mutant(a[n2:])


def egg_crate(n, m, amp=50.0, tilt=1.0, noise=0.0, seed=0):
    """checkerboard on a tilt: every other cell a local crest that nothing drains into"""
    ii, jj = np.indices((n, m))
    z = tilt * (n - 1 - ii) + amp * ((ii + jj) % 2) + 100.0
    if noise:
        z += np.random.default_rng(seed).random((n, m)) * noise
    return z


def in_degree(A, nn):
    """in-edges per cell of the oracle's graph (CSC: column j lists the cells j drains into)"""
    indptr, indices, data = A
    return np.bincount(indices[data != 0], minlength=nn)


def max_sources_per_tile(deg, shape, T=32):
    """the largest count of in-degree-0 cells over the full 32 x 32 tiles of the sweep"""
    n, m = shape
    z = (deg.reshape(n, m) == 0)[:n // T * T, :m // T * T]
    return int(z.reshape(n // T, T, m // T, T).sum(axis=(1, 3)).max())


def funnel(n, center=None, holes=0, seed=0):
    """a bowl: every cell falls toward the `center` cell (a pit that never drains), so all of the halo of the tile around
    it flows in.  holes > 0: small one-cell sinks scattered on the slopes just outside that tile, whose pit search drains
    them into it -- inlets that arrive as pit sources"""
    ci, cj = center or (n // 2, n // 2)
    ii, jj = np.indices((n, n))
    z = np.hypot(ii - ci, jj - cj) * 3.0 + 10.0 + 0.001 * ii
    if holes:
        rng = np.random.default_rng(seed)
        ti, tj = ci // 32 * 32, cj // 32 * 32
        for _ in range(holes):
            side = rng.integers(4)
            k = int(rng.integers(2, 30))
            i, j = [(ti - 2, tj + k), (ti + 33, tj + k), (ti + k, tj - 2), (ti + k, tj + 33)][side]
            z[i, j] -= 4.0
    return z


def tile_inlets(A, shape, ti, tj, T=32):
    """halo cells of the 32 x 32 tile at (ti, tj) (tile units) with a graph edge into the tile, and pit sources outside the
    halo with one"""
    n, m = shape
    indptr, indices, data = A
    i0, j0 = ti * T, tj * T
    inside = np.zeros((n, m), bool)
    inside[i0:i0 + T, j0:j0 + T] = True
    halo = ndimage.binary_dilation(inside, structure=np.ones((3, 3), bool)) & ~inside
    src = np.repeat(np.arange(n * m), np.diff(indptr))
    into = inside.ravel()[indices] & (data != 0)
    s = np.unique(src[into])
    s = s[~inside.ravel()[s]]
    return int(halo.ravel()[s].sum()), int((~halo.ravel()[s]).sum())
