"""Elevation conditioning, host side: quantisation-pit filling, flat interpolation and pit drain paths.

These are the three steps the reference runs before the slope stencil when `fill_flats` /
`drain_pits_path` are set (creare-com/pydem v1.2.1, pydem/dem_processing.py: calc_fill_pit_artifacts
:396-426, calc_fill_flats :551-579 with _fill_flat :308-394, calc_pit_drain_paths :428-548, helpers
pydem/utils.py:270-468).  The product path runs them ON THE DEVICE (csrc/cond_device.hip, csrc/cond_paths.hip,
through DEMProcessor.calc_fill_flats / calc_pit_drain_paths -- tiles with no-data cells included since round 4: the
device replays scipy's ring filter where a NaN is near); this module is what remains on the host: masked arrays,
surfaces of a dtype the device cannot hold (int64), a tile whose no-data cells alternate along a line for longer than
the bounded replay looks back, and the rare tile on which the order-preserving parallel schedule of the pit paths
gives up.  It is also the twin the device path is tested against (its masks come from scipy itself).  The vectorised prologues stay in numpy / scipy.ndimage (3x3 filters,
connected-component labels, the argsort whose tie order is part of the result); the per-region / per-pit loops run in
the native library (csrc/cond_host.cpp, host code behind the same C-ABI).  Results are pinned bit for bit by
tests/golden/g5_* and g7_* (captured from the reference); the numpy statements the native loops were written from are
test infrastructure (tests/conditioning_numpy.py).
"""
import ctypes as C
import warnings

import numpy as np
from scipy import ndimage


def _native():
    from . import _ffi
    return _ffi.load()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)

_EIGHT = np.ones((3, 3), bool)
_CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
_RING = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]], bool)
_SQRT2 = np.sqrt(2.0)


def _sea_mask(a, below_sea):
    return (a != 0) if below_sea else (a > 0)


# ----------------------------------------------------------------------------------------------
# quantisation artefacts (reference :396-426)
# ----------------------------------------------------------------------------------------------
def fill_pit_artifacts(elev, maximum_pit_area=32.0, fill_flats_below_sea=False):
    """Raise by one unit every small flat depression whose whole 8-connected rim is exactly one unit
    higher -- the signature of integer quantisation.  Keeps the input dtype."""
    if np.ma.isMaskedArray(elev):
        elev = np.ma.filled(elev.astype(np.float64), np.nan)          # masked cells are no-data (:213-214)
    elev = np.asarray(elev)
    if elev.ndim != 2:
        raise ValueError("elevation must be a 2-D array")
    low = (ndimage.minimum_filter(elev, (3, 3)) >= elev) & _sea_mask(elev, fill_flats_below_sea)
    lab, nlab = ndimage.label(low, structure=_EIGHT)
    lab = np.ascontiguousarray(lab, np.int32)
    z = np.ascontiguousarray(elev, np.float64)
    up = np.empty(elev.shape, np.uint8)
    lib = _native()
    # (a float32 surface computes `rim - 1` in float32, :424: the library is told)
    if lib.pydem_cond_pit_artifacts(_ptr(z), elev.shape[0], elev.shape[1], _ptr(lab), int(nlab), float(maximum_pit_area),
                                    int(elev.dtype == np.float32), _ptr(up)):
        raise RuntimeError("pydem_cond_pit_artifacts failed")
    return elev + up.astype(elev.dtype)


# ----------------------------------------------------------------------------------------------
# flats (reference :551-579, :308-394)
# ----------------------------------------------------------------------------------------------
def fill_flats(elev, maximum_pit_area=32.0, fill_flats_below_sea=False, fill_flats_source_tol=1,
               fill_flats_peaks=True, fill_flats_pits=True):
    """calc_fill_flats (:551-579): artefact pits first (when maximum_pit_area is set), then every flat is
    re-surfaced between its uphill rim and its outlet.  Returns float64."""
    if maximum_pit_area:
        elev = fill_pit_artifacts(elev, maximum_pit_area, fill_flats_below_sea)
    data = np.ascontiguousarray(np.ma.filled(np.asarray(elev).astype('float64'), np.nan))
    built = data.copy()
    flat = (ndimage.minimum_filter(data, (3, 3)) >= data) & _sea_mask(data, fill_flats_below_sea)
    flat[0, 0] = flat[-1, 0] = flat[0, -1] = flat[-1, -1] = False          # corners never (:569-572)
    lab, nlab = ndimage.label(flat, structure=_EIGHT)
    lab = np.ascontiguousarray(lab, np.int32)
    lib = _native()
    if lib.pydem_cond_fill_flats(_ptr(data), _ptr(built), data.shape[0], data.shape[1], _ptr(lab), int(nlab),
                                 float(fill_flats_source_tol), int(bool(fill_flats_peaks)), int(bool(fill_flats_pits))):
        raise RuntimeError("pydem_cond_fill_flats failed")
    return built


# ----------------------------------------------------------------------------------------------
# pit drain paths (reference :428-548)
# ----------------------------------------------------------------------------------------------
def pit_drain_paths(elev, dX, dY, drain_pits_max_iter=300, drain_pits_max_dist=32, drain_pits_max_dist_XY=None,
                    fill_flats_below_sea=False):
    """calc_pit_drain_paths (:428-548): every strict local minimum, lowest first, is connected to the first
    lower cell found by growing a region through its lowest rim cells; the cells on the way get elevations
    that fall linearly from pit to outlet.  The surface is edited IN PLACE and sequentially -- later pits
    see earlier paths -- in the array's own dtype, exactly like the reference (integer surfaces truncate the
    path values, float32 surfaces round them).  Returns (elev, n_failed, max_iter_used)."""
    if np.ma.isMaskedArray(elev):
        elev = np.ma.filled(elev.astype(np.float64), np.nan)
    elev = np.asarray(elev)
    if elev.ndim != 2:
        raise ValueError("elevation must be a 2-D array")
    if not (elev.flags.c_contiguous and elev.flags.writeable):
        elev = np.array(elev, order='C')
    dtype = elev.dtype
    # the library works on float64 values; `mode` tells it the dtype whose rounding the stored path values get (:539)
    mode = 0 if dtype == np.float64 else (2 if dtype == np.float32 else (1 if dtype.kind in 'iu' else None))
    if mode is None:
        raise TypeError("unsupported elevation dtype %r" % (dtype,))
    e = elev.ravel()
    lows = (ndimage.minimum_filter(elev, footprint=_RING).ravel() > e) & _sea_mask(e, fill_flats_below_sea)
    pit_ids = np.where(lows)[0]
    # the reference's own call on the array's own dtype (:450): the tie order of numpy's sort is part of the result
    order = np.ascontiguousarray(pit_ids[np.argsort(e[pit_ids])], np.int64)
    work = elev if mode == 0 else np.ascontiguousarray(elev, np.float64)
    dXc = np.ascontiguousarray(dX, np.float64)
    dYc = np.ascontiguousarray(dY, np.float64)
    failed = C.c_int64(0)
    used = C.c_int64(0)
    lib = _native()
    if lib.pydem_cond_pit_paths(_ptr(work), elev.shape[0], elev.shape[1], _ptr(order), order.size, _ptr(dXc), dXc.size, _ptr(dYc),
                                int(drain_pits_max_iter), int(drain_pits_max_dist or 0),
                                float(drain_pits_max_dist_XY) if drain_pits_max_dist_XY else 0.0, int(mode), C.byref(failed), C.byref(used)):
        raise RuntimeError("pydem_cond_pit_paths failed")
    if mode != 0:
        elev[...] = work.astype(dtype)
    if failed.value:
        warnings.warn("Warning %d pits had no place to drain to in this chunk" % failed.value)
    return elev, int(failed.value), int(used.value)


# ---- depression filling (no reference method): the host twin of pydem_fill_depressions (csrc/fill_depressions.hip) ----
def fill_depressions_epsilon(z, epsilon):
    """The epsilon a fill of the float64 surface `z` (NaN: no data) uses, by the rules of pydem_fill_depressions
    (include/pydem_hip.h): None is automatic, 2**-32 times the smallest power of two >= max |z| over the finite cells (1.0 if that
    is 0); a finite value >= 0 is used as given.  ValueError for a negative or non-finite value and for one that vanishes
    when it is added to max |z|."""
    with np.errstate(invalid='ignore'):
        fin = np.abs(z[np.isfinite(z)])
    amax = float(fin.max()) if fin.size else 0.0
    if epsilon is None:
        if amax > 0:
            f, e = np.frexp(amax)
            e = int(e) - 1 if f == 0.5 else int(e)
        else:
            e = 0
        with np.errstate(over='ignore', under='ignore'):
            eps = float(np.ldexp(1.0, e - 32))
        if not (eps > 0 and np.isfinite(eps)):
            raise ValueError("fill_depressions: no automatic epsilon for max |z| = %r" % amax)
    else:
        try:
            eps = float(epsilon)
        except (TypeError, ValueError):
            raise ValueError("fill_depressions: epsilon must be a number >= 0 or None (got %r)" % (epsilon,))
        if not (np.isfinite(eps) and eps >= 0):
            raise ValueError("fill_depressions: epsilon must be finite and >= 0, or None for the automatic value (got %r)" % (epsilon,))
    if eps > 0 and amax + eps == amax:
        raise ValueError("fill_depressions: epsilon %r is not representable at the surface's magnitude (max |z| = %r)" % (eps, amax))
    return eps


def _fill_inputs(what, elev, outlets):
    """(z, nan, is_open) of a fill: the float64 surface (masked cells and NaN are no data), its no-data mask and its open cells"""
    if np.ma.isMaskedArray(elev):
        z = np.ma.filled(elev.astype(np.float64), np.nan)
    else:
        z = np.array(elev, dtype=np.float64)
    if z.ndim != 2:
        raise ValueError("%s: a 2-D elevation array is needed (got shape %r)" % (what, z.shape))
    if np.isinf(z).any():
        raise ValueError("%s: the elevation holds +-inf" % what)
    n, m = z.shape
    nan = np.isnan(z)
    is_open = np.zeros((n, m), bool)
    if n and m:
        is_open[0, :] = is_open[-1, :] = True
        is_open[:, 0] = is_open[:, -1] = True
    if nan.any():
        is_open |= ndimage.binary_dilation(nan, structure=_EIGHT)
    if outlets is not None:
        o = np.asarray(outlets)
        if o.shape != z.shape:
            raise ValueError("%s: outlets of shape %r for a surface of shape %r" % (what, o.shape, z.shape))
        is_open |= o.astype(bool)
    is_open &= ~nan
    return z, nan, is_open


def fill_depressions(elev, epsilon=None, outlets=None):
    """Depression filling by priority flood + epsilon (Barnes et al. 2014) with the semantics of pydem_fill_depressions
    (include/pydem_hip.h): open cells -- the finite cells on the border, beside a no-data cell, or marked in the boolean mask
    `outlets` -- keep their elevation, and every other finite cell becomes max(z, min over its finite 8-neighbours of (W + eps)),
    the greatest such surface.  Masked cells and NaN are no data.  Returns (W, depth, epsilon_used): float64 arrays (depth = W - z,
    NaN where z is) and the epsilon the call used.  It serves what the device path does not take: masked arrays, dtypes the
    device cannot hold, tiles with fewer than three rows or columns."""
    import heapq
    z, nan, is_open = _fill_inputs("fill_depressions", elev, outlets)
    n, m = z.shape
    eps = fill_depressions_epsilon(z, epsilon)
    W = np.where(nan, np.nan, np.inf)
    W[is_open] = z[is_open]
    zl = z.tolist()
    seen = (is_open | nan).tolist()
    heap = [(zl[r][c], r, c) for r, c in zip(*np.nonzero(is_open))]
    heapq.heapify(heap)
    out = []
    while heap:
        w, r, c = heapq.heappop(heap)
        s = w + eps                                 # (the same for the eight neighbours)
        for rr in (r - 1, r, r + 1):
            if rr < 0 or rr >= n:
                continue
            row_seen, row_z = seen[rr], zl[rr]
            for cc in (c - 1, c, c + 1):
                if cc < 0 or cc >= m or row_seen[cc]:
                    continue
                row_seen[cc] = True
                v = s if s > row_z[cc] else row_z[cc]
                out.append((rr, cc, v))
                heapq.heappush(heap, (v, rr, cc))
    if out:
        rr, cc, vv = zip(*out)
        W[np.array(rr), np.array(cc)] = np.array(vv, np.float64)
    return W, W - z, eps


# ---- depression filling across tiles: the host twin of the pydem_fill_seam_* session (csrc/fill_depressions.hip) ----
SEAM_SIDES = ('top', 'bottom', 'left', 'right')


def _side_index(side, n, m):
    """the cells of a tile's border line as an index into an (n, m) array"""
    return {'top': (0, slice(None)), 'bottom': (n - 1, slice(None)), 'left': (slice(None), 0), 'right': (slice(None), m - 1)}[side]


class SeamFill(object):
    """One tile's part of a fill across tiles, with the semantics of pydem_fill_seam_begin / _relax / _get_lines / _end
    (include/pydem_hip.h).  `seam_lines`: {'top' | 'bottom' | 'left' | 'right': boolean line} (missing or None: none), the
    border cells whose 8 lattice neighbours other tiles hold: they are not open by position.  W starts at z on the open cells --
    the other border cells, cells beside no data, `outlets` -- and at +inf elsewhere; `relax(eps, caps)` lowers it to the
    greatest solution of W = max(z, min(cap, min over the in-tile finite neighbours of (W + eps))) that lies below what it
    holds, with a heap-ordered flood from the open cells (first call) and from the cells whose cap fell.  Caps may only fall
    (ValueError otherwise); NaN in a cap counts as +inf.  It also serves the tiles the device does not take (fewer than three
    rows or columns, masked arrays)."""

    def __init__(self, z, outlets=None, seam_lines=None):
        self.z, self.nan, _ = _fill_inputs("SeamFill", z, outlets)
        n, m = self.z.shape
        self.shape = (n, m)
        seam = np.zeros((n, m), bool)
        for side in SEAM_SIDES:
            line = None if seam_lines is None else seam_lines.get(side)
            if line is not None:
                line = np.asarray(line).astype(bool)
                if line.shape != np.shape(seam[_side_index(side, n, m)]):
                    raise ValueError("SeamFill: seam line %r of shape %r for a tile of shape %r" % (side, line.shape, (n, m)))
                seam[_side_index(side, n, m)] |= line
        by_position = np.zeros((n, m), bool)
        if n and m:
            by_position[0, :] = by_position[-1, :] = True
            by_position[:, 0] = by_position[:, -1] = True
        # open: as in fill_depressions, except that a seam cell is not open by position
        is_open = by_position & ~seam
        if self.nan.any():
            is_open |= ndimage.binary_dilation(self.nan, structure=_EIGHT)
        if outlets is not None:
            is_open |= np.asarray(outlets).astype(bool)
        self.is_open = is_open & ~self.nan
        self.outlets = None if outlets is None else np.asarray(outlets).astype(bool)
        with np.errstate(invalid='ignore'):
            fin = np.abs(self.z[~self.nan])
        self.amax = float(fin.max()) if fin.size else 0.0
        self.W = np.where(self.nan, np.nan, np.inf)
        self.W[self.is_open] = self.z[self.is_open]
        self.cap = np.full((n, m), np.inf)
        self.eps = None
        self._first = True

    def relax(self, eps, caps=None):
        """Lower W to the fixed point for `caps` ({side: float64 line}; a missing side keeps its caps; at a corner the smaller of two
        lines counts).  Returns the number of cells whose W fell."""
        import heapq
        eps = float(eps)
        if not (np.isfinite(eps) and eps >= 0):
            raise ValueError("SeamFill.relax: epsilon must be finite and >= 0 (got %r)" % (eps,))
        if self.eps is not None and eps != self.eps:
            raise ValueError("SeamFill.relax: epsilon %r, the session began with %r" % (eps, self.eps))
        if eps > 0 and self.amax + eps == self.amax:
            raise ValueError("SeamFill.relax: epsilon %r is not representable at the surface's magnitude (max |z| = %r)" % (eps, self.amax))
        n, m = self.shape
        lines = getattr(self, '_cap_lines', None)
        if lines is None:
            lines = self._cap_lines = {side: np.full(np.shape(self.cap[_side_index(side, n, m)]), np.inf) for side in SEAM_SIDES}
        new = {}
        for side in SEAM_SIDES:
            line = None if caps is None else caps.get(side)
            if line is None:
                continue
            line = np.array(line, np.float64)
            if line.shape != lines[side].shape:
                raise ValueError("SeamFill.relax: cap line %r of shape %r for a tile of shape %r" % (side, line.shape, (n, m)))
            line[np.isnan(line)] = np.inf
            if (line > lines[side]).any():
                raise ValueError("SeamFill.relax: cap line %r rises above the cap the session holds; caps may only fall" % side)
            new[side] = line
        self.eps = eps
        lines.update(new)
        cap = np.full((n, m), np.inf)
        for side in SEAM_SIDES:
            idx = _side_index(side, n, m)
            cap[idx] = np.minimum(cap[idx], lines[side])
        fell = cap < self.cap
        self.cap = cap
        before = self.W.copy()
        W, zl, capl = self.W.tolist(), self.z.tolist(), cap.tolist()
        fixed = (self.is_open | self.nan).tolist()
        heap = []
        if self._first:
            heap = [(W[r][c], r, c) for r, c in zip(*np.nonzero(self.is_open))]
            self._first = False
        for r, c in zip(*np.nonzero(fell & ~self.is_open & ~self.nan)):
            v = capl[r][c] if capl[r][c] > zl[r][c] else zl[r][c]
            if v < W[r][c]:
                W[r][c] = v
                heap.append((v, int(r), int(c)))
        heapq.heapify(heap)
        while heap:
            w, r, c = heapq.heappop(heap)
            if w > W[r][c]:
                continue                            # (the cell fell again after this entry was pushed)
            s = w + eps
            for rr in (r - 1, r, r + 1):
                if rr < 0 or rr >= n:
                    continue
                row_fixed, row_z, row_W, row_cap = fixed[rr], zl[rr], W[rr], capl[rr]
                for cc in (c - 1, c, c + 1):
                    if cc < 0 or cc >= m or row_fixed[cc]:
                        continue
                    v = s if s < row_cap[cc] else row_cap[cc]
                    if not v > row_z[cc]:
                        v = row_z[cc]
                    if v < row_W[cc]:
                        row_W[cc] = v
                        heapq.heappush(heap, (v, rr, cc))
        self.W = np.array(W, np.float64).reshape(n, m)
        with np.errstate(invalid='ignore'):
            return int(np.count_nonzero(self.W < before))

    def lines(self, requests):
        """[(axis, index)] -> rows (axis 0) and columns (axis 1) of W, copies"""
        return [np.array(self.W[index, :] if axis == 0 else self.W[:, index]) for axis, index in requests]

    def end(self, commit=True):
        """commit: (W, depth) -- RuntimeError while W still holds +inf; otherwise None.  The session is over either way."""
        if not commit:
            return None
        if np.isinf(self.W).any():
            raise RuntimeError("SeamFill.end: %d cells of W are still +inf (no relaxation has reached them)" % int(np.isinf(self.W).sum()))
        return self.W, self.W - self.z

    # ---- the inventory across tiles: the twin of pydem_fill_seam_label / _get_id_lines / _inventory / _labels (include/pydem_hip.h)
    ids = None                    # the plane of local ids after label()

    def label(self):
        """The 8-connected components of W > z inside the tile, numbered in ascending order of their first cell: (roots, levels,
        largest depth) -- the first cell (int32 linear index) and the level of each.  RuntimeError while W holds +inf."""
        if np.isinf(self.W).any():
            raise RuntimeError("SeamFill.label: cells of W are still +inf (no relaxation has reached them)")
        with np.errstate(invalid='ignore'):
            raised = self.W > self.z
        lab, K = ndimage.label(raised, structure=_EIGHT)
        self.ids = np.where(self.nan, -1, lab).astype(np.int32)
        idx = np.flatnonzero(raised)
        roots = np.zeros(K, np.int32)
        roots[lab.ravel()[idx[::-1]] - 1] = idx[::-1]               # (the last store of a label is its smallest index)
        depth = self.W.ravel()[idx] - self.z.ravel()[idx]
        return roots, self.W.ravel()[roots], float(depth.max()) if K else 0.0

    def _labelled(self, what):
        if self.ids is None:
            raise RuntimeError("SeamFill.%s: the session has no labels (label first)" % what)

    def id_lines(self, requests):
        """[(axis, index)] -> rows (axis 0) and columns (axis 1) of the id plane, copies"""
        self._labelled('id_lines')
        return [np.array(self.ids[index, :] if axis == 0 else self.ids[:, index]) for axis, index in requests]

    def inventory(self, lut, n_rows, owner, halo_ids, halo_W, row_area, shift_area, shift_volume):
        """The tile's partial table over the cells `owner` marks: uint64 [len(SEAM_TABLE_COLS), n_rows], word for word what
        pydem_fill_seam_inventory returns (include/pydem_hip.h has every argument and column).  The outlets are those of the
        session."""
        self._labelled('inventory')
        n, m = self.shape
        NN, T = n * m, int(n_rows)
        lut = np.asarray(lut, np.int64)
        halo_ids, halo_W = np.asarray(halo_ids, np.int64), np.asarray(halo_W, np.float64)
        if lut.shape != (int(self.ids.max(initial=0)) + 1,) or halo_ids.shape != (2 * m + 2 * n + 4,) or halo_W.shape != halo_ids.shape:
            raise ValueError("SeamFill.inventory: lookup of shape %r, halo of shape %r for a tile of shape %r" % (lut.shape, halo_ids.shape, (n, m)))
        if lut.min(initial=0) < 0 or lut.max(initial=0) > T or halo_ids.min() < -1 or halo_ids.max() > T:
            raise ValueError("SeamFill.inventory: a lookup or halo entry outside 0 (-1) .. %d" % T)
        col = {nm: k for k, nm in enumerate(SEAM_TABLE_COLS)}
        tab = np.zeros((len(SEAM_TABLE_COLS), T), np.uint64)
        for nm in ('r0', 'c0', 'zmin', 'bottom', 'pour'):
            tab[col[nm]] = ~np.uint64(0)
        if T == 0:
            return tab
        owner = np.asarray(owner).astype(bool)
        ra = np.ascontiguousarray(row_area, np.float64)
        z, W = self.z, self.W
        g = np.where(self.ids > 0, lut[np.maximum(self.ids, 0)], np.where(self.ids < 0, -1, 0))        # rows, 0, -1 per cell
        idx = np.flatnonzero(owner & (g > 0))
        k = g.ravel()[idx] - 1
        r, c = idx // m, idx % m
        zc = z.ravel()[idx]
        key = (zc + 0.0).view(np.uint64)
        key = np.where(key >> np.uint64(63), ~key, key | np.uint64(1 << 63))
        tab[col['cells']] = np.bincount(k, minlength=T).astype(np.uint64)
        for nm, v, op in (('r0', r, np.minimum), ('r1', r, np.maximum), ('c0', c, np.minimum), ('c1', c, np.maximum), ('zmin', key, np.minimum)):
            op.at(tab[col[nm]], k, v.astype(np.uint64))
        low = key == tab[col['zmin']][k]
        np.minimum.at(tab[col['bottom']], k[low], idx[low].astype(np.uint64))
        has = tab[col['bottom']] < NN
        tab[col['bottom_elev']][has] = z.ravel()[tab[col['bottom']][has].astype(np.int64)].view(np.uint64)
        depth = W.ravel()[idx] - zc
        for nm, terms in (('area', np.ldexp(ra[r], int(shift_area))), ('volume', np.ldexp(depth * ra[r], int(shift_volume)))):
            s = np.zeros(T, np.int64)
            np.add.at(s, k, np.rint(terms).astype(np.int64))
            tab[col[nm]] = s.view(np.uint64)
        # sills, on the window with its halo ring
        gp = np.zeros((n + 2, m + 2), np.int64)
        Wp = np.zeros((n + 2, m + 2))
        gp[1:-1, 1:-1], Wp[1:-1, 1:-1] = g, W
        for plane, halo in ((gp, halo_ids), (Wp, halo_W)):
            plane[0, :], plane[-1, :] = halo[:m + 2], halo[m + 2:2 * m + 4]
            plane[1:-1, 0], plane[1:-1, -1] = halo[2 * m + 4:2 * m + 4 + n], halo[2 * m + 4 + n:]
        cand = owner & (self.ids == 0)
        is_open = np.zeros((n, m), bool) if self.outlets is None else self.outlets.copy()
        pairs = []
        for dr in (0, 1, 2):
            for dc in (0, 1, 2):
                if dr == 1 and dc == 1:
                    continue
                nl = gp[dr:dr + n, dc:dc + m]
                is_open |= nl < 0
                with np.errstate(invalid='ignore'):
                    cell = np.flatnonzero(cand & (nl > 0) & (Wp[dr:dr + n, dc:dc + m] == z))
                pairs.append((nl.ravel()[cell] - 1) * NN + cell)
        pairs = np.unique(np.concatenate(pairs))
        sl, sc = pairs // NN, pairs % NN
        tab[col['n_sills']] = np.bincount(sl, minlength=T).astype(np.uint64)
        np.minimum.at(tab[col['pour']], sl, sc.astype(np.uint64))
        np.maximum.at(tab[col['open']], sl, is_open.ravel()[sc].astype(np.uint64))
        return tab

    def labels(self, lut):
        """the label plane: lut[local id] on raised cells, 0 and -1 as in the id plane"""
        self._labelled('labels')
        lut = np.asarray(lut, np.int32)
        return np.where(self.ids > 0, lut[np.maximum(self.ids, 0)], self.ids).astype(np.int32)


# the columns of a tile's partial table (pydem_fill_seam_inventory, SeamFill.inventory), and the key of a double in 'zmin'
SEAM_TABLE_COLS = ('cells', 'r0', 'r1', 'c0', 'c1', 'zmin', 'bottom', 'pour', 'n_sills', 'open', 'area', 'volume', 'bottom_elev')


# ---- depression inventory (no reference method): the host twin of pydem_depressions (csrc/depressions.hip) ----
DEPRESSION_DTYPE = np.dtype([('cells', np.int64), ('r0', np.int64), ('r1', np.int64), ('c0', np.int64), ('c1', np.int64),
                             ('spill_elev', np.float64), ('bottom_row', np.int64), ('bottom_col', np.int64), ('bottom_elev', np.float64),
                             ('max_depth', np.float64), ('pour_row', np.int64), ('pour_col', np.int64), ('n_sills', np.int64),
                             ('open_sill', np.int64), ('area', np.float64), ('volume', np.float64), ('mean_depth', np.float64)])


def fixed_point(cells, largest):
    """(shift, quantum) of the fixed-point sums of pydem_depressions: B = min(40, 62 - ceil(log2(max(cells, 2)))) fraction bits,
    E from frexp of the largest term; a term p adds rint(ldexp(p, shift)), shift = B - E, and the quantum is 2**(E - B)."""
    B = min(40, 62 - (max(int(cells), 2) - 1).bit_length())
    E = int(np.frexp(float(largest))[1])
    return B - E, float(np.ldexp(1.0, E - B))


def depression_limits(what, **limits):
    """the limits of a depression filter as numbers >= 0 (None stays None); ValueError otherwise"""
    out = {}
    for nm, v in limits.items():
        if v is not None:
            try:
                v = float(v) if 'cells' not in nm else int(v)
            except (TypeError, ValueError):
                raise ValueError("%s: %s must be a number >= 0 (got %r)" % (what, nm, v))
            if not (v >= 0) or not np.isfinite(v):
                raise ValueError("%s: %s must be finite and >= 0 (got %r)" % (what, nm, v))
        out[nm] = v
    return out


def depression_table(cells, r0, r1, c0, c1, spill, bottom, bottom_elev, pour, n_sills, open_sill, area, volume, m):
    """the structured table of calc_depressions from its columns (bottom and pour as linear indices r * m + c)"""
    t = np.zeros(len(cells), DEPRESSION_DTYPE)
    t['cells'], t['r0'], t['r1'], t['c0'], t['c1'] = cells, r0, r1, c0, c1
    t['spill_elev'], t['bottom_elev'] = spill, bottom_elev
    t['bottom_row'], t['bottom_col'] = np.asarray(bottom) // m, np.asarray(bottom) % m
    t['pour_row'], t['pour_col'] = np.asarray(pour) // m, np.asarray(pour) % m
    t['max_depth'] = t['spill_elev'] - t['bottom_elev']
    t['n_sills'], t['open_sill'], t['area'], t['volume'] = n_sills, open_sill, area, volume
    t['mean_depth'] = t['volume'] / t['area']
    return t


def label_depressions(elev, outlets=None, min_depth=0.0, min_cells=1, min_volume=0.0, dX2dY2=None):
    """The depression inventory with the semantics of pydem_depressions (include/pydem_hip.h): W is the classic fill (epsilon 0) of
    the surface, a depression an 8-connected component of W > z, numbered in ascending order of its smallest linear index.  Returns
    (label, table, quanta): the int32 label raster (0: in no kept depression, -1: no data), the structured table (DEPRESSION_DTYPE;
    area and volume are the fixed-point sums of the header, in the units of dX2dY2 -- the cell area per row, 1 by default) and the
    quanta (area, volume) of those sums.  Depressions below min_depth, min_cells or min_volume are dropped and the rest renumbered
    in the same order.  It serves what the device path does not take: masked arrays, dtypes the device cannot hold, tiles with
    fewer than three rows or columns."""
    lim = depression_limits("label_depressions", min_depth=min_depth, min_cells=min_cells, min_volume=min_volume)
    z, nan, is_open = _fill_inputs("label_depressions", elev, outlets)
    n, m = z.shape
    ra = np.ones(n) if dX2dY2 is None else np.ascontiguousarray(dX2dY2, np.float64)
    if ra.shape != (n,):
        raise ValueError("label_depressions: dX2dY2 of shape %r for %d rows" % (ra.shape, n))
    W = fill_depressions(z, 0.0, outlets)[0]
    with np.errstate(invalid='ignore'):
        raised = W > z
    lab, K = ndimage.label(raised, structure=_EIGHT)            # numbered in raster order of each component's first cell
    amax = float(ra.max()) if n else 0.0
    idx = np.flatnonzero(raised)
    depth = W.ravel()[idx] - z.ravel()[idx]
    sh_a, q_a = fixed_point(n * m, amax)
    sh_v, q_v = fixed_point(n * m, (float(depth.max()) if K else 0.0) * amax)
    label = np.where(nan, -1, 0).astype(np.int32)
    if K == 0:
        return label, np.zeros(0, DEPRESSION_DTYPE), (q_a, q_v)
    order = np.argsort(lab.ravel()[idx], kind='stable')         # by label, ascending index within a label
    idx, depth = idx[order], depth[order]
    cells = np.bincount(lab.ravel()[idx] - 1, minlength=K).astype(np.int64)
    first = np.concatenate(([0], np.cumsum(cells)[:-1]))
    r, c = idx // m, idx % m
    zc = z.ravel()[idx]
    zmin = np.minimum.reduceat(zc, first)
    bottom = np.minimum.reduceat(np.where(zc == np.repeat(zmin, cells), idx, n * m), first)
    spill = W.ravel()[idx[first]]
    area = np.add.reduceat(np.rint(np.ldexp(ra[r], sh_a)).astype(np.int64), first)
    volume = np.add.reduceat(np.rint(np.ldexp(depth * ra[r], sh_v)).astype(np.int64), first)
    # sills: finite cells that are not raised, beside a depression whose level is their elevation
    cand = ~raised & ~nan
    lp = np.pad(lab, 1)
    Wp = np.pad(W, 1, constant_values=np.nan)
    pairs = []
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if dr == 1 and dc == 1:
                continue
            nl = lp[dr:dr + n, dc:dc + m]
            with np.errstate(invalid='ignore'):
                hit = cand & (nl > 0) & (Wp[dr:dr + n, dc:dc + m] == z)
            cell = np.flatnonzero(hit)
            pairs.append((nl.ravel()[cell].astype(np.int64) - 1) * (n * m) + cell)
    pairs = np.unique(np.concatenate(pairs))
    sl, sc = pairs // (n * m), pairs % (n * m)
    n_sills = np.bincount(sl, minlength=K).astype(np.int64)
    if (n_sills == 0).any():
        raise RuntimeError("label_depressions: a depression without a sill cell")
    sfirst = np.concatenate(([0], np.cumsum(n_sills)[:-1]))
    pour = sc[sfirst]                                           # (np.unique sorted them: the smallest cell of each label comes first)
    open_sill = np.maximum.reduceat(is_open.ravel()[sc].astype(np.int64), sfirst)
    table = depression_table(cells, np.minimum.reduceat(r, first), np.maximum.reduceat(r, first), np.minimum.reduceat(c, first),
                             np.maximum.reduceat(c, first), spill, bottom, z.ravel()[bottom], pour, n_sills, open_sill,
                             area.astype(np.float64) * q_a, volume.astype(np.float64) * q_v, m)
    keep = (table['max_depth'] >= lim['min_depth']) & (table['cells'] >= lim['min_cells']) & (table['volume'] >= lim['min_volume'])
    lut = np.zeros(K + 1, np.int32)
    lut[1:][keep] = np.arange(1, int(keep.sum()) + 1)
    label = np.where(nan, -1, lut[lab]).astype(np.int32)
    return label, table[keep], (q_a, q_v)


def over_limits(table, max_depth=None, max_cells=None, max_volume=None):
    """the depressions of `table` that exceed one of the given limits (boolean array)"""
    over = np.zeros(len(table), bool)
    if max_depth is not None:
        over |= table['max_depth'] > max_depth
    if max_cells is not None:
        over |= table['cells'] > max_cells
    if max_volume is not None:
        over |= table['volume'] > max_volume
    return over


def limited_outlets(inventory, shape, outlets, max_depth, max_cells, max_volume, max_rounds):
    """The loop of the limited fill: `inventory(mask)` returns the depression table under the outlets `mask`; the bottoms of the
    depressions over a limit become outlets until none is over one.  Every round adds at least one new outlet (a bottom is a
    raised cell, so it was none).  Returns (mask, kept_sinks [N, 2]); RuntimeError when max_rounds rounds did not suffice."""
    mask = np.zeros(shape, bool) if outlets is None else np.array(outlets, dtype=bool)
    kept = np.zeros((0, 2), np.int64)
    for rnd in range(int(max_rounds) + 1):
        table = inventory(mask)
        over = over_limits(table, max_depth, max_cells, max_volume)
        if not over.any():
            return mask, kept
        if rnd == int(max_rounds):
            break
        new = np.stack([table['bottom_row'][over], table['bottom_col'][over]], axis=1)
        mask[new[:, 0], new[:, 1]] = True
        kept = np.concatenate([kept, new])
    raise RuntimeError("fill_depressions_limited: depressions over the limits remain after %d rounds (max_rounds)" % int(max_rounds))


def fill_depressions_limited(elev, max_depth=None, max_cells=None, max_volume=None, epsilon=None, outlets=None, max_rounds=64,
                             dX2dY2=None):
    """The z-limit fill (ArcGIS Fill's z-limit, WhiteboxTools' max_depth): a depression deeper than max_depth, larger than
    max_cells or holding more than max_volume is kept, everything else is filled -- the shallow depressions nested inside a kept
    one included.  The inventory (label_depressions) is taken with the outlets collected so far, the bottoms of the depressions
    over a limit join the outlets, and when none is over a limit one fill_depressions(epsilon, outlets=collected) follows.
    Returns (W, depth, epsilon_used, kept_sinks): kept_sinks is the (N, 2) int array of the outlets the loop added.  RuntimeError
    after max_rounds rounds, with the input untouched.  With no limit it is fill_depressions."""
    lim = depression_limits("fill_depressions_limited", max_depth=max_depth, max_cells=max_cells, max_volume=max_volume)
    z, nan, _ = _fill_inputs("fill_depressions_limited", elev, outlets)
    if all(v is None for v in lim.values()):
        return fill_depressions(elev, epsilon, outlets) + (np.zeros((0, 2), np.int64),)
    mask, kept = limited_outlets(lambda o: label_depressions(z, o, dX2dY2=dX2dY2)[1], z.shape, outlets, lim['max_depth'],
                                 lim['max_cells'], lim['max_volume'], max_rounds)
    return fill_depressions(z, epsilon, mask) + (kept,)
