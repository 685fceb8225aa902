"""Large tiles for the depression fill and the depression inventory whose exact answer is cheap (tests/test_large_depression_fields.py
ties them to the host twins at a small size, tests/test_gpu_depressions_large.py holds the device against them above the sizes at
which its capped grids loop and the fixed-point sums lose a fraction bit).

Mosaic: copies of the small designed fields, shelf-packed with one no-data row or column between neighbours, the rest of the tile no
data.  A border cell of an embedded patch lies beside no data or on the tile's border: it is open, as it is in the patch alone.  The
open sets coincide, so the fill of the mosaic is the mosaic of the patch fills and its depressions are those of the patches; only
epsilon (from the whole tile's max |z|), the numbering (by smallest linear index in the tile) and the fixed-point sums (the tile's
cell count, row areas and largest term) belong to the tile, and they are formed here with numpy.

Great lake: a border ring whose unique lowest cell (S, not a corner) touches an interior that lies below S everywhere.  W = S on the
interior, one depression; every column follows from z alone."""
import numpy as np

import depression_fields as D
import fill_fields as F

# ---- the patches -------------------------------------------------------------------------------------------------------------------
_PATCH = {}
_PATCH_FILL = {}
_PATCH_LABEL = {}


def patch_builders():
    d = dict(D.builders())
    d.update(F.designed())
    d['fractal96'] = lambda: F.fractal(96, 80)
    return d


def patch(name):
    """the float64 surface of a patch, built once"""
    if name not in _PATCH:
        _PATCH[name] = np.array(patch_builders()[name](), dtype=np.float64)
    return _PATCH[name]


def patch_fill(name, eps):
    """W of the host flood of the patch alone under an explicit epsilon, computed once"""
    if (name, eps) not in _PATCH_FILL:
        from pydem_amd import conditioning
        _PATCH_FILL[name, eps] = conditioning.fill_depressions(patch(name), eps)[0]
    return _PATCH_FILL[name, eps]


def patch_labels(name):
    """(label raster, K, first): the host twin's labels of the patch alone and the local linear index of each depression's first
    cell, computed once"""
    if name not in _PATCH_LABEL:
        from pydem_amd import conditioning
        lab, table, _ = conditioning.label_depressions(patch(name))
        flat = lab.ravel()
        idx = np.flatnonzero(flat > 0)
        ids, at = np.unique(flat[idx], return_index=True)           # (first occurrence in raster order)
        assert np.array_equal(ids, np.arange(1, len(table) + 1))
        _PATCH_LABEL[name] = lab, len(table), idx[at]
    return _PATCH_LABEL[name]


# The order of the shelves' cycle: the 961-pit checkerboard comes round three times as often as the others.
def cycle():
    names = sorted(patch_builders())
    out = []
    for i, nm in enumerate(names):
        out.append(nm)
        if i % 8 == 3:
            out.append('checkerboard')
    return out


# ---- the tile's own numbers ------------------------------------------------------------------------------------------------------
def spacing(n):
    """DEMProcessor spacing keywords of an n-row tile whose cell area falls from row to row (as depression_fields.varying_spacing_kwargs
    does on its 50 rows): 30 m of latitude, 30 m * cos(40 .. 50 degrees) of longitude"""
    dX2 = 30.0 * np.cos(np.deg2rad(40.0 + (10.0 / n) * np.arange(n)))
    return dict(dX=0.5 * (dX2[:-1] + dX2[1:]), dY=np.full(n - 1, 30.0), dX2=dX2, dY2=np.full(n, 30.0))


def row_area(n):
    kw = spacing(n)
    return kw['dX2'] * kw['dY2']


def open_cells(z):
    """finite cells on the border or beside a no-data cell"""
    nan = np.isnan(z)
    near = nan.copy()
    near[1:, :] |= nan[:-1, :]
    near[:-1, :] |= nan[1:, :]
    side = near.copy()
    side[:, 1:] |= near[:, :-1]
    side[:, :-1] |= near[:, 1:]
    side[0, :] = side[-1, :] = True
    side[:, 0] = side[:, -1] = True
    return side & ~nan


def int_sums(terms, shift, first):
    """exact int64 sums of rint(ldexp(term, shift)) over the runs that start at `first`"""
    return np.add.reduceat(np.rint(np.ldexp(terms, shift)).astype(np.int64), first)


def inventory(z, W, label, K, ra):
    """(label, table, quanta) of a tile from its classic fill W, its label raster (ids 1..K numbered by smallest linear index, 0, -1 on
    no data) and its row areas: every column of conditioning.DEPRESSION_DTYPE, formed directly from the planes"""
    from pydem_amd import conditioning as C
    n, m = z.shape
    NN = n * m
    flat = label.ravel()
    idx = np.flatnonzero(flat > 0)
    idx = idx[np.argsort(flat[idx], kind='stable')]                  # by id, ascending index within an id
    ids = flat[idx].astype(np.int64)
    r, c = idx // m, idx % m
    zc = z.ravel()[idx]
    depth = W.ravel()[idx] - zc
    amax = float(ra.max())
    sh_a, q_a = C.fixed_point(NN, amax)
    sh_v, q_v = C.fixed_point(NN, (float(depth.max()) if K else 0.0) * amax)
    if K == 0:
        return label, np.zeros(0, C.DEPRESSION_DTYPE), (q_a, q_v)
    first = np.flatnonzero(np.concatenate(([True], ids[1:] != ids[:-1])))
    assert len(first) == K and np.array_equal(ids[first], np.arange(1, K + 1))
    cells = np.diff(np.concatenate((first, [len(idx)])))
    zmin = np.minimum.reduceat(zc, first)
    bottom = np.minimum.reduceat(np.where(zc == np.repeat(zmin, cells), idx, NN), first)
    spill = np.maximum.reduceat(W.ravel()[idx], first)
    assert np.array_equal(spill, np.minimum.reduceat(W.ravel()[idx], first))        # one level per depression
    area = int_sums(ra[r], sh_a, first)
    volume = int_sums(depth * ra[r], sh_v, first)
    # sills: finite cells that are not raised, beside a cell of a depression whose level is their elevation
    cand = flat.reshape(n, m) == 0
    pairs = []
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            a = (slice(max(0, -dr), n - max(0, dr)), slice(max(0, -dc), m - max(0, dc)))       # the cell
            b = (slice(max(0, dr), n - max(0, -dr)), slice(max(0, dc), m - max(0, -dc)))       # its neighbour
            hit = cand[a] & (label[b] > 0)
            rr, cc = np.nonzero(hit)
            ra_, ca_ = rr + a[0].start, cc + a[1].start
            rb_, cb_ = rr + b[0].start, cc + b[1].start
            ok = W[rb_, cb_] == z[ra_, ca_]
            pairs.append((label[rb_, cb_][ok].astype(np.int64) - 1) * NN + (ra_[ok] * m + ca_[ok]))
    pairs = np.unique(np.concatenate(pairs))
    sid, scell = pairs // NN, pairs % NN
    sfirst = np.flatnonzero(np.concatenate(([True], sid[1:] != sid[:-1])))
    assert np.array_equal(sid[sfirst], np.arange(K))                 # every depression has a sill
    n_sills = np.diff(np.concatenate((sfirst, [len(sid)])))
    pour = scell[sfirst]
    open_sill = np.maximum.reduceat(open_cells(z).ravel()[scell].astype(np.int64), sfirst)
    table = C.depression_table(cells, np.minimum.reduceat(r, first), np.maximum.reduceat(r, first), np.minimum.reduceat(c, first),
                               np.maximum.reduceat(c, first), spill, bottom, z.ravel()[bottom], pour, n_sills, open_sill,
                               area.astype(np.float64) * q_a, volume.astype(np.float64) * q_v, m)
    return label, table, (q_a, q_v)


def filtered(inv, min_depth=0.0, min_cells=1):
    """the inventory with the depressions below min_depth or min_cells dropped and the rest renumbered in the same order"""
    label, table, quanta = inv
    keep = (table['max_depth'] >= min_depth) & (table['cells'] >= min_cells)
    lut = np.zeros(len(table) + 2, np.int32)
    lut[1:-1][keep] = np.arange(1, int(keep.sum()) + 1)
    lut[-1] = -1                                                     # (label -1 indexes the last word)
    return lut[label], table[keep], quanta


# ---- the mosaic ------------------------------------------------------------------------------------------------------------------
class Mosaic:
    """z (n, m) and placements [(name, row, col)]"""

    def __init__(self, n, m, names=None):
        names = cycle() if names is None else list(names)
        self.z = np.full((n, m), np.nan)
        self.placements = []
        k = 0
        r = 0
        while True:
            c = 0
            tall = 0
            skipped = 0
            while skipped < len(names):                 # a shelf: the cycle goes on until the next patch is too wide
                p = patch(names[k % len(names)])
                if r + p.shape[0] > n:
                    k += 1                              # too tall for what is left: the next one may fit
                    skipped += 1
                    continue
                if c + p.shape[1] > m:
                    break
                self.z[r:r + p.shape[0], c:c + p.shape[1]] = p
                self.placements.append((names[k % len(names)], r, c))
                tall = max(tall, p.shape[0])
                c += p.shape[1] + 1
                k += 1
                skipped = 0
            if tall == 0:
                break
            r += tall + 1
        self._W = {}
        self._labels = None
        self._inv = {}

    def epsilon(self, eps):
        from pydem_amd import conditioning
        return conditioning.fill_depressions_epsilon(self.z, eps)

    def fill(self, eps):
        """the composed W under eps (None: the automatic value of the WHOLE tile, passed to every patch fill)"""
        eps = self.epsilon(eps)
        if eps not in self._W:
            W = np.full(self.z.shape, np.nan)
            for name, r, c in self.placements:
                p = patch_fill(name, eps)
                W[r:r + p.shape[0], c:c + p.shape[1]] = p
            W.setflags(write=False)
            self._W[eps] = W
        return self._W[eps]

    def labels(self):
        """(label raster, K): the patches' labels renumbered in ascending order of each depression's first cell in the tile"""
        if self._labels is None:
            n, m = self.z.shape
            lab = np.where(np.isnan(self.z), -1, 0).astype(np.int32)
            firsts = []
            off = 0
            for name, r, c in self.placements:
                pl, k, pf = patch_labels(name)
                h, w = pl.shape
                sub = lab[r:r + h, c:c + w]
                sub[pl > 0] = pl[pl > 0] + off
                firsts.append((r + pf // w) * m + c + pf % w)
                off += k
            order = np.argsort(np.concatenate(firsts)) if off else np.zeros(0, np.int64)     # (first cells are distinct)
            lut = np.zeros(off + 2, np.int32)
            lut[1:-1][order] = np.arange(1, off + 1)
            lut[-1] = -1
            lab = lut[lab]
            lab.setflags(write=False)
            self._labels = lab, off
        return self._labels

    def inventory(self, ra):
        """(label, table, quanta) under the row areas `ra`, computed once per ra"""
        key = np.asarray(ra, np.float64).tobytes()
        if key not in self._inv:
            lab, K = self.labels()
            self._inv[key] = inventory(self.z, self.fill(0.0), lab, K, np.asarray(ra, np.float64))
        return self._inv[key]


_MOSAIC = {}


def mosaic(n, m):
    """the mosaic of the cycle on an (n, m) tile, built once per shape"""
    if (n, m) not in _MOSAIC:
        _MOSAIC[n, m] = Mosaic(n, m)
    return _MOSAIC[n, m]


# ---- the great lake --------------------------------------------------------------------------------------------------------------
class GreatLake:
    """z (n, m): fractal relief in [1, 1001) on the border ring, the same relief lowered by 2000 inside it, and the border cell
    (0, m // 3) at S = 0.5, the unique lowest cell of the ring; it touches the interior.  Every way from an interior cell to an open
    cell ends on the ring, whose lowest cell is S and beside the interior, and the whole interior lies below S: W = S there."""

    def __init__(self, n, m):
        from pydem_amd import synth
        z = synth.fractal(n, m, seed=5)
        z[1:-1, 1:-1] -= 2000.0
        self.sill = (0, m // 3)
        self.S = 0.5
        z[self.sill] = self.S
        ring = np.ones((n, m), bool)
        ring[1:-1, 1:-1] = False
        assert 0 < self.sill[1] < m - 1 and (z[ring] == self.S).sum() == 1 and z[ring].min() == self.S
        assert z[1:-1, 1:-1].max() < self.S
        z.setflags(write=False)
        self.z = z
        self.cells = (n - 2) * (m - 2)
        W = z.copy()
        W[1:-1, 1:-1] = self.S
        W.setflags(write=False)
        self.W = W
        label = np.zeros((n, m), np.int32)
        label[1:-1, 1:-1] = 1
        self.label = label
        self._inv = None

    def terms(self, ra):
        """(area terms, volume terms) of the interior cells in raster order"""
        m = self.z.shape[1]
        a = np.repeat(ra[1:-1], m - 2)
        return a, (self.S - self.z[1:-1, 1:-1]).ravel() * a

    def sums(self, ra):
        """(area sum, volume sum, quanta): the exact int64 sums and their quanta"""
        from pydem_amd import conditioning as C
        a, v = self.terms(ra)
        amax = float(ra.max())
        depth_max = self.S - float(self.z[1:-1, 1:-1].min())
        sh_a, q_a = C.fixed_point(self.z.size, amax)
        sh_v, q_v = C.fixed_point(self.z.size, depth_max * amax)
        first = np.zeros(1, np.int64)
        return int(int_sums(a, sh_a, first)[0]), int(int_sums(v, sh_v, first)[0]), (q_a, q_v)

    def inventory(self, ra):
        """(label, table, quanta) in closed form"""
        from pydem_amd import conditioning as C
        n, m = self.z.shape
        inner = self.z[1:-1, 1:-1]
        k = int(np.argmin(inner))                       # the first minimum in raster order
        bottom = (1 + k // (m - 2)) * m + 1 + k % (m - 2)
        sa, sv, (q_a, q_v) = self.sums(ra)
        table = C.depression_table([self.cells], [1], [n - 2], [1], [m - 2], [self.S], [bottom], [self.z.ravel()[bottom]],
                                   [self.sill[0] * m + self.sill[1]], [1], [1], [float(sa) * q_a], [float(sv) * q_v], m)
        return self.label, table, (q_a, q_v)


_LAKE = {}


def great_lake(n, m):
    if (n, m) not in _LAKE:
        _LAKE[n, m] = GreatLake(n, m)
    return _LAKE[n, m]
