"""Designed facets for the stencil (csrc/stencil.hip): small elevation fields made of independent 3 x 3 patches, each of which
hands ONE facet of its centre cell a chosen pair of slopes, and the values the reference must return there.  Plain numpy, no
device: tests/test_stencil_fields.py holds the kit (and the oracle) to its own claims, tests/test_gpu_stencil_bits.py holds
the kernels to it.

A patch for facet k with slopes (s1, s2) and that row's spacings (d1, d2):  z2 = 0,  z1 = z2 + s2 d2,  z0 = z1 + s1 d1 at the
centre, z1 / z2 at the facet's two neighbours (offsets E1 / E2 below, the reference's facet table), the other six neighbours
at the power of two above z0 + 4 |z0| + 8 max|s| max(d1, d2): no other facet of the centre descends further.  Patch centres sit at (1 + 3a, 1 + 3b):
no two patches share a cell.  Facets 0, 3, 4, 7 take (d1, d2) = (dX, dY), the others (dY, dX); facets 0-3 use spacing row
i - 1, facets 4-7 row i (_get_d1_d2).

What is expected of a designed cell is formed from the STORED elevations, the way the reference forms it: the slopes
(z0 - z1) / d1 and (z1 - z2) / d2 (the subtraction in float32 for a float32 field), the state of the facet from them
(_calc_direction I1-I3), the magnitude as separate numpy operations, the direction in np.longdouble.

Every field keeps a patch column per wavefront strip free (`spare_cols`): marked(field, value) puts a NaN or a huge elevation
into every row of it, which sends every band of every strip down the kernel's exact path and changes no designed cell.

Every designed slope lies within [2^-480, 2^480] and every square stays normal: slopes outside the window the kernel
documents are not this kit's business."""
import functools

import numpy as np

L = np.longdouble
E1R = np.array([0, -1, -1, 0, 0, 1, 1, 0]); E1C = np.array([1, 0, 0, -1, -1, 0, 0, 1])
E2R = np.array([-1, -1, -1, -1, 1, 1, 1, 1]); E2C = np.array([1, 1, -1, -1, -1, -1, 1, 1])
FAMILY_A = (0, 3, 4, 7)                        # d1, d2 = dX, dY; the others dY, dX
CARDINAL, DIAGONAL, INTERIOR, TIE = 1, 2, 3, 4
SCALES = (1.0, 0.3711, 2.0 ** -470, 2.0 ** 470)
STRIP = 62                                     # output columns of a wavefront of the marching kernel
PATCH_COLS = 38                                # 114 columns: two strips, the second one ragged


def cdiv(a, b):
    return -(-a // b)


def chunk_rows(n, m):
    """csrc/stencil.hip launch_stencil: rows per chunk halve from 128 while the tile gives fewer than 12288 wavefronts, down to 16"""
    rows = 128
    while rows > 16 and cdiv(m - 2, STRIP) * cdiv(n - 2, rows) < 12288:
        rows >>= 1
    return rows


def strip_columns(m):
    """[first, one past the last] column the lanes of each strip read"""
    return [(STRIP * s, min(STRIP * s + 64, m)) for s in range(cdiv(m - 2, STRIP))]


class Field(object):
    """z (float64 or float32), dX, dY (n - 1), the designed cells i, j, k, the centre columns of the spare patch columns, what
    marked() put there"""

    def __init__(self, name, z, dX, dY, i, j, k, spare_cols=(), marker=None):
        self.name, self.z, self.dX, self.dY = name, z, np.asarray(dX, np.float64), np.asarray(dY, np.float64)
        self.i, self.j, self.k = (np.asarray(x, np.int64) for x in (i, j, k))
        self.spare_cols, self.marker = tuple(spare_cols), marker
        self.shape = z.shape

    @property
    def spacing(self):
        return dict(dX=self.dX, dY=self.dY)

    @functools.lru_cache(maxsize=None)
    def expected(self):
        return expected(self.z, self.dX, self.dY, self.i, self.j, self.k)


def expected(z, dX, dY, i, j, k):
    """What the reference computes at the cells (i, j) if facet k decides them, from the stored elevations:
    s1, s2, sd (subtraction in z's dtype), s1_f64, s2_f64 (subtraction in float64), d1, d2, kind, mag (float64),
    r, direction, theta (longdouble; theta = the table angle of the winner), a0, a1 and k_win: the facet that wins (k, or the
    one across the diagonal -- see below)"""
    n = z.shape[0]
    row = np.where(k < 4, i - 1, i)
    assert row.min() >= 0 and row.max() <= n - 2
    fam_a = np.isin(k, FAMILY_A)
    d1 = np.where(fam_a, dX[row], dY[row]); d2 = np.where(fam_a, dY[row], dX[row])
    z0, z1, z2 = z[i, j], z[i + E1R[k], j + E1C[k]], z[i + E2R[k], j + E2C[k]]
    hyp = np.sqrt(d1 * d1 + d2 * d2)
    s1 = (z0 - z1).astype(np.float64) / d1                      # (a float32 field subtracts in float32, the division promotes)
    s2 = (z1 - z2).astype(np.float64) / d2
    sd = (z0 - z2).astype(np.float64) / hyp
    z64 = [np.asarray(x, np.float64) for x in (z0, z1, z2)]
    both = (s1 > 0) & (s2 > 0)
    cross_a, cross_b = s2 * d1, s1 * d2
    kind = np.full(k.shape, INTERIOR)
    kind[both & (cross_a == cross_b)] = TIE
    kind[((s1 <= 0) & (s2 > 0)) | (both & (cross_a > cross_b))] = DIAGONAL
    kind[(s1 > 0) & (s2 <= 0)] = CARDINAL
    assert not ((s1 <= 0) & ((s2 <= 0) | (sd <= 0))).any(), "a designed facet does not descend"
    inner = (kind == INTERIOR) | (kind == TIE)
    rad2 = s1 * s1 + s2 * s2
    # the facet across the shared diagonal (k ^ 1: same spacing row, same sd, its first neighbour a filler above z0) is in the
    # diagonal state with sd^2: next to the diagonal that can reach the interior s1^2 + s2^2 after rounding, and the
    # reference's strict `>` then hands the cell to whichever of the two comes first
    kp = k ^ 1
    cand = np.where(kind == CARDINAL, s1 * s1, np.where(kind == DIAGONAL, sd * sd, rad2))
    partner = (sd > 0) & np.where(kp < k, sd * sd >= cand, sd * sd > cand)      # (a diagonal winner with kp < k: the same sd^2, the first one keeps it)
    kind[partner] = DIAGONAL
    k_win = np.where(partner, kp, k)
    mag = np.where(kind == CARDINAL, np.sqrt(s1 * s1), np.where(kind == DIAGONAL, np.sqrt(sd * sd), np.sqrt(rad2)))
    theta = np.arctan2(d2.astype(L), d1.astype(L))
    theta_win = np.where(partner, np.arctan2(d1.astype(L), d2.astype(L)), theta)
    inner = inner & ~partner
    with np.errstate(invalid='ignore'):
        r = np.where(inner, np.arctan2(s2.astype(L), s1.astype(L)), np.where(kind == DIAGONAL, theta_win, L(0)))
    a0 = (k_win + 1) >> 1
    a1 = np.where(k_win & 1, -1.0, 1.0)
    direction = r * a1.astype(L) + (a0.astype(np.float64) * np.pi / 2).astype(L)
    theta = theta_win
    return dict(s1=s1, s2=s2, sd=sd, s1_f64=(z64[0] - z64[1]) / d1, s2_f64=(z64[1] - z64[2]) / d2, d1=d1, d2=d2, kind=kind,
                mag=mag, r=r, direction=direction, theta=theta, a0=a0, a1=a1, k_win=k_win)


def table_index(s1, s2):
    """(kf, swap) of the kernel's arctangent for slopes s1, s2 > 0: the table entry nearest to 16 min / max, and whether the
    arguments change places.  (The kernel picks kf with a raw reciprocal: within a few spacings of (k + 1/2) / 16 it may
    take the other entry, which is what the designed ratios there are for.)"""
    num, den = np.minimum(s1, s2), np.maximum(s1, s2)
    return np.rint(16.0 * (num / den)).astype(int), s2 > s1


# ---------------------------------------------------------------------------------------------------------------------------
# ratios
def base_ratios():
    """s2 / s1 in (0, 1): (k + h) / 16 for k = 1 .. 15, h in {0, 1/2}, and -2 .. 2 spacings around each -- where the table
    index switches (h = 1/2: the reduced argument is largest there) and where it is zero; 1 - j spacings for j = 1 .. 3;
    2^-1, 2^-4 .. 2^-25"""
    qs = []
    for k in range(1, 16):
        for h in (0.0, 0.5):
            q = (k + h) / 16
            qs += [q + t * np.spacing(q) for t in (-2, -1, 0, 1, 2)]
    qs += [1.0 - j * 2.0 ** -53 for j in (1, 2, 3)]
    qs += [2.0 ** -e for e in range(1, 26, 3)]
    return sorted(set(qs))


def pair_ratios(d1, d2):
    """s2 / s1 for a facet with spacings (d1, d2), all with s2 d1 < s1 d2 by a margin (interior): the base ratios scaled by
    d2 / d1 (the whole sector), the base ratios themselves and their reciprocals (the switches of the table index without and
    with `swap`), as far as they lie below 31/32 of d2 / d1.  Pairs (ratio, what it is the reciprocal of or None)."""
    t = d2 / d1
    base = base_ratios()
    qs = [(q * t, None) for q in base] + [(q, None) for q in base] + [(1.0 / q, q) for q in base]
    return sorted(set(q for q in qs if q[0] <= t * 0.96875 and q[0] >= 2.0 ** -26))


# ---------------------------------------------------------------------------------------------------------------------------
# the assembly
def _spares(m):
    """centre columns of the spare patch columns: one inside the lanes of each strip"""
    out = []
    for lo, hi in strip_columns(m):
        b = min((lo + 30) // 3, (m - 3) // 3 - 1)
        assert lo + 2 <= 1 + 3 * b <= hi - 3
        out.append(1 + 3 * b)
    return out


def _tuned_drops(s1, q, d1, d2, inverse=None):
    """(z0 - z1, z1 - z2) for slopes s1 and q s1: of the elevations z1 within 4 spacings of q s1 d2 and z0 within 2 spacings of
    z1 + s1 d1, the pair whose REALISED ratio ((z1 - 0) / d2) / ((z0 - z1) / d1) comes nearest to q -- the roundings on the way
    move the ratio by a spacing or two, and the ratios next to a switch of the table index are meant to be where they say.
    `inverse`: the ratio was formed as 1 / inverse and it is s1 / s2 that is meant to sit at `inverse` (the `swap` branch)."""
    def around(x, steps):
        c = [np.float64(x)]
        for _ in range(steps):
            c = [np.nextafter(c[0], -np.inf)] + c + [np.nextafter(c[-1], np.inf)]
        return np.array(c)
    want = L(q) if inverse is None else L(inverse)
    for steps in (4, 32, 256):                  # (where z1 is large against the drop to it, z0 - z1 moves in coarse steps: look further)
        z1 = around(q * s1 * d2, steps)[:, None]
        z0 = np.concatenate([around(c + s1 * d1, 2) for c in z1[:, 0]]).reshape(-1, 5)
        s2r, s1r = (z1 / d2).astype(L), ((z0 - z1) / d1).astype(L)             # the slopes as the reference forms them
        miss = np.abs((s2r / s1r if inverse is None else s1r / s2r) - want)
        a, b = np.unravel_index(np.argmin(miss), miss.shape)
        if miss[a, b] <= np.spacing(np.float64(want)) / 2:
            break
    return float(z0[a, b] - z1[a, 0]), float(z1[a, 0])


def _filler(f):
    """the power of two at or above f: two fillers are equal or a factor of two apart, so that no filler cell sees a slope of a
    few spacings of its elevation (at scale 2^-470 the square of such a slope is subnormal: outside the kernel's window)"""
    m, e = np.frexp(f)
    return float(np.ldexp(1.0, e if m != 0.5 else e - 1))


def _assemble(name, groups, spacing_of, dtype=np.float64, patch_cols=PATCH_COLS):
    """groups: lists of patch specs, each group starts a patch row; spacing_of(n, rows of each group) -> dX, dY.
    A spec is (k, 'slopes', s1, s2) or (k, 'ratio', s1, s2 / s1, inverse or None) or (k, 'drops', z0 - z1, z1 - z2) or (k, 'cardinal', z0 - z1) -- the last one moves to the
    facet across the same edge if that one's spacing row gives the larger slope (it would win)."""
    m = 3 * patch_cols
    spare = _spares(m)
    free = [b for b in range(patch_cols) if 1 + 3 * b not in spare]
    slots, group_rows, a = [], [], 0
    for g in groups:
        rows = cdiv(len(g), len(free))
        group_rows.append((3 * a, 3 * (a + rows)))
        for q, spec in enumerate(g):
            slots.append((a + q // len(free), free[q % len(free)], spec))
        a += rows
    n = 3 * a
    dX, dY = spacing_of(n, group_rows)
    z = np.zeros((n, m))
    filled = np.zeros((n, m), bool)
    ci, cj, ck, fill = [], [], [], []
    mate = {0: 7, 7: 0, 3: 4, 4: 3}
    for pa, pb, spec in slots:
        i, j, k = 1 + 3 * pa, 1 + 3 * pb, spec[0]

        def dd(k):
            r = i - 1 if k < 4 else i
            return (dX[r], dY[r]) if k in FAMILY_A else (dY[r], dX[r])
        if spec[1] == 'cardinal':
            if k in mate and (dd(mate[k])[0], mate[k]) < (dd(k)[0], k):
                k = mate[k]
            elif k in (2, 6):
                k -= 1                                       # (facets 1 / 5 come first across the same edge, same spacing row)
            drop1, drop2 = spec[2], 0.0
        d1, d2 = dd(k)
        if spec[1] == 'slopes':
            drop1, drop2 = spec[2] * d1, spec[3] * d2
        elif spec[1] == 'ratio':
            drop1, drop2 = _tuned_drops(spec[2], spec[3], d1, d2, spec[4])
        elif spec[1] == 'drops':
            drop1, drop2 = spec[2], spec[3]
        z2 = 0.0; z1 = z2 + drop2; z0 = z1 + drop1
        f = _filler(z0 + 4 * abs(z0) + 8 * max(abs(drop1 / d1), abs(drop2 / d2)) * max(d1, d2))
        z[i - 1:i + 2, j - 1:j + 2] = f
        z[i, j] = z0; z[i + E1R[k], j + E1C[k]] = z1; z[i + E2R[k], j + E2C[k]] = z2
        filled[i - 1:i + 2, j - 1:j + 2] = True
        ci.append(i); cj.append(j); ck.append(k); fill.append(f)
    z[~filled] = max(fill)
    z = z.astype(dtype)
    assert np.isfinite(z).all()
    return Field(name, z, dX, dY, ci, cj, ck, spare)


def _uniform(dx, dy):
    return lambda n, group_rows: (np.full(n - 1, float(dx)), np.full(n - 1, float(dy)))


def _per_group(pairs):
    def f(n, group_rows):
        dX, dY = np.ones(n - 1), np.ones(n - 1)
        for (lo, hi), (dx, dy) in zip(group_rows, pairs):
            dX[lo:hi] = dx; dY[lo:hi] = dy
        return dX, dY
    return f


@functools.lru_cache(maxsize=None)
def ratio_field(scale, dtype='float64'):
    """unit spacing (exact quotients: the arctangent alone), s1 = scale, s2 = q scale, every base ratio on all 8 facets"""
    qs = [q for q in base_ratios() if q * scale >= 2.0 ** -479]
    specs = [(k, 'ratio', scale, q, None) for q in qs for k in range(8)]
    return _assemble('ratio %g %s' % (scale, dtype), [specs], _uniform(1, 1), np.dtype(dtype))


SWAP_PAIRS = ((1, 17), (17, 1), (20, 30), (1, 40))       # (dX, dY).  (1, 40): the only one whose sector reaches table entry 0 with `swap`


@functools.lru_cache(maxsize=None)
def swapped_field(dtype='float64'):
    """dX != dY: theta > pi / 4 for one family of facets, so s2 > s1 is interior -- the `swap` branch of the arctangent"""
    groups = []
    for dx, dy in SWAP_PAIRS:
        specs = []
        for fam, (d1, d2) in (((0, 3, 4, 7), (dx, dy)), ((1, 2, 5, 6), (dy, dx))):
            for idx, (q, inverse) in enumerate(pair_ratios(float(d1), float(d2))):
                s1 = (1.0, 0.3711)[idx & 1] if q <= 1 else (1.0, 0.3711)[idx & 1] / q      # (the larger slope is the scale)
                specs.append((fam[idx % 4], 'ratio', s1, q, inverse))
        groups.append(specs)
    return _assemble('swapped ' + dtype, groups, _per_group(SWAP_PAIRS), np.dtype(dtype))


TIE_PAIRS = ((1, 17), (30, 20), (3, 7), (1, 1))
TIE_FACTORS = tuple(c * 2.0 ** e for c, e in ((1, 0), (1, -3), (1, 7), (3, 0), (3, -11), (5, 2), (7, -6), (11, 4), (13, -20), (1, -460),
                                               (3, -462), (1, 455), (5, 452), (25, -5), (1, 30), (9, -33)))


@functools.lru_cache(maxsize=None)
def tie_field():
    """slopes in the exact ratio of the spacings, s1 = c d1, s2 = c d2 with c a small integer times a power of two: every
    elevation, slope and cross product is exact, s2 d1 == s1 d2, the reference's arctangent is the table angle"""
    groups = []
    for dx, dy in TIE_PAIRS:
        specs = []
        for c in TIE_FACTORS:
            for k in range(8):
                d1, d2 = (dx, dy) if k in FAMILY_A else (dy, dx)
                specs.append((k, 'slopes', c * d1, c * d2))
        groups.append(specs)
    return _assemble('tie', groups, _per_group(TIE_PAIRS))


AWKWARD = (1 + 2.0 ** -52, 2 - 2.0 ** -52, 3.0, 1 / 3.0, 0.1, 92.66254330558)


def _awkward_spacing(n, group_rows):
    """spacings whose reciprocals round badly, another one in every row (cycles of 7 and 8 rows against patch rows of 3)"""
    r = np.arange(n - 1, dtype=np.float64)
    cx = AWKWARD + (None,)
    cy = AWKWARD[3:] + AWKWARD[:3] + (None, None)
    dX = np.array([cx[q % 7] if cx[q % 7] is not None else 25 + 0.01 * q for q in range(n - 1)])
    dY = np.array([cy[q % 8] if cy[q % 8] is not None else (31 - 0.004 * q if q % 8 == 6 else 25 + 0.01 * q) for q in range(n - 1)])
    return dX, dY


@functools.lru_cache(maxsize=None)
def quotient_field(dtype='float64'):
    """cardinal winners (s2 <= 0: mag = |s1|, a quotient by dX or dY) and diagonal winners (mag = |sd|, a quotient by the
    hypotenuse; both ways into that state: s1 <= 0 < s2, and s2 d1 > s1 d2), numerators random over 40 binades and small
    integers, spacings of _awkward_spacing"""
    rng = np.random.default_rng(20240)
    count = 36 * 36
    nums = np.ldexp(rng.uniform(1.0, 2.0, count), rng.integers(-20, 20, count))
    nums[::3] = rng.integers(1, 4000, nums[::3].size)
    if dtype == 'float32':
        nums = nums.astype(np.float32).astype(np.float64)
    specs = []
    for q, a in enumerate(nums):
        k, how = q % 8, (q // 8) % 4
        if how == 0:
            specs.append((k, 'cardinal', a))
        elif how == 1:
            specs.append((k, 'drops', a * 0.875, -a * 0.125) if k in (1, 5) else (k, 'cardinal', a))     # s2 < 0 where no other spacing row competes
        elif how == 2:
            specs.append((k, 'drops', 0.0, a))                                 # s1 == 0 < s2: diagonal
        else:
            specs.append((k, 'drops', a * 2.0 ** -20, a * (1 - 2.0 ** -20)))   # s2 d1 > s1 d2: diagonal
    return _assemble('quotient ' + dtype, [specs], _awkward_spacing, np.dtype(dtype))


def marked(field, value):
    """the field with `value` (NaN, a huge elevation) in every row of every spare patch column: at least two columns from the
    cells of any patch, so no designed cell and none of its neighbours changes"""
    z = field.z.copy()
    for c in field.spare_cols:
        z[:, c] = value
    return Field('%s marked %s' % (field.name, 'NaN' if np.isnan(value) else '2^%d' % round(np.log2(value))), z, field.dX, field.dY,
                 field.i, field.j, field.k, field.spare_cols, value)


# ---------------------------------------------------------------------------------------------------------------------------
# perimeter patches: the same design for cells of the first / last row and column (k_stencil_perimeter: `/`, sqrt, atan2_pos)
EDGE_FACETS = dict(top=(5, 6), bottom=(1, 2), left=(0, 7), right=(3, 4))
CORNER_FACETS = ((6, 7), (4, 5), (0, 1), (2, 3))       # top left, top right, bottom left, bottom right


@functools.lru_cache(maxsize=None)
def perimeter_field(dx, dy, dtype='float64', side=66):
    """A plateau (flat: mag = -1 throughout the interior) whose border cells carry designed facets.  The facet of an edge
    cell is one whose first neighbour z1 is the interior neighbour the copy rule looks at: that cell then drains ALONG the edge
    to z2 (direction exactly 0, pi/2, pi or 3 pi/2: outside the rule's open interval) -- or is a flat, for a corner, whose
    diagonal neighbour is z2 -- so the copy rule brings nothing and the designed facet decides the cell."""
    n = m = 3 * side
    dX, dY = np.full(n - 1, float(dx)), np.full(n - 1, float(dy))
    cells = [('top', 0, 1 + 3 * b) for b in range(1, side - 1)] + [('bottom', n - 1, 1 + 3 * b) for b in range(1, side - 1)]
    cells += [('left', 1 + 3 * a, 0) for a in range(1, side - 1)] + [('right', 1 + 3 * a, m - 1) for a in range(1, side - 1)]
    ratios = {}
    for fam in (True, False):
        d1, d2 = (dx, dy) if fam else (dy, dx)
        qs = [q for q, _ in pair_ratios(float(d1), float(d2))]
        ratios[fam] = qs[::max(1, cdiv(2 * len(qs), len(cells)))]
    patches, used = [], {True: 0, False: 0}
    for idx, (edge, i, j) in enumerate(cells):
        k = EDGE_FACETS[edge][(idx // 2) & 1]
        fam = k in FAMILY_A
        q = ratios[fam][used[fam] % len(ratios[fam])]; used[fam] += 1
        patches.append((i, j, k, q))
    for c, (i, j) in enumerate(((0, 0), (0, m - 1), (n - 1, 0), (n - 1, m - 1))):
        k = CORNER_FACETS[c][(c + int(dx > dy)) & 1]
        t = dy / dx if k in FAMILY_A else dx / dy
        patches.append((i, j, k, (0.3, 0.77, 0.52, 0.91)[c] * t))
    z = np.zeros((n, m))
    ci, cj, ck, fill = [], [], [], []
    for idx, (i, j, k, q) in enumerate(patches):
        d1, d2 = (dx, dy) if k in FAMILY_A else (dy, dx)
        s1 = (1.0, 0.3711)[idx & 1] if q <= 1 else (1.0, 0.3711)[idx & 1] / q
        z2 = 0.0; z1 = z2 + s1 * q * d2; z0 = z1 + s1 * d1
        z[i, j] = z0; z[i + E1R[k], j + E1C[k]] = z1; z[i + E2R[k], j + E2C[k]] = z2
        ci.append(i); cj.append(j); ck.append(k); fill.append(_filler(z0 + 4 * abs(z0) + 8 * max(s1, s1 * q) * max(d1, d2)))
    designed = np.zeros((n, m), bool)
    for i, j, k in zip(ci, cj, ck):
        designed[i, j] = designed[i + E1R[k], j + E1C[k]] = designed[i + E2R[k], j + E2C[k]] = True
    z[~designed] = max(fill)
    return Field('perimeter %g x %g %s' % (dx, dy, dtype), z.astype(np.dtype(dtype)), dX, dY, ci, cj, ck)


PERIMETER_PAIRS = ((1, 1), (20, 30), (30, 20))


def float64_fields():
    """every float64 field of the kit, perimeter fields last"""
    return [ratio_field(s) for s in SCALES] + [swapped_field(), tie_field(), quotient_field()] + [perimeter_field(*p) for p in PERIMETER_PAIRS]


F32_SCALES = (1.0, 0.3711, 2.0 ** 40, 2.0 ** -40)


def float32_fields():
    """the ratio and quotient designs (and the perimeter's) with every elevation a float32 value"""
    return [ratio_field(s, 'float32') for s in F32_SCALES] + [quotient_field('float32')] + [perimeter_field(*p, dtype='float32') for p in PERIMETER_PAIRS]
