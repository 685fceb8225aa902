"""Designed inputs for the graph stage and the wetness index (csrc/uca.hip: k_section_proportion with keep_edge of
csrc/uca_graph.h, k_graph_inmask, k_corner_todo, k_twi): direction planes that are SET, not computed, so that the device and the
oracle see the same bits and every comparison between them is exact.  Plain numpy, no device: tests/test_graph_fields.py holds
the kit (and the oracle) to its own claims, tests/test_gpu_graph_bits.py holds the kernels to the oracle on it.

Directions.  Row i has its own theta_i = atan2(dY[r], dX[r]), r = clamp(i - 1, 0, n - 3) (reference :1031-1033).  Quadrant q
(sec0 = q) splits at t1 = theta (q even) or pi/2 - theta (q odd) into sections 2q and 2q + 1; the first is t1 wide, the second
t2 = pi/2 - t1.  The designed values of a row sit at the nine boundaries q pi/2 (q = 0..4) and q pi/2 + t1 (q = 0..3): the value
itself, 1 and 2 nextafter steps either side, and offsets of 1e-9, 0.5e-8, 2e-8, 0.0099 and 0.0101 of the width of the section they
fall into -- proportion or 1 - proportion on both sides of the keep-filter's 1e-8 and of the inlet rule's 1e-2.  Plus 0, 2 pi,
nextafter(2 pi, 0) and NaN (a NaN direction on a cell that is not flat: both implementations convert it to sec0 = 0 and carry a NaN
proportion, which the keep-filter drops).  Negative directions are out of contract (the stencil's range is [0, 2 pi], flats carry
-1 under the flats mask) and are left out; everything else is seeded uniform.

Elevations.  No cell ties with a target except where designed, and a kept edge never climbs (z_to <= z_from), so every field is
acyclic whatever its directions are.  The surface is a patchwork of four tilts, descending towards the middle of quadrant 0, 1, 2
and 3: every designed value meets, in some row, a patch where both of its targets are lower.  On top of it: cells whose two targets
are, in turn, lower / higher / equal / NaN (keep_cases), inlet cells on each side whose only kept out-edge weighs 0.0099 or 0.0101
(inlets), one whose only kept out-edge weighs exactly 1e-2 (exact_tol), the six corner cases of :920-930 and an in-sum and an
out-sum of 0.0099 and 0.0101 at a corner (CORNER_CASES; equality with the corner rule's 1e-2 is not reached), flats.

TWI.  (uca, mag, options) cases whose quotient uca / (mag + min_slope) is chosen: see twi_cases()."""
import functools
import math

import numpy as np

L = np.longdouble
H = np.pi / 2
E1R = np.array([0, -1, -1, 0, 0, 1, 1, 0]); E1C = np.array([1, 0, 0, -1, -1, 0, 0, 1])          # the reference's facet table: first (cardinal)
E2R = np.array([-1, -1, -1, -1, 1, 1, 1, 1]); E2C = np.array([1, 1, -1, -1, -1, -1, 1, 1])      # and second (diagonal) neighbour
RELS = (1e-9, 0.5e-8, 2e-8, 0.0099, 0.0101)
STEPS = (-2, -1, 1, 2)
TOL = 1e-2
SIDE_SECTIONS = dict(left=(6, 7, 0, 1), right=(2, 3, 4, 5), top=(4, 5, 6, 7), bottom=(0, 1, 2, 3))           # :913-919
CORNER_CASES = ('side_rule', 'outsum_alone', 'insum_zero', 'insum_small', 'insum_large_no_out', 'nan_elevation',
                'insum_below', 'insum_above', 'outsum_below', 'outsum_above')       # the last four: 0.0099 / 0.0101 either side of the corner rule's 1e-2
CORNER_TODO = dict(side_rule=True, outsum_alone=True, insum_zero=True, insum_small=True, insum_large_no_out=False, nan_elevation=False,
                   insum_below=True, insum_above=False, outsum_below=False, outsum_above=True)


def theta_rows(dX, dY, n):
    """theta of every row (libm's atan2 through math: what the oracle and the library's host code call)"""
    r = np.clip(np.arange(n) - 1, 0, n - 3)
    return np.array([math.atan2(dY[k], dX[k]) for k in r])


def _steps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def designed_values(theta):
    """[(value, label)] of one row; label = (kind, q, class): kind 'quadrant' (boundary q pi/2) or 'inner' (q pi/2 + t1), class
    'exact', 'step%+d', '%+g' (an offset in widths of the section the value falls into); or ('special', 0, name)"""
    out = []
    for kind, qs in (('quadrant', range(5)), ('inner', range(4))):
        for q in qs:
            t1 = theta if q % 2 == 0 else H - theta
            if kind == 'quadrant':
                B, below, above = H * q, t1, t1             # (the second section of quadrant q - 1 is as wide as the first of q)
            else:
                B, below, above = H * q + t1, t1, H - t1
            out.append((B, (kind, q, 'exact')))
            out += [(_steps(B, k), (kind, q, 'step%+d' % k)) for k in STEPS]
            out += [(B - r * below, (kind, q, '%+g' % -r)) for r in RELS] + [(B + r * above, (kind, q, '%+g' % r)) for r in RELS]
    out = [(v, lab) for v, lab in out if 0.0 <= v <= 2 * np.pi]
    out += [(0.0, ('special', 0, 'zero')), (2 * np.pi, ('special', 0, 'two_pi')),
            (np.nextafter(2 * np.pi, 0), ('special', 0, 'below_two_pi')), (np.nan, ('special', 0, 'nan'))]
    return out


def expected_labels():
    """every label a row can carry: all but the values below 0 and above 2 pi"""
    return sorted(set(lab for _, lab in designed_values(0.7)))


class Field(object):
    """z, direction, mag (float64), flats (uint8), spacing; label[i][j]: the designed value a cell carries or None; notes: what
    the builders placed, by name -> list of cells"""

    def __init__(self, name, n, m, dX, dY, dX2, dY2, seed, drain_pits=False):
        self.name, self.shape, self.drain_pits = name, (n, m), drain_pits
        self.dX, self.dY, self.dX2, self.dY2 = (np.asarray(x, np.float64) for x in (dX, dY, dX2, dY2))
        self.seed = seed
        self.notes = {}
        self.exact_tol_cell = None

    def build(self):
        n, m = self.shape
        rng = np.random.default_rng(self.seed)
        self.theta = theta_rows(self.dX, self.dY, n)
        self.direction = rng.uniform(0.0, 2 * np.pi, (n, m))
        self.label = [[None] * m for _ in range(n)]
        for i in range(n):
            vals = designed_values(self.theta[i])
            K = len(vals)
            if m >= K:
                cells = [((k + 7 * i) % m, vals[k]) for k in range(K)]
            else:
                cells = [(j, vals[(i * m + j) % K]) for j in range(m)]
            for j, (v, lab) in cells:
                self.direction[i, j] = v
                self.label[i][j] = lab
        self.z = _surface(n, m)
        self.mag = np.ones((n, m))
        self.flats = np.zeros((n, m), np.uint8)
        return self

    def seal(self):
        for a in (self.z, self.direction, self.mag, self.flats):
            a.setflags(write=False)
        return self

    @property
    def spacing(self):
        return dict(dX=self.dX, dY=self.dY, dX2=self.dX2, dY2=self.dY2)

    def labels(self):
        return set(lab for row in self.label for lab in row if lab is not None)

    def set_direction(self, i, j, v, note=None):
        self.direction[i, j] = v
        self.label[i][j] = None
        if note:
            self.notes.setdefault(note, []).append((i, j))

    def t1(self, i, q):
        return self.theta[i] if q % 2 == 0 else H - self.theta[i]


def _surface(n, m):
    """four tilts: patch b descends along the direction b pi/2 + pi/4 + 0.1 (3 per cell), plus a ripple that breaks ties"""
    i, j = np.mgrid[0:n, 0:m].astype(np.float64)
    band = ((i // max(1, -(-n // 4))) + (j // 25)).astype(np.int64) % 4
    phi = band * H + np.pi / 4 + 0.1
    return 5000.0 - 3.0 * (np.cos(phi) * j - np.sin(phi) * i) + 0.05 * np.sin(1.3 * i + 0.7 * j + 0.11 * i * j)


# ---------------------------------------------------------------------------------------------------------------------------
# what the builders put on top of the base field
def _keep_cases(F, cells, nan_cell):
    """interior cells that hand half of their flow to each target (the middle of an even section), the targets in turn lower,
    higher, equal and NaN; an equal target carries the same direction (it points away: no loop)"""
    outcomes = [(a, b) for a in ('lower', 'higher', 'equal', 'nan') for b in ('lower', 'higher', 'equal', 'nan')]
    n, m = F.shape
    for k, (i, j) in enumerate(cells):
        assert 1 <= i < n - 1 and 1 <= j < m - 1
        q = k % 4
        d = H * q + F.t1(i, q) / 2
        F.set_direction(i, j, d, 'keep')
        F.z[i, j] = z0 = 5000.0 + k
        for (dr, dc), how in zip(((E1R[2 * q], E1C[2 * q]), (E2R[2 * q], E2C[2 * q])), outcomes[k % len(outcomes)]):
            t = (i + dr, j + dc)
            F.z[t] = dict(lower=z0 - 7.0, higher=z0 + 7.0, equal=z0, nan=np.nan)[how]
            if how == 'equal':
                F.set_direction(t[0], t[1], d)
    F.z[nan_cell] = np.nan                          # ... and a cell that is NaN itself


def _inlets(F, side, cells):
    """non-corner cells of one side, section an inlet section of that side, ONE kept out-edge of weight 0.0099 / 0.0101: the small
    share goes to the diagonal (d just above the quadrant boundary) or to the cardinal target (d just below the inner boundary),
    the other target is raised"""
    q = dict(left=0, right=2, top=3, bottom=1)[side]            # an even section 2q of that side's inlet sections with both targets inside
    sec = 2 * q
    assert sec in SIDE_SECTIONS[side]
    k = 0
    for rel in (0.0099, 0.0101):
        for small in ('diagonal', 'cardinal'):
            i, j = cells[k]; k += 1
            t1 = F.t1(i, q)
            d = H * q + rel * t1 if small == 'diagonal' else H * q + (1 - rel) * t1
            F.set_direction(i, j, d, 'inlet_' + side)
            F.z[i, j] = z0 = 5100.0 + k
            c, g = (i + E1R[sec], j + E1C[sec]), (i + E2R[sec], j + E2C[sec])
            F.z[c] = z0 + 7.0 if small == 'diagonal' else z0 - 7.0
            F.z[g] = z0 - 7.0 if small == 'diagonal' else z0 + 7.0


def _corner(F, corner, case):
    """one of CORNER_CASES at the corner 'tl', 'tr', 'bl', 'br'"""
    n, m = F.shape
    top, left = corner[0] == 't', corner[1] == 'l'
    ci, cj = (0 if top else n - 1), (0 if left else m - 1)
    ri, rj = (1 if top else -1), (1 if left else -1)
    V, Hn, D = (ci + ri, cj), (ci, cj + rj), (ci + ri, cj + rj)
    z0 = 5200.0
    F.z[ci, cj] = z0
    towards_v = 3 * H if top else H                 # the corner drains into V: section 6 / 2, the whole flow on the cardinal target
    away = np.pi if left else 0.0                   # both targets outside the tile
    inward_h = {'tl': 0.0, 'tr': np.nextafter(np.pi, 0), 'bl': np.nextafter(2 * np.pi, 0), 'br': np.pi}[corner]     # a section that is no inlet section of the row
    v_to_corner = H if top else 3 * H               # V drains into the corner: section 2 / 6, the whole flow on the cardinal target
    F.notes.setdefault('corner_' + case, []).append((ci, cj))
    if case == 'side_rule':
        F.set_direction(ci, cj, towards_v)
        F.z[V] = z0 - 7.0
    elif case in ('outsum_alone', 'outsum_below', 'outsum_above'):
        if case != 'outsum_alone':
            # the whole out-sum is ONE share of 0.0099 / 0.0101 on Hn (the diagonal target is outside), the section no inlet section of the bottom row
            rel = 0.0099 if case == 'outsum_below' else 0.0101
            theta = F.theta[ci]
            inward_h = {'bl': 3 * H + (H - theta) + rel * theta,             # section 7: proportion = (quadrant - (pi/2 - theta)) / theta, on E
                        'br': 2 * H + (1 - rel) * theta}[corner]             # section 4: proportion = 1 - quadrant / theta, on W
        F.set_direction(ci, cj, inward_h)
        F.z[Hn] = z0 - 7.0
        F.set_direction(V[0], V[1], v_to_corner)
        F.z[V] = z0 + 7.0
        F.z[D] = z0 - 9.0
    else:
        F.set_direction(ci, cj, away)
        F.z[Hn] = z0 - 7.0; F.z[D] = z0 - 9.0       # neither can drain uphill into the corner
        if case in ('insum_zero', 'nan_elevation'):
            F.z[V] = z0 - 8.0
            if case == 'nan_elevation':
                F.z[ci, cj] = np.nan
        else:
            w = dict(insum_small=0.005, insum_below=0.0099, insum_above=0.0101, insum_large_no_out=1.0)[case]
            qv = 1 if top else 3
            F.set_direction(V[0], V[1], H * qv + (1 - w) * F.t1(V[0], qv))        # section 2 qv: proportion = 1 - quadrant / t1 = w on the cardinal target
            F.z[V] = z0 + 7.0                         # (its other share goes to Hn, below the corner, or out of the tile)


def _flat(F, cells):
    for i, j in cells:
        F.flats[i, j] = 1; F.mag[i, j] = -1.0
        F.set_direction(i, j, -1.0, 'flat')


def _exact_tol(F, i):
    """left-side cell (i, 0) whose only kept out-edge weighs exactly 1e-2: section 1 (proportion = (quadrant - theta) / (pi/2 - theta),
    the share of the cardinal target N), on a row whose theta is tiny, so that the steps of d are finer than those of the share.
    Sets the spacing of row i - 1; the search is over a few dY and the neighbours of theta + 0.01 (pi/2 - theta)."""
    r = min(max(i - 1, 0), F.shape[0] - 3)
    for dy in (1.0, 1.1, 1.3, 1.7, 1.9, 2.3, 2.9, 3.1):
        theta = math.atan2(dy, 1000.0)
        cth = H - theta
        d0 = theta + 0.01 * cth
        for k in range(-64, 65):
            d = _steps(d0, k)
            quadrant = d - H * 0.0
            if quadrant > theta and (quadrant - theta) / cth == TOL:
                F.dX[r], F.dY[r] = 1000.0, dy
                F.theta = theta_rows(F.dX, F.dY, F.shape[0])
                for ii in range(F.shape[0]):                                  # the rows that share the new theta carry their own designed values
                    if F.theta[ii] == theta:
                        for j, lab in enumerate(F.label[ii]):
                            if lab is not None:
                                F.direction[ii, j] = dict((b, a) for a, b in designed_values(theta))[lab]
                F.set_direction(i, 0, d, 'exact_tol')
                F.z[i, 0] = 5300.0; F.z[i - 1, 0] = 5290.0; F.z[i - 1, 1] = 5310.0     # N lower (kept), NE higher (dropped)
                F.exact_tol_cell = (i, 0)
                return
    raise AssertionError('no direction gives a share of exactly 1e-2')


# ---------------------------------------------------------------------------------------------------------------------------
# the fields
@functools.lru_cache(maxsize=None)
def tiny_field():
    """(3, 3): all perimeter, one theta for every row; uniform spacing"""
    F = Field('tiny 3 x 3', 3, 3, np.full(2, 20.0), np.full(2, 30.0), np.full(3, 20.0), np.full(3, 30.0), 101).build()
    _corner(F, 'tl', 'insum_small')
    return F.seal()


@functools.lru_cache(maxsize=None)
def strip_field():
    """(3, 300): one interior row, a second, partly filled 256-column block; uniform spacing"""
    n, m = 3, 300
    F = Field('strip 3 x 300', n, m, np.full(n - 1, 30.0), np.full(n - 1, 17.0), np.full(n, 30.0), np.full(n, 17.0), 102).build()
    _keep_cases(F, [(1, 150 + 4 * k) for k in range(16)], (1, 220))
    _inlets(F, 'top', [(0, 230 + 4 * k) for k in range(4)])
    _inlets(F, 'bottom', [(2, 250 + 4 * k) for k in range(4)])
    _flat(F, [(0, 280), (1, 283), (2, 286), (0, m - 1)])
    _corner(F, 'tl', 'nan_elevation'); _corner(F, 'br', 'insum_large_no_out')
    return F.seal()


def _varying(n, lo, hi):
    dX, dY = np.linspace(lo[0], hi[0], n - 1), np.linspace(lo[1], hi[1], n - 1)
    return dX, dY, np.linspace(lo[0], hi[0], n), np.linspace(lo[1], hi[1], n)


@functools.lru_cache(maxsize=None)
def block_field():
    """(24, 300): a second, partly filled 256-column block, spacing that varies per row"""
    n, m = 24, 300
    F = Field('block 24 x 300', n, m, *_varying(n, (20.0, 31.0), (27.0, 19.0)), seed=103).build()
    _keep_cases(F, [(3 + 4 * (k // 8), 200 + 5 * (k % 8)) for k in range(32)], (9, 242))
    _inlets(F, 'left', [(4 + 4 * k, 0) for k in range(4)])
    _inlets(F, 'right', [(4 + 4 * k, m - 1) for k in range(4)])
    _inlets(F, 'top', [(0, 245 + 4 * k) for k in range(4)])
    _inlets(F, 'bottom', [(n - 1, 245 + 4 * k) for k in range(4)])
    _flat(F, [(0, 270), (n - 1, 273), (21, 0), (21, m - 1), (10, 275), (10, 276), (11, 276)])
    for corner, case in zip(('tl', 'tr', 'bl', 'br'), ('side_rule', 'outsum_alone', 'insum_zero', 'insum_small')):
        _corner(F, corner, case)
    return F.seal()


@functools.lru_cache(maxsize=None)
def tall_field():
    """(300, 5): 300 thetas from 83 to 9 degrees, rows 0 / 1 and n - 2 / n - 1 share theta through the clamp; a share of exactly 1e-2"""
    n, m = 300, 5
    F = Field('tall 300 x 5', n, m, *_varying(n, (5.0, 40.0), (50.0, 8.0)), seed=104).build()
    _keep_cases(F, [(20 + 4 * k, 2) for k in range(16)], (90, 2))
    _inlets(F, 'left', [(100 + 4 * k, 0) for k in range(4)])
    _inlets(F, 'right', [(120 + 4 * k, m - 1) for k in range(4)])
    _flat(F, [(150, 0), (152, 2), (154, m - 1)])
    _exact_tol(F, 200)
    for corner, case in zip(('tl', 'tr', 'bl', 'br'), ('outsum_alone', 'insum_large_no_out', 'side_rule', 'nan_elevation')):
        _corner(F, corner, case)
    return F.seal()


PITS = ((5, 10), (5, 40), (10, 25), (14, 55), (15, 12))


@functools.lru_cache(maxsize=None)
def pit_field():
    """(20, 70), drain_pits=True: single-cell pits, 2 below their lowest neighbour (flats = 1, mag = -1, direction = -1).  The pit
    search patches flats and mag there; section and proportion come from the mask as it was before"""
    n, m = 20, 70
    F = Field('pits 20 x 70', n, m, *_varying(n, (22.0, 30.0), (26.0, 21.0)), seed=105, drain_pits=True).build()
    for i, j in PITS:
        F.z[i, j] = F.z[i - 1:i + 2, j - 1:j + 2].min() - 2.0
    _flat(F, PITS)
    return F.seal()


@functools.lru_cache(maxsize=None)
def corner_field():
    """(5, 7): the corner rule's own 1e-2 (k_corner_todo) from both sides -- an in-sum and an out-sum of 0.0099 and of 0.0101, each
    the only thing that decides its corner"""
    n, m = 5, 7
    F = Field('corners 5 x 7', n, m, *_varying(n, (21.0, 33.0), (29.0, 18.0)), seed=106).build()
    for corner, case in zip(('tl', 'tr', 'bl', 'br'), ('insum_below', 'insum_above', 'outsum_below', 'outsum_above')):
        _corner(F, corner, case)
    return F.seal()


def graph_fields():
    return [tiny_field(), strip_field(), block_field(), tall_field(), pit_field(), corner_field()]


@functools.lru_cache(maxsize=None)
def oracle_of(F):
    """the CPU oracle after calc_uca on the field's planes, computed once per field and process and never changed"""
    import warnings
    from oracle import oracle as O
    o = O.OracleDEM(F.z, drain_pits=F.drain_pits, **F.spacing)
    o.mag, o.direction, o.flats = F.mag.copy(), F.direction.copy(), F.flats.copy()       # (the pit search patches mag and flats in place)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    return o


# ---------------------------------------------------------------------------------------------------------------------------
# the reference lines the oracle cites (dem_processing.py:1021-1070), in numpy
def section_proportion(direction, flats, dX, dY):
    """(section int8, proportion) of _calc_uca_section_proportion.  A NaN direction has no floor: both implementations convert it
    to sec0 = 0 (stated here, not computed)"""
    n, m = direction.shape
    theta = theta_rows(dX, dY, n)[:, None] * np.ones((1, m))                             # :1031-1033
    d = direction
    finite = np.isfinite(d)
    sec0 = np.zeros(d.shape, np.int8)
    sec0[finite] = np.floor(d[finite] / np.pi * 2).astype('int8')                        # :1035
    with np.errstate(invalid='ignore'):
        quadrant = d - np.pi / 2 * sec0                                                  # :1037
        section = (sec0 * 2 + ((quadrant > theta) & (sec0 % 2 == 0))
                   + ((quadrant > (np.pi / 2 - theta)) & (sec0 % 2 == 1))).astype('int8')   # :1040-1043
        proportion = np.full(d.shape, np.nan)
        I1 = (section == 0) | (section == 1) | (section == 4) | (section == 5)          # :1050
        I = I1 & (quadrant <= theta)
        proportion[I] = quadrant[I] / theta[I]                                           # :1052-1053
        I = I1 & (quadrant > theta)
        proportion[I] = (quadrant[I] - theta[I]) / (np.pi / 2 - theta[I])                # :1054-1056
        I = ~I1 & (quadrant <= (np.pi / 2 - theta))
        proportion[I] = quadrant[I] / (np.pi / 2 - theta[I])                             # :1057-1059
        I = ~I1 & (quadrant > (np.pi / 2 - theta))
        proportion[I] = (quadrant[I] - (np.pi / 2 - theta[I])) / theta[I]                # :1060-1062
    fl = np.asarray(flats, bool)
    section[fl] = -1; proportion[fl] = np.nan                                            # :1064-1065
    section[section == 8] = 0                                                            # :1067
    adjust = np.array([1, -1, 1, -1, 1, -1, 1, -1])                                      # ang_adj[:, 1]
    proportion = (1 + adjust[section]) / 2.0 - adjust[section] * proportion              # :1068
    return section, proportion


# ---------------------------------------------------------------------------------------------------------------------------
# what a field exercises, counted on the oracle's results
def graph_stats(F, section, proportion, A):
    """counts by name, from the oracle's section / proportion and CSC adjacency (indptr, indices, data) of the field"""
    n, m = F.shape
    z, d = F.z, F.direction
    indptr, indices, data = A
    c = {}
    theta = F.theta[:, None] * np.ones((1, m))
    nonflat = F.flats == 0
    with np.errstate(invalid='ignore'):
        sec0 = np.zeros((n, m), np.int64)
        ok = np.isfinite(d) & nonflat
        sec0[ok] = np.floor(d[ok] / np.pi * 2)
        quadrant = d - np.pi / 2 * sec0
        t1 = np.where(sec0 % 2 == 0, theta, H - theta)
        near = ok & (np.abs(quadrant - t1) <= 2.5 * np.spacing(d))
        for q in range(4):
            c['q%d quadrant > t1, within two steps' % q] = int((near & (sec0 == q) & (quadrant > t1)).sum())
            c['q%d quadrant <= t1, within two steps' % q] = int((near & (sec0 == q) & (quadrant <= t1)).sum())
        c['quadrant == theta (q = 0)'] = int((ok & (sec0 == 0) & (quadrant == theta)).sum())
        c['sec == 8 folds to 0'] = int((ok & (sec0 == 4)).sum())
        c['NaN direction on a cell that is not flat'] = int((np.isnan(d) & nonflat).sum())
        for s in range(-1, 8):
            c['section %d' % s] = int((section == s).sum())
        p = proportion
        c['proportion == 0'] = int((p == 0).sum()); c['proportion == 1'] = int((p == 1).sum())
        c['0 < proportion <= 1e-8'] = int(((p > 0) & (p <= 1e-8)).sum())
        c['0 < 1 - proportion <= 1e-8'] = int(((1 - p > 0) & (1 - p <= 1e-8)).sum())
        # keep-filter, per facet kind
        ii, jj = np.mgrid[0:n, 0:m]
        s = np.where((section >= 0) & (section <= 7), section, 0)
        real = (section >= 0) & (section <= 7)
        for kind, er, ec, w in (('cardinal', E1R, E1C, p), ('diagonal', E2R, E2C, 1 - p)):
            ti, tj = ii + er[s], jj + ec[s]
            inside = (ti >= 0) & (ti < n) & (tj >= 0) & (tj < m)
            zt = np.where(inside, z[np.clip(ti, 0, n - 1), np.clip(tj, 0, m - 1)], np.nan)
            big = real & (w > 1e-8)
            c[kind + ': outside'] = int((big & ~inside).sum())
            c[kind + ': lower'] = int((big & inside & (zt < z)).sum())
            c[kind + ': higher'] = int((big & inside & (zt > z)).sum())
            c[kind + ': equal'] = int((big & inside & (zt == z)).sum())
            c[kind + ': NaN target'] = int((big & inside & np.isnan(zt) & ~np.isnan(z)).sum())
            c[kind + ': NaN source'] = int((big & inside & ~np.isnan(zt) & np.isnan(z)).sum())
            down = real & inside & (zt <= z)
            c[kind + ': 1e-9 < w <= 1e-8, target lower'] = int((down & (w > 1e-9) & (w <= 1e-8)).sum())
            c[kind + ': 1e-8 < w <= 1e-7, target lower'] = int((down & (w > 1e-8) & (w <= 1e-7)).sum())
            c[kind + ': w == 0, target lower'] = int((down & (w == 0)).sum())
            c[kind + ': w is NaN'] = int((real & inside & np.isnan(w)).sum())
    # sums of the kept edges
    NN = n * m
    outdeg = np.diff(indptr)
    src = np.repeat(np.arange(NN), outdeg)
    outsum = np.bincount(src, data, NN).reshape(n, m)
    insum = np.bincount(indices, data, NN).reshape(n, m)
    outdeg = outdeg.reshape(n, m)
    for k in range(3):
        c['out-degree %d' % k] = int((outdeg == k).sum())
    sides = dict(left=(slice(1, n - 1), 0), right=(slice(1, n - 1), m - 1), top=(0, slice(1, m - 1)), bottom=(n - 1, slice(1, m - 1)))
    for side, sl in sides.items():
        inlet = np.isin(section[sl], SIDE_SECTIONS[side]) & (outdeg[sl] == 1)
        o = outsum[sl]
        c[side + ': one kept edge, outsum in (0.0098, 1e-2)'] = int((inlet & (o > 0.0098) & (o < TOL)).sum())
        c[side + ': one kept edge, outsum in (1e-2, 0.0102)'] = int((inlet & (o > TOL) & (o < 0.0102)).sum())
        c['outsum == 1e-2 on an inlet section'] = c.get('outsum == 1e-2 on an inlet section', 0) + int((inlet & (o == TOL)).sum())
    for case in CORNER_CASES:
        c['corner: ' + case] = 0
    for (ci, cj), row_side in (((0, 0), 'top'), ((0, m - 1), 'top'), ((n - 1, 0), 'bottom'), ((n - 1, m - 1), 'bottom')):
        o, i_, sec = outsum[ci, cj], insum[ci, cj], section[ci, cj]
        side_rule = o > TOL and sec in SIDE_SECTIONS[row_side]                # (at a corner the row's rule overwrites the column's, :917-919)
        if np.isnan(z[ci, cj]):
            case = 'nan_elevation' if (side_rule or o > TOL or i_ < TOL) else None
        elif side_rule:
            case = 'side_rule'
        elif TOL < o < 0.0102:
            case = 'outsum_above' if i_ >= TOL else None
        elif 0.0098 < o < TOL:
            case = 'outsum_below' if i_ >= TOL else None
        elif o > TOL:
            case = 'outsum_alone' if i_ >= TOL else None
        elif i_ == 0:
            case = 'insum_zero'
        elif 0.0098 < i_ < TOL:
            case = 'insum_below' if outdeg[ci, cj] == 0 else None
        elif TOL < i_ < 0.0102:
            case = 'insum_above' if outdeg[ci, cj] == 0 else None
        elif i_ < TOL:
            case = 'insum_small' if outdeg[ci, cj] == 0 else None
        else:
            case = 'insum_large_no_out' if outdeg[ci, cj] == 0 else None
        if case:
            c['corner: ' + case] += 1
    return c


def merge_counts(dicts):
    out = {}
    for dct in dicts:
        for k, v in dct.items():
            out[k] = out.get(k, 0) + v
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# TWI
class TwiCase(object):
    """uca, mag and the options of calc_twi (reference :1647-1677)"""

    def __init__(self, name, uca, mag, min_slope=1e-3, min_area=np.inf, sat=32.0, lim_twi=False, lim_uca=False):
        self.name = name
        self.uca, self.mag = np.ascontiguousarray(uca, np.float64), np.ascontiguousarray(mag, np.float64)
        self.uca.setflags(write=False); self.mag.setflags(write=False)
        self.min_slope, self.min_area, self.sat, self.lim_twi, self.lim_uca = float(min_slope), float(min_area), float(sat), bool(lim_twi), bool(lim_uca)

    @property
    def options(self):
        return dict(twi_min_slope=self.min_slope, twi_min_area=self.min_area, uca_saturation_limit=self.sat,
                    apply_twi_limits=self.lim_twi, apply_twi_limits_on_uca=self.lim_uca)

    def quotient(self):
        """the float64 quotient whose logarithm is taken: one comparison, one addition, one correctly rounded division"""
        t = self.uca.copy()
        if self.lim_uca:
            cap = self.sat * self.min_area
            t[t > cap] = cap
        with np.errstate(all='ignore'):
            return t / (self.mag + self.min_slope)

    def cap(self):
        with np.errstate(all='ignore'):
            return math.log(self.sat * self.min_area / self.min_slope) if np.isfinite(self.min_area) else np.inf


MIN_SLOPE_2 = 2.0 ** -10          # with mag = 1 - 2^-10 the divisor is exactly 1: the quotient is uca


NEAR_CAP_ULPS = (-4, -3, -2, -1, 0, 1, 2, 3, 4)


def near_cap_quotient(ratio, j):
    """The quotient next to `ratio` whose logarithm lies j ulp from cap = log(ratio) (the float64 value the host forms), as near to
    the middle of that float64's rounding interval as the quotient's steps allow: a step of the quotient moves the logarithm by
    spacing(ratio) / ratio, a few hundredths of an ulp of the cap, so stepping the quotient itself by one or two never leaves the
    cap.  Any logarithm good to 0.4 ulp returns cap + j ulp there; one good to 3 ulp is below the cap at j = -4, above at j = 4."""
    cap = math.log(ratio)
    ulp = np.spacing(cap)
    per_step = np.spacing(ratio) / ratio / ulp
    span = int(np.ceil((abs(j) + 1) / per_step))
    q = ratio + np.arange(-span, span + 1) * np.spacing(ratio)              # (exact: a few hundred steps inside one binade)
    assert (np.diff(q) == np.spacing(ratio)).all()
    miss = np.abs(np.log(q.astype(L)) - (L(cap) + L(j) * L(ulp))) / L(ulp)
    k = int(np.argmin(miss))
    assert miss[k] < 0.1, (ratio, j, float(miss[k]))
    return float(q[k])


def _special_planes(min_slope, min_area, sat):
    """the (7, 9) tile of specials for one option set, with the divisor 1 wherever the quotient is chosen"""
    one = 1.0 - min_slope
    assert one + min_slope == 1.0
    q = [1.0] + [_steps(1.0, k) for k in STEPS]
    q += [5e-324, 7 * 5e-324, 2.0 ** -1040, 2.2250738585072014e-308, np.finfo(np.float64).max, 1e308]
    q += [0.0, np.nan, np.inf]
    cap_u = sat * min_area
    if np.isfinite(cap_u):
        q += [cap_u, _steps(cap_u, -1), _steps(cap_u, 1)]
        ratio = cap_u / min_slope                  # log(ratio) is the cap: results at the cap and next to it (divisor min_slope below)
    uca, mag = list(q), [one] * len(q)
    if np.isfinite(cap_u):
        for k in (-1, 0, 1):
            uca.append(_steps(ratio, k) * min_slope); mag.append(0.0)     # the cap's own quotient and its neighbours, divisor 0 + min_slope
        for j in NEAR_CAP_ULPS:
            uca.append(near_cap_quotient(ratio, j)); mag.append(one)      # results j ulp from the cap, divisor 1
    # divisors: negative (mag = -1: a flat), NaN, exactly zero (mag = -min_slope) with uca > 0 and with uca = 0
    uca += [3.0, 3.0, 3.0, 0.0, np.inf]; mag += [-1.0, np.nan, -min_slope, -min_slope, -min_slope]
    uca = np.array(uca + [2.5] * (63 - len(uca))); mag = np.array(mag + [0.25] * (63 - len(mag)))
    assert uca.size == 63
    return uca.reshape(7, 9), mag.reshape(7, 9)


def twi_cases(large=True):
    """Every TWI case: the specials under all four settings of the limits and with twi_min_area = inf, quotients 1 +- 2^-k, 30
    decades of seeded log-uniform values, and (large=True) a tile of more cells than k_twi's grid holds threads"""
    out = []
    for lim_twi in (False, True):
        for lim_uca in (False, True):
            for min_area, tag in ((900.0, '900'), (np.inf, 'inf')):
                u, g = _special_planes(MIN_SLOPE_2, min_area, 32.0)
                out.append(TwiCase('specials twi=%d uca=%d area=%s' % (lim_twi, lim_uca, tag), u, g, MIN_SLOPE_2, min_area, 32.0, lim_twi, lim_uca))
    k = np.arange(10, 53)
    near = np.concatenate([1 + 2.0 ** -k, 1 - 2.0 ** -k, 1 + 3 * 2.0 ** -k, 1 - 3 * 2.0 ** -k])
    near = np.concatenate([near, np.full(180 - near.size, 1.0)]).reshape(4, 45)
    out.append(TwiCase('near one', near, np.full(near.shape, 1.0 - MIN_SLOPE_2), MIN_SLOPE_2))
    rng = np.random.default_rng(7)
    uca = 10.0 ** rng.uniform(-5, 25, (40, 300)); mag = 10.0 ** rng.uniform(-6, 1, (40, 300))
    for lim_twi, lim_uca in ((False, False), (True, False), (True, True)):
        out.append(TwiCase('thirty decades twi=%d uca=%d' % (lim_twi, lim_uca), uca, mag, 1e-3, 625.0, 32.0, lim_twi, lim_uca))
    if large:
        out.append(large_twi_case())
    return out


@functools.lru_cache(maxsize=None)
def large_twi_case():
    """(1000, 2100): 2 100 000 cells > 8192 x 256 threads of k_twi's grid: the grid-stride trip runs, the last one partial; uca
    and mag are functions of the cell index"""
    n, m = 1000, 2100
    c = np.arange(n * m, dtype=np.float64)
    uca = (900.0 + 0.37 * c).reshape(n, m)
    mag = (np.mod(c * 7919.0, 1000.0) / 1000.0).reshape(n, m)
    return TwiCase('large', uca, mag, 1e-3, 900.0, 32.0, True, True)


def twi_check(case, twi, ref_twi, bound):
    """The bars of a TWI plane against the oracle's (ref_twi) and the logarithm in long double.  Returns (worst error in ulps of the
    long-double value over the cells that are measured, number of cells measured, number of cells held to the oracle's bits).
      - NaN, -inf, +inf where the oracle has them;
      - where the long-double logarithm is beyond the cap by more than `bound` ulps, any conforming logarithm is capped: the
        oracle's bits (the cap is a host log in both);
      - elsewhere |twi - min(log q, cap)| in ulps of that value, and never above the cap."""
    twi, ref = np.asarray(twi, np.float64).ravel(), np.asarray(ref_twi, np.float64).ravel()
    q = case.quotient().ravel()
    for name, f in (('NaN', np.isnan), ('-inf', np.isneginf), ('+inf', np.isposinf)):
        assert np.array_equal(f(twi), f(ref)), '%s: %s pattern differs (%d against %d)' % (case.name, name, f(twi).sum(), f(ref).sum())
    cap = case.cap() if case.lim_twi else np.inf
    with np.errstate(all='ignore'):
        logq = np.log(q.astype(L))
        fin = np.isfinite(ref)
        if np.isfinite(cap):
            sure = fin & (logq > L(cap) + L(bound) * L(np.spacing(abs(cap))))
        else:
            sure = np.zeros(q.shape, bool)
        assert np.array_equal(twi[sure].view(np.int64), ref[sure].view(np.int64)), '%s: capped cells differ from the oracle' % case.name
        rest = fin & ~sure
        want = np.minimum(logq[rest], L(cap))
        assert (twi[rest] <= cap).all(), '%s: a value above the cap' % case.name
        unit = np.spacing(np.abs(want.astype(np.float64))).astype(L)
        ulps = np.abs(twi[rest].astype(L) - want) / unit
    worst = float(ulps.max()) if ulps.size else 0.0
    return worst, int(rest.sum()), int(sure.sum())
