"""Designed flats for the distance sweeps of fill_flats (csrc/cond_device.hip, stage_fill_flats).  TEST INFRASTRUCTURE ONLY.

The reference stops each chamfer distance of a flat in the sweep in which its last cell gets a FIRST value, not at
convergence (tests/conditioning_numpy.py::_chamfer_distance), so the stopping sweep is part of the result -- but on an
ordinary lake the distances are already final by then and a region that stops a sweep late goes unnoticed.  It shows
only where a cheaper path with MORE hops than the region's last first arrival exists.  The zigzag lake is built for
that: a one-cell-wide corridor of 2k diagonal hops (cost 2k sqrt 2) whose two ends are also joined by a cardinal detour
v rows below it (2k + 2v hops, cost 2k + 2v).  The corridor brings the first values, the detour the final ones, later.

Every field is a small integer-valued tile (so it also fits int16) on a tilted plane that has no flats of its own; the
cells around a lake are set explicitly: its ring to level + 5, one ring cell to level + 1 (the only source within the
reference's source tolerance), one ring cell to the level itself with a cell at level - 1 beyond it (the outlet; the
cell beyond is a one-pixel pit, a labelled region of its own that fill_flats leaves alone).  What each field is (the
labelled regions, the stop sweeps, the sizes against the engine thresholds) is pinned by tests/test_flat_fields.py;
tests/test_gpu_flat_engines.py runs them through every sweep engine of the device."""
from collections import namedtuple

import numpy as np

LEVEL = 100.0
Lake = namedtuple('Lake', 'name mask')
Field = namedtuple('Field', 'name z lakes sinks')        # sinks: the one-pixel pits beyond the outlets


def _grow(mask):
    """The mask and its 8-neighbours (inside the array)."""
    out = mask.copy()
    n, m = mask.shape
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            out[max(0, di):n + min(0, di), max(0, dj):m + min(0, dj)] |= mask[max(0, -di):n + min(0, -di), max(0, -dj):m + min(0, -dj)]
    return out


class _Tile:
    def __init__(self, name, n, m, base=1000.0):
        i, j = np.mgrid[0:n, 0:m]
        self.name = name
        self.z = base + 3.0 * i + 7.0 * j          # strictly rising along both axes: only the corner (0, 0) is a minimum
        self.lakes, self.sinks = [], []
        self.taken = np.zeros((n, m), bool)

    def lake(self, name, cells, level=LEVEL, source=None, outlet=None, sink=None):
        mask = np.zeros(self.z.shape, bool)
        if isinstance(cells, np.ndarray):
            mask |= cells
        else:
            ii, jj = zip(*cells)
            assert min(ii) >= 0 and min(jj) >= 0
            mask[list(ii), list(jj)] = True
        ring = _grow(mask) & ~mask
        own = mask | ring
        if sink is not None:
            one = np.zeros_like(mask)
            one[sink] = True
            assert not (_grow(one) & mask).any(), "the pit beyond the outlet touches the lake"
            own |= _grow(one)
        assert not (own & self.taken).any(), "%s overlaps an earlier lake" % name
        self.taken |= own
        self.z[ring] = level + 5
        self.z[mask] = level
        if source is not None:
            assert ring[source]
            self.z[source] = level + 1
        if outlet is not None:
            assert ring[outlet] and sink is not None and not own[0, 0]
            self.z[outlet] = level
            self.z[sink] = level - 1
            self.sinks.append(tuple(int(v) for v in sink))
        self.lakes.append(Lake(name, mask))

    def field(self):
        assert np.array_equal(self.z, np.round(self.z)) and self.z.max() < 32767 and self.z.min() > 0
        return Field(self.name, self.z, self.lakes, self.sinks)


def zigzag_cells(k, v, r0, c0, spur=0):
    """Corridor between rows r0 and r0 + 1 from (r0 + 1, c0) to (r0 + 1, c0 + 2k); detour down both end columns and along
    row r0 + 1 + v.  2 (2k + 1) + 2 (v - 1) cells; with its ring, source, outlet and pit it covers rows r0 - 1 .. r0 + 2 + v,
    columns c0 - 3 .. c0 + 2k + 1.  `spur`: a dead end of that many cells along row r0 + 3, inside the loop, from the
    first column of the detour."""
    assert k >= 2 and v >= 2
    cells = [(r0 + 1 - (c & 1), c0 + c) for c in range(2 * k + 1)]
    cells += [(r, c0) for r in range(r0 + 2, r0 + 1 + v)] + [(r, c0 + 2 * k) for r in range(r0 + 2, r0 + 1 + v)]
    cells += [(r0 + 1 + v, c0 + c) for c in range(2 * k + 1)]
    if spur:
        assert v >= 4 and spur + 4 <= 2 * k        # two rows from the corridor and from the detour, the pit clear of the far column
        cells += [(r0 + 3, c0 + c) for c in range(1, spur + 1)]
    return cells


ZIG_ROWS = lambda v: v + 4          # rows / columns of the footprint above
ZIG_COLS = lambda k: 2 * k + 5


def _add_zigzag(t, name, k, v, r0, c0, apart=0):
    """Source beside the start of the corridor.  The outlet beside it too -- both distances then stop one sweep apart, half
    way round the loop -- or (`apart` = length of the spur) at the end of a spur: the outlet distance has the spur to
    walk before it goes round the loop and stops that many sweeps later."""
    if apart:
        outlet, sink = (r0 + 3, c0 + apart + 1), (r0 + 3, c0 + apart + 2)
    else:
        outlet, sink = (r0 + 1, c0 - 1), (r0 + 1, c0 - 2)
    t.lake(name, zigzag_cells(k, v, r0, c0, apart), source=(r0, c0 - 1), outlet=outlet, sink=sink)


def zigzag(k, v, apart=0):
    t = _Tile('zigzag_k%d_v%d%s' % (k, v, '_apart%d' % apart if apart else ''), ZIG_ROWS(v) + 4, ZIG_COLS(k) + 4)
    _add_zigzag(t, 'zig', k, v, 3, 5, apart)
    return t.field()


def _square(r0, c0, h, w):
    return [(r, c) for r in range(r0, r0 + h) for c in range(c0, c0 + w)]


def _add_square(t, name, r0, c0, h, w):
    """A plain lake: source at the middle of its top side, outlet (and the pit beyond) at the middle of its left side."""
    t.lake(name, _square(r0, c0, h, w), source=(r0 - 1, c0 + w // 2), outlet=(r0 + h // 2, c0 - 1), sink=(r0 + h // 2, c0 - 2))


# (k, v, apart) of the family, in shelf order: the stops (pinned in tests/test_flat_fields.py) spread over the sweeps of
# the 16-sweep passes that start at sweep 33
FAMILY = [(16, 2, 0), (17, 3, 0), (18, 4, 10), (19, 3, 0), (20, 4, 0), (21, 2, 0), (22, 4, 12),
          (23, 4, 0), (24, 2, 0), (25, 5, 0), (26, 3, 0), (27, 4, 20), (28, 2, 0), (29, 3, 0),
          (30, 3, 0), (31, 5, 0), (32, 4, 0), (33, 4, 25), (34, 3, 0), (36, 5, 0), (38, 4, 0),
          (40, 5, 0), (44, 5, 30), (47, 5, 0)]


def zig_family():
    """24 zigzags on shelves 9 rows apart (one shelf has its corridor on rows 31 / 32, across a corner of four 32 x 32
    blocks), and below them one plain 96 x 96 lake: 9216 cells, more than the resident-workgroup kernel takes, so that
    with no environment set the first 32 sweeps are launches per sweep and the several-sweeps-per-pass engine starts at
    sweep 33, like with PYDEM_FLAT_COOP=0 PYDEM_FLAT_SMALL=0."""
    width = 236
    shelves, row, used = [], [], 0
    for k, v, apart in FAMILY:
        w = ZIG_COLS(k) + 1
        if used + w > width - 2:
            shelves.append(row)
            row, used = [], 0
        row.append((k, v, apart, used + 4))
        used += w
    shelves.append(row)
    top = 13
    t = _Tile('zig_family', top + 9 * len(shelves) + 4 + 96 + 4, width)
    for s, row in enumerate(shelves):
        for k, v, apart, c0 in row:
            _add_zigzag(t, 'zig_k%d_v%d%s' % (k, v, '_apart%d' % apart if apart else ''), k, v, top + 9 * s, c0, apart)
    _add_square(t, 'ballast', top + 9 * len(shelves) + 3, 60, 96, 96)
    return t.field()


def default_route():
    """One 130 x 130 lake (16900 cells: longer than the list the several-sweeps-per-pass engine accepts, so sweeps 1-32
    are launches per sweep whatever the environment) and three zigzags that stop in the middle of later passes."""
    t = _Tile('default_route', 140, 262)
    _add_square(t, 'square', 5, 5, 130, 130)
    _add_zigzag(t, 'zig_k30_v3', 30, 3, 8, 145)
    _add_zigzag(t, 'zig_k40_v5', 40, 5, 30, 145)
    _add_zigzag(t, 'zig_k52_v4_apart30', 52, 4, 60, 145, apart=30)
    return t.field()


def long_zigzag(k=262, v=5):
    """One zigzag that stops after sweep 513: a few hundred cells on the list, for more sweeps than one launch of the
    resident-workgroup kernel runs."""
    t = _Tile('long_zigzag', ZIG_ROWS(v) + 11, ZIG_COLS(k) + 8)
    _add_zigzag(t, 'zig', k, v, 6, 7)
    return t.field()


def edge_lakes():
    """75 x 117 (neither a multiple of 32): four lakes without a level outlet, each touching one side of the tile -- the
    last (ragged) block row and column, the first row and column -- and at least 40 cells deep from it, so that their cells
    on the tile edge are the outlet seeds and the distances from them still run at sweep 33."""
    t = _Tile('edge_lakes', 75, 117)
    t.lake('bottom', _square(30, 40, 45, 21), source=(29, 50))
    t.lake('right', _square(5, 70, 21, 47), source=(15, 69))
    t.lake('top', _square(0, 5, 45, 21), source=(45, 15))
    t.lake('left', _square(50, 0, 21, 36), source=(60, 36))
    return t.field()


def centre_seeds():
    """A summit plateau and a closed depression, 72 x 72 flat cells each, on a LOW plane (around a rectangle every plane cell
    keeps a lower plane neighbour).  The plateau is 74 x 74 cells at one level with everything around it lower: its outer
    cells have a lower neighbour and are not flat -- they are the level ring of the flat inside, its outlet -- and with no
    higher cell around it the uphill seed is the centre cell.  The depression has every ring cell higher, one of them the
    source, and no outlet: the outlet seed is its centre cell."""
    t = _Tile('centre_seeds', 84, 168, base=10.0)
    plateau = np.zeros(t.z.shape, bool)
    plateau[5:79, 5:79] = True
    summit = np.zeros(t.z.shape, bool)
    summit[6:78, 6:78] = True
    t.z[plateau] = 5000.0
    t.lakes.append(Lake('summit', summit))
    t.taken |= _grow(plateau)
    t.lake('depression', _square(6, 90, 72, 72), level=3000.0, source=(5, 120))
    return t.field()


def all_fields():
    return [zigzag(30, 3), zigzag(40, 5), zigzag(30, 4, apart=20), zig_family(), default_route(), long_zigzag(),
            edge_lakes(), centre_seeds()]
