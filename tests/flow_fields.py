"""Flow fields designed for the engine the flow-graph sweeps share (csrc/flowdist.h: calc_dist_down / calc_hand, calc_dist_up,
calc_up_dependence / calc_watershed / calc_rev_accum): 32 x 32 tile passes with halo stamps, the "visit only if a neighbour
progressed" rule and a parity pair of progress words, then a Kahn queue for what the passes leave.  Fractal terrain has short
chains, few rounds per visit, pits that drain into the next tile and every facet section mixed into every tile; each field
here isolates one of those:

    row_snake    one chain over the whole grid that crosses a tile boundary in every row: dozens of passes
    tile_snake   a column snake inside each tile: 1024 rounds in one visit, one visit per tile
    fan(k)       one facet section k, two out-edges per cell with p != 1 - p: every tile edge and corner in two directions
    far_pit      one pit whose drains all lie two tiles away: only the stall-then-queue fallback finishes it
    near_pit     one pit at a tile corner with drains in the three other tiles around the corner
    tall, wide   chains longer than the row kernels' grid (more than 4096 rows) and than one workgroup's 256 columns

and for the UCA sweep (csrc/uca.hip, tests/test_gpu_uca_fields.py), whose edge taint reaches every cell of the fields above:

    roof(kl, kr) two fans side by side that flow apart: only one of the top and bottom rows is an inlet row, so the taint
                 covers part of the grid and part of most 32-blocks
    tile_snake_wide        tile_snake over five blocks of columns: two of them are wholly open after the two full passes
    tall_long, wide_long   tall and wide with a side of 16500: past the 16384 rows / 64 x 256 columns of the capped launches
    strip        a 16500 x 5 or 5 x 16500 fractal tile, slopes computed: the same caps with flats, pits and every section

A field is a `Field`: the elevation, the spacing, the options of OracleDEM / DEMProcessor, mag / direction / flats where the
field is hand-made (None: the slopes are computed), the target of the downslope calls and `facts`, what the tests assert
about it.  Hand-made fields take drain_pits=False and dX = 2, dY = 3; so do the computed ones unless they say otherwise.
tests/test_flow_fields.py pins on the oracle's graph what each field is; tests/test_gpu_flow_fields.py runs them on the device.
The processor accepts the three columns of tall() and the three rows of wide().

Not product code: numpy only, seeded and deterministic."""
import collections
import functools
import warnings

import numpy as np

T = 32                  # the tile edge of the passes (DD_T)
E, N, W, S = 0.0, 0.5 * np.pi, np.pi, 1.5 * np.pi
_STEP = {(0, 1): E, (-1, 0): N, (0, -1): W, (1, 0): S}

Field = collections.namedtuple('Field', 'name elev spacing options mag direction flats target facts')


def _spacing():
    return dict(dX=2.0, dY=3.0)


def crossings(path):
    """steps of the path whose two cells lie in different 32-blocks"""
    p = np.asarray(path)
    b = p // T
    return int((b[1:] != b[:-1]).any(axis=1).sum())


def longest_run_in_one_block(path):
    """the longest run of consecutive path cells inside one 32-block"""
    p = np.asarray(path)
    b = p // T
    cut = np.flatnonzero((b[1:] != b[:-1]).any(axis=1)) + 1
    return int(np.diff(np.r_[0, cut, len(p)]).max())


def _from_paths(name, shape, paths, last=E, **facts):
    """The hand-made field of chains: every cell of a path points at the next one (a cardinal direction: one out-edge),
    the last one along `last`, which must lead off the grid; the elevation falls 0.5 per step."""
    n, m = shape
    elev = np.zeros(shape)
    direction = np.full(shape, np.nan)
    target = np.zeros(shape, bool)
    for path in paths:
        p = np.asarray(path)
        step = np.diff(p, axis=0)
        assert (np.abs(step).sum(axis=1) == 1).all(), "%s: the path is not adjacent at every step" % name
        direction[p[:-1, 0], p[:-1, 1]] = [_STEP[tuple(s)] for s in step.tolist()]
        direction[p[-1, 0], p[-1, 1]] = last
        elev[p[:, 0], p[:, 1]] = 0.5 * (len(p) - 1 - np.arange(len(p)))
        target[p[-1, 0], p[-1, 1]] = True
    assert not np.isnan(direction).any() and sum(len(p) for p in paths) == n * m, "%s: the paths do not cover the grid once" % name
    longest = max(paths, key=len)
    facts.update(paths=[np.asarray(p) for p in paths], path=np.asarray(longest), depth=len(longest), crossings=crossings(longest))
    return Field(name, elev, _spacing(), dict(drain_pits=False), np.ones(shape), direction, np.zeros(shape, bool), target, facts)


@functools.lru_cache(maxsize=None)
def row_snake(n=70, m=45):
    """A boustrophedon over the whole grid: east along row 0, west along row 1, ...: one chain of n * m cells."""
    path = [(i, j) for i in range(n) for j in (range(m) if i % 2 == 0 else range(m - 1, -1, -1))]
    return _from_paths('row_snake', (n, m), [path], last=(W if n % 2 == 0 else E))


@functools.lru_cache(maxsize=None)
def tile_snake(n=40, m=70, name='tile_snake'):
    """A column snake inside each 32-block (down column 0, up column 1, ...), which leaves the block at the top of its last
    column for the block to the east; one chain per tile row.  Every block, the ragged ones included, needs an even number
    of columns for that."""
    paths = []
    for i0 in range(0, n, T):
        rows = list(range(i0, min(i0 + T, n)))
        path = []
        for j0 in range(0, m, T):
            cols = range(j0, min(j0 + T, m))
            assert len(cols) % 2 == 0, "tile_snake: a block of %d columns ends at the bottom of its last column" % len(cols)
            for j in cols:
                path += [(i, j) for i in (rows if (j - j0) % 2 == 0 else rows[::-1])]
        paths.append(path)
    f = _from_paths(name, (n, m), paths, last=E)
    f.facts['longest_run'] = longest_run_in_one_block(f.facts['path'])
    return f


def tile_snake_wide():
    """tile_snake over five blocks of columns: the first two full passes of the UCA sweep finish one block each, so the third
    and fourth block are open in all their 1024 cells when the pass after them visits them"""
    return tile_snake(40, 134, 'tile_snake_wide')


@functools.lru_cache(maxsize=None)
def fan(k, mirror=False, n=70, m=45):
    """Uniform direction (k + 0.3) pi / 4 on a plane that falls along it: facet section k everywhere, two out-edges per cell
    away from the outflow border.  mirror: the left-right mirror of the field (direction pi - d, columns reversed)."""
    d = (k + 0.3) * np.pi / 4
    sp = _spacing()
    ii, jj = np.indices((n, m))
    x, y = jj * sp['dX'], -ii * sp['dY']                     # east and north of the cell (0, 0)
    elev = 1000.0 - (x * np.cos(d) + y * np.sin(d))
    if mirror:
        d = (np.pi - d) % (2 * np.pi)
        elev = np.ascontiguousarray(elev[:, ::-1])
    direction = np.full((n, m), d)
    # the outflow border: the cells one of whose two facet neighbours lies off the grid
    e1 = [(0, 1), (-1, 0), (-1, 0), (0, -1), (0, -1), (1, 0), (1, 0), (0, 1)]
    e2 = [(-1, 1), (-1, 1), (-1, -1), (-1, -1), (1, -1), (1, -1), (1, 1), (1, 1)]
    sec = int(np.floor(d / (np.pi / 4) + 1e-9)) % 8 if not mirror else (3 - k) % 8
    target = np.zeros((n, m), bool)
    for di, dj in (e1[sec], e2[sec]):
        target |= (ii + di < 0) | (ii + di >= n) | (jj + dj < 0) | (jj + dj >= m)
    name = 'fan%d%s' % (k, '_mirror' if mirror else '')
    return Field(name, elev, sp, dict(drain_pits=False), np.ones((n, m)), direction, np.zeros((n, m), bool), target,
                 dict(section=sec, k=k))


def _row_varying(n):
    import capacity_terrain as CT
    dX, dY = CT.spacing(n, seed=4)
    return dict(dX=dX, dY=dY, dX2=np.r_[dX, dX[-1]] + 0.003, dY2=np.r_[dY[0], dY] - 0.007)


@functools.lru_cache(maxsize=None)
def far_pit(row_varying=False, max_dist=60):
    """A pyramid basin of Chebyshev radius 50 around the pit (16, 16) on a gentle plane, slopes computed: with a reach of 60
    cells the pit drains over the basin's rim, two tiles away.  row_varying: the spacing of capacity_terrain.spacing, so the
    pit edges span 50 rows of different cell sizes.  max_dist=None: the default reach (the pit finds no drain)."""
    n, m = 96, 112
    ii, jj = np.indices((n, m))
    r = np.maximum(np.abs(ii - 16), np.abs(jj - 16))
    elev = np.where(r <= 50, 100.0 + r, 50.0 - 0.01 * (ii + jj))
    opt = dict(drain_pits=True)
    if max_dist is not None:
        opt['drain_pits_max_dist'] = max_dist
    name = 'far_pit%s%s' % ('_rows' if row_varying else '', '' if max_dist == 60 else '_reach_%s' % max_dist)
    return Field(name, elev, _row_varying(n) if row_varying else _spacing(), opt, None, None, None, elev < 60, dict(pit=(16, 16), radius=50))


@functools.lru_cache(maxsize=None)
def near_pit():
    """The plane 1000 - i - 1.3 j with the cell (30, 30) lowered 0.05 below (31, 31): a pit at the corner of the block (0, 0)
    with drains, at the default reach, in the three other blocks around that corner."""
    n, m = 70, 45
    ii, jj = np.indices((n, m))
    elev = 1000.0 - ii - 1.3 * jj
    elev[30, 30] = elev[31, 31] - 0.05
    target = np.zeros((n, m), bool)
    target[-1, :] = True
    target[:, -1] = True
    return Field('near_pit', elev, _spacing(), dict(drain_pits=True), None, None, None, target, dict(pit=(30, 30)))


@functools.lru_cache(maxsize=None)
def tall(n=4100, m=3, name='tall'):
    """Every column flows south: chains of n cells, more rows than the grid of the row kernels has workgroups (4096)."""
    paths = [[(i, j) for i in range(n)] for j in (1, 0, 2)]            # (the middle column first: `path` is that one)
    return _from_paths(name, (n, m), paths, last=S)


@functools.lru_cache(maxsize=None)
def wide(n=3, m=700, name='wide'):
    """Every row flows west: chains of m cells over three workgroups of the row kernels (256 columns each)."""
    paths = [[(i, j) for j in range(m - 1, -1, -1)] for i in (1, 0, 2)]
    return _from_paths(name, (n, m), paths, last=W)


LONG = 16500            # more rows than the row and column kernels of csrc/uca.hip have workgroups (16384) or threads


def tall_long():
    """tall with 16500 rows: the grid-stride branch of every kernel whose grid is capped at 16384 rows"""
    return tall(LONG, 3, 'tall_long')


def wide_long():
    """wide with 16500 columns: 65 workgroups of 256 columns where the capped launches have 64"""
    return wide(3, LONG, 'wide_long')


@functools.lru_cache(maxsize=None)
def roof(kl, kr, n=70, m=90):
    """Two fans side by side: the columns left of m // 2 take the uniform direction (kl + 0.3) pi / 4, the others
    (kr + 0.3) pi / 4, each half on the plane of `fan` that falls along its direction.  With (kl, kr) = (3, 0) or (4, 7) the
    halves flow apart, no edge crosses the ridge, and only the bottom (top) row is an inlet row: the edge taint spreads over
    part of the grid only."""
    sp = _spacing()
    ii, jj = np.indices((n, m))
    x, y = jj * sp['dX'], -ii * sp['dY']
    left = jj < m // 2
    direction = np.where(left, (kl + 0.3) * np.pi / 4, (kr + 0.3) * np.pi / 4)
    elev = 1000.0 - (x * np.cos(direction) + y * np.sin(direction))
    e1 = [(0, 1), (-1, 0), (-1, 0), (0, -1), (0, -1), (1, 0), (1, 0), (0, 1)]
    e2 = [(-1, 1), (-1, 1), (-1, -1), (-1, -1), (1, -1), (1, -1), (1, 1), (1, 1)]
    target = np.zeros((n, m), bool)
    for half, k in ((left, kl), (~left, kr)):
        for di, dj in (e1[k], e2[k]):
            target |= half & ((ii + di < 0) | (ii + di >= n) | (jj + dj < 0) | (jj + dj >= m))
    return Field('roof%d%d' % (kl, kr), elev, sp, dict(drain_pits=False), np.ones((n, m)), direction, np.zeros((n, m), bool), target,
                 dict(sections=(kl, kr), ridge=m // 2))


@functools.lru_cache(maxsize=None)
def strip(shape, seed=61):
    """A fractal tile five cells across and 16500 long, slopes computed, pits drained: flats, pits and every facet section
    where one side is longer than the capped grids of the row, column and line-gather kernels."""
    from pydem_amd import synth
    elev = synth.fractal(shape[0], shape[1], seed=seed, top_shift=7, n_octaves=7)
    return Field('strip_%dx%d' % shape, elev, dict(dX=30.0, dY=30.0), dict(drain_pits=True), None, None, None, None, dict(seed=seed))


def blocks_mixed(mask):
    """(32-blocks that hold both True and False cells of `mask`, all 32-blocks)"""
    n, m = mask.shape
    mixed = total = 0
    for i0 in range(0, n, T):
        for j0 in range(0, m, T):
            b = mask[i0:i0 + T, j0:j0 + T]
            total += 1
            mixed += bool(b.any() and not b.all())
    return mixed, total


def oracle(field):
    """The CPU oracle on the field, after calc_uca (o.A is the flow graph)."""
    from oracle import oracle as O
    o = O.OracleDEM(field.elev, **dict(field.spacing, **field.options))
    if field.direction is not None:
        o.mag, o.direction, o.flats = field.mag.copy(), field.direction.copy(), field.flats.astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    return o


def out_degree(o):
    return np.diff(o.A[0]).reshape(o.elev.shape)


def pit_edges_kept(o):
    """(pit cell, its destinations in o.A): a drained pit loses its facet edges, so every out-edge it has is a pit edge"""
    indptr, indices, _ = o.A
    pits = np.unique(o.pit_i)
    return [(int(p), indices[indptr[p]:indptr[p + 1]].astype(np.int64)) for p in pits]
