"""Small tiles whose edge fix-up cascades are wider than one workgroup: two 128 x 6000 ridges, the round programs run on
them, the oracle's plain rounds of every program (computed once per process and shared) and the frontier widths of every
round.  A cascade's frontier grows by at most two cells per level, so only a long, thin tile gets a frontier past the
one-workgroup caps of csrc/uca_edge.hip (4096 cells in the classic and the cell-indexed form, 1024 records in the compact
one) with fewer than a million cells.  tests/test_edge_terrain.py holds the recipe to the widths the GPU tests rest on;
tests/test_gpu_edge_forms.py runs the programs on the device."""
import functools
import warnings

import numpy as np

SHAPE = (128, 6000)
SIDES = {'left': (slice(None), 0), 'right': (slice(None), -1), 'top': (0, slice(None)), 'bottom': (-1, slice(None))}
KEYS = tuple(SIDES)
SMALL_CAP = 4096        # k_edge_small / k_einc_small hold a frontier of up to this many cells
CINC_CAP = 1024         # k_cinc_small walks frontiers of up to this many records


@functools.lru_cache(maxsize=None)
def terrain(name):
    """(Shared, read-only.)  ridge_smooth: a plane falling away from row 0 and from column 3000 under 2 mm of noise, so that every cell drains
    from the top line and nothing is finished after the first pass.  ridge_rough: the same with a rough band (pits, pit ->
    drain edges, flats) and a band of terraces (rounded to whole metres) across the flow."""
    n, m = SHAPE
    rng = np.random.default_rng(1)
    row = np.arange(n, dtype=np.float64)[:, None]
    col = np.arange(m, dtype=np.float64)[None, :]
    z = 500 - 1.5 * row - 0.004 * abs(col - 3000) + rng.normal(0, 0.002, (n, m))
    if name == 'ridge_rough':
        z[30:60, 1500:4500] += rng.normal(0, 1.2, (30, 3000))
        z[70:90, 2000:4000] = np.rint(z[70:90, 2000:4000])
    elif name != 'ridge_smooth':
        raise KeyError(name)
    z.setflags(write=False)
    return z


def _cols(*ranges):
    a = np.zeros(SHAPE[1], bool)
    for lo, hi in ranges:
        a[lo:hi] = True
    return a


def _round(top=None, sides=False, everything=False):
    n, m = SHAPE
    if everything:
        return {k: np.ones(n if k in ('left', 'right') else m, bool) for k in KEYS}
    return {'left': np.full(n, sides), 'right': np.full(n, sides), 'top': top, 'bottom': np.zeros(m, bool)}


def program(name):
    """A round program: the `done` masks of the four neighbour strips, round by round."""
    everything = _round(everything=True)
    if name == 'outer2000_then_all':
        return [_round(_cols((0, 1000), (5000, 6000)), sides=True), everything]
    if name == 'inner4200_then_all':
        return [_round(_cols((900, 5100))), everything]
    if name == 'outer5000_then_all':
        return [_round(_cols((0, 2500), (3500, 6000)), sides=True), everything]
    if name == 'all_at_once':
        return [everything]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def first_pass(tname):
    """The oracle's tile after its first pass (graph, areas, masks); shared, never modified."""
    from oracle import oracle as O
    o = O.OracleDEM(terrain(tname), dX=30.0, dY=30.0, drain_pits=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        o.calc_uca()
    for a in (o.uca, o.edge_todo, o.edge_done, o.elev, o.flats):
        a.setflags(write=False)
    return o


def strip_values(tname, nan_at=None):
    """What the neighbours hold: distinct from the tile's own areas everywhere, so a seed that is not taken shows."""
    o = first_pass(tname)
    value = {k: np.nan_to_num(o.uca[sl], nan=900.0) + 1000.0 for k, sl in SIDES.items()}
    if nan_at is not None:
        value['top'][nan_at] = np.nan
    return value


def downstream(A, seeds):
    """The cells the water of `seeds` (bool, tile-shaped) reaches in the flow graph A, the seeds included."""
    indptr, indices, _ = A
    reached = np.ascontiguousarray(seeds).ravel().copy()
    front = np.flatnonzero(reached)
    while front.size:
        cnt = indptr[front + 1] - indptr[front]
        at = np.repeat(indptr[front] - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(cnt.sum())
        tgt = np.unique(indices[at])
        front = tgt[~reached[tgt]]
        reached[front] = True
    return reached.reshape(np.shape(seeds))


def level_widths(A, newly, seeds=None):
    """Kahn levels of the cells of `newly` (bool, tile-shaped) in the flow graph A = (indptr, indices, data) by source
    cell, counting only edges inside the set: the widths of the levels in which a cascade finishes these cells.  Cells of
    `seeds` receive nothing (a finished cell on the tile's edge never does): they are level 0 whatever flows into them."""
    indptr, indices, _ = A
    inset = np.ascontiguousarray(newly).ravel()
    src = np.repeat(np.arange(inset.size), np.diff(indptr))
    keep = inset[src] & inset[indices]
    if seeds is not None:
        keep &= ~np.ascontiguousarray(seeds).ravel()[indices]
    src, dst = src[keep], indices[keep]
    indeg = np.bincount(dst, minlength=inset.size)
    order = np.argsort(src, kind='stable')
    dst = dst[order]
    ptr = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=inset.size))))
    front = np.flatnonzero(inset & (indeg == 0))
    widths, seen = [], 0
    while front.size:
        widths.append(int(front.size))
        seen += front.size
        cnt = ptr[front + 1] - ptr[front]
        at = np.repeat(ptr[front] - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(cnt.sum())
        tgt = dst[at]
        np.subtract.at(indeg, tgt, 1)
        tgt = np.unique(tgt)
        front = tgt[indeg[tgt] == 0]
    assert seen == int(inset.sum()), "the newly finished cells do not form a DAG"
    return widths


def perimeter():
    p = np.zeros(SHAPE, bool)
    for sl in SIDES.values():
        p[sl] = True
    return p


def interior_widths(A, newly):
    """Frontier widths of the condensed form's interior cascade (the catch-up): the rounds have finished the watched cells
    -- here the perimeter -- on the condensed graph, so all of them that are newly done start the cascade together at
    level 0 and are never entered again; the levels after it hold interior cells only."""
    return level_widths(A, newly, newly & perimeter())


def operator_entries(tname):
    """About how many entries the vectors of the condensed operator hold after the first pass: for every unfinished cell
    the span of bottom-line columns its water reaches first (on these ridges the water of a cell fans out over a
    contiguous stretch of the bottom line; the few cells that also reach a side column are left out).  The device build
    keeps these vectors in a merge pool of 16 x (records + 16384) entries and gives up when it is full."""
    o = first_pass(tname)
    indptr, indices, _ = o.A
    m = SHAPE[1]
    NN = indptr.size - 1
    nd = ~o.edge_done.ravel()
    watched = nd & perimeter().ravel()
    src = np.repeat(np.arange(NN), np.diff(indptr))
    keep = nd[src] & nd[indices]
    src, dst = src[keep], indices[keep]
    left = np.bincount(src, minlength=NN)
    order = np.argsort(dst, kind='stable')
    by_dst = src[order]
    ptr = np.concatenate(([0], np.cumsum(np.bincount(dst, minlength=NN))))
    lo, hi = np.full(NN, NN, np.int64), np.full(NN, -1, np.int64)
    front = np.flatnonzero(nd & (left == 0))
    while front.size:                                   # from the outlets upstream: a watched cell ends the path
        tl, th = np.where(watched[front], front, lo[front]), np.where(watched[front], front, hi[front])
        cnt = ptr[front + 1] - ptr[front]
        at = np.repeat(ptr[front] - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(cnt.sum())
        p = by_dst[at]
        np.minimum.at(lo, p, np.repeat(tl, cnt))
        np.maximum.at(hi, p, np.repeat(th, cnt))
        np.subtract.at(left, p, 1)
        p = np.unique(p)
        front = p[left[p] == 0]
    one_line = nd & (hi >= 0) & (hi // m == lo // m)
    return int((hi - lo + 1)[one_line].sum()), int(nd.sum())


class Round(object):
    """One round of a program: what goes to the device (value, done, todo), what the oracle's plain round makes of it
    (uca, edge_todo, edge_done; todo_oracle is its 'todo' input under the pool rule) and the frontier widths: `widths` of
    the cascade that finishes cells (the incremental forms), `sweep_widths` of the classic round's sweep, which also
    carries partial sums to the cells below the seeds that stay unfinished; `inlets` counts the cells its floods start
    from; `interior_widths` of the condensed form's catch-up after this round, see interior_widths()."""
    __slots__ = ('value', 'done', 'todo', 'todo_oracle', 'uca', 'edge_todo', 'edge_done', 'widths', 'sweep_widths', 'inlets',
                 'interior_widths')


@functools.lru_cache(maxsize=None)
def oracle_rounds(tname, pname, nan_at=None):
    """The oracle's plain rounds of program `pname` on terrain `tname`, with the pool schedule's seed rule (a not-done
    edge cell adopts a finished neighbour value: todo | (done & ~edge_done)); shared, never modified."""
    from oracle import oracle as O
    o = first_pass(tname)
    value = strip_values(tname, nan_at)
    uca, todo, done = o.uca, o.edge_todo, o.edge_done
    out = []
    for dn in program(pname):
        r = Round()
        r.value, r.done = value, dn
        r.todo = {k: todo[sl].copy() for k, sl in SIDES.items()}
        r.todo_oracle = {k: r.todo[k] | (dn[k] & ~done[sl]) for k, sl in SIDES.items()}
        uca, todo, done_new = O.uca_update(o.elev, o.flats, o.A, value, dn, r.todo_oracle, uca)
        r.widths = level_widths(o.A, done_new & ~done)
        r.interior_widths = interior_widths(o.A, done_new & ~done)
        e_done, e_todo = np.zeros(SHAPE, bool), np.zeros(SHAPE, bool)
        for k, sl in SIDES.items():
            e_done[sl] |= dn[k]
            e_todo[sl] |= r.todo_oracle[k]
        seeds = e_done & e_todo
        r.sweep_widths = level_widths(o.A, downstream(o.A, seeds), seeds)
        r.inlets = int(e_todo.sum())
        done = done_new
        r.uca, r.edge_todo, r.edge_done = uca, todo, done
        for a in (uca, todo, done):
            a.setflags(write=False)
        out.append(r)
    return out


def crossings(widths, cap):
    """Levels at which the widths pass `cap`: (upward, downward), each a list of level numbers (the first level on the
    other side).  A cascade that starts above the cap has not crossed it."""
    up = [k for k in range(1, len(widths)) if widths[k - 1] <= cap < widths[k]]
    down = [k for k in range(1, len(widths)) if widths[k - 1] > cap >= widths[k]]
    return up, down


def schedule(widths, cap, batch=16):
    """How a cascade of these widths is shared out between the one-workgroup kernel (frontiers up to `cap`) and the level
    kernels (batches of `batch` levels with one look of the host per batch, csrc/uca_edge.hip edge_wide_levels):
    (levels run by the level kernels, hand-overs with levels run on both sides)."""
    width = lambda r: widths[r] if r < len(widths) else 0
    r, wide, hand, prev = 0, 0, 0, None
    while width(r) > 0:
        r0 = r
        while 0 < width(r) <= cap:
            r += 1
        if r > r0:
            hand += prev == 1
            prev = 0
        r0 = r
        while width(r) > cap:
            r += batch
        if r > r0:
            wide += r - r0
            hand += prev == 0
            prev = 1
    return wide, hand


def least_handovers(widths, cap):
    """Hand-overs the cascade has however many levels (up to 32) the host launches per look."""
    return min(schedule(widths, cap, batch)[1] for batch in range(1, 33))
