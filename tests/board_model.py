"""The edge board of pydem_amd/csrc/comm.hip without a mosaic: hand-made tiles, the manager's own rule functions called on them,
and the board layout / descriptors the manager would build.

Nothing here restates a strip rule: `StubManager` only supplies what `ProcessManager._edge_inputs`, `_todo_dropped`,
`_adopt_finished`, `_tile_metric` (and the two request lists) read, and those functions are called unbound on it.  What IS
restated, because the kernels define it: the strip hash (`strip_hash`) and -- from the host wave loop of
`_process_uca_edges_pool_device` -- the schedule (`ScheduleModel`).

  SparseTile      a tile that only holds the lines somebody reads (rows and columns kept equal where they cross)
  StubManager     neighbour table -> `_edge_line`, `tiles_shape`, `grid_slice`, `edge_data`, `check_1overlap`
  BoardPlan       line layout, offsets28 / flags8, readers, side neighbours, snapshots, the board as doubles
  expected_scalars / strip_hash / ScheduleModel
  mosaic / eval_cases / schedule_cases   the designed inputs shared by the CPU and the GPU tier
"""
import functools

import numpy as np

from pydem_amd.process_manager import CORNERS, SIDES, ProcessManager

OWN = {'left': (1, 0), 'right': (1, -1), 'top': (0, 0), 'bottom': (0, -1)}
MASKS = ('edge_done', 'edge_todo')
FAR = 10 ** 9              # a tile index no mosaic has: the all-finished neighbour of `_count_todo`


# ------------------------------------------------------------------------------------------------ tiles
class SparseTile(object):
    """A tile of shape (n, m) known only by its lines: (name, axis, index) -> 1-D array, axis 0 = row `index` (m values),
    axis 1 = column `index` (n values); negative indices count from the end and name the same line."""

    def __init__(self, shape):
        self.shape = (int(shape[0]), int(shape[1]))
        self.lines = {}

    def norm(self, axis, index):
        lim = self.shape[0] if axis == 0 else self.shape[1]
        j = index + lim if index < 0 else index
        assert 0 <= j < lim, (self.shape, axis, index)
        return j

    def line(self, name, axis, index):
        key = (name, axis, self.norm(axis, index))
        if key not in self.lines:
            length = self.shape[1] if axis == 0 else self.shape[0]
            self.lines[key] = np.zeros(length, np.float64 if name == 'uca' else bool)
        return self.lines[key]

    def set_cell(self, name, r, c, value):
        """the cell (r, c) in every line that runs through it"""
        r, c = self.norm(0, r), self.norm(1, c)
        hit = 0
        for (nm, axis, j), arr in self.lines.items():
            if nm == name and axis == 0 and j == r:
                arr[c] = value; hit += 1
            if nm == name and axis == 1 and j == c:
                arr[r] = value; hit += 1
        assert hit, "no line of %s through (%d, %d)" % (name, r, c)

    def set_line(self, name, axis, index, value):
        """one value along a whole line, also where other lines cross it"""
        j = self.norm(axis, index)
        for p in range(self.shape[1] if axis == 0 else self.shape[0]):
            self.set_cell(name, j if axis == 0 else p, p if axis == 0 else j, value)

    def reconcile(self):
        """where a row and a column cross they hold one cell: the row's value"""
        for (nm, axis, r), row in self.lines.items():
            if axis != 0:
                continue
            for (nm2, axis2, c), col in self.lines.items():
                if axis2 == 1 and nm2 == nm:
                    col[r] = row[c]

    def generate(self, fn, *args):
        """every line from a function of the cells: fn(name, rows, cols, *args) -> values"""
        n, m = self.shape
        for (nm, axis, j), arr in self.lines.items():
            rows = np.full(m, j) if axis == 0 else np.arange(n)
            cols = np.arange(m) if axis == 0 else np.full(n, j)
            arr[:] = fn(nm, rows, cols, *args)

    def copy(self):
        t = SparseTile(self.shape)
        t.lines = {k: v.copy() for k, v in self.lines.items()}
        return t


# ------------------------------------------------------------------------------------------------ the manager, hand-made
class StubManager(object):
    """What the manager's rule functions read, from a neighbour table.

    shapes: [(n, m)] per tile.  table[i][side] is None (no neighbour: the mosaic has a hole), 'self' (the edge table points
    the tile at its own line: the mosaic border) or (tile, axis, index); table[i][corner] is None or (tile, row, col, one_overlap).
    `grid_slice[i]` and `edge_data[i][key]` are only ever handed back to `check_1overlap`, so they carry its answer."""

    def __init__(self, shapes, table):
        self.tiles_shape = [(int(n), int(m)) for n, m in shapes]
        self.n_inputs = len(self.tiles_shape)
        self.grid_slice = list(range(self.n_inputs))
        self.edge_data = []
        self._where = []
        for i in range(self.n_inputs):
            where, ov = {}, {}
            for key in SIDES:
                e = table[i].get(key)
                if e is None:
                    where[key] = (-1, OWN[key][0], 0)
                elif e == 'self':
                    where[key] = (i,) + OWN[key]
                else:
                    where[key] = (int(e[0]), int(e[1]), int(e[2]))
                ov[key] = False
            for key in CORNERS:
                e = table[i].get(key)
                where[key] = (-1, 0, 0) if e is None else (int(e[0]), int(e[1]), int(e[2]))
                ov[key] = bool(e[3]) if e is not None else False
            self._where.append(where)
            self.edge_data.append(ov)
        for i in range(self.n_inputs):                    # a strip and the line it reads are equally long
            n, m = self.tiles_shape[i]
            for key in SIDES:
                src, axis, idx = self._where[i][key]
                if src >= 0:
                    assert axis in (0, 1) and self.tiles_shape[src][0 if axis == 1 else 1] == (n if key in ('left', 'right') else m), (i, key, src)
                    lim = self.tiles_shape[src][0 if axis == 0 else 1]
                    assert -lim <= idx < lim, (i, key)
            for key in CORNERS:
                src, r, c = self._where[i][key]
                if src >= 0:
                    assert 0 <= r < self.tiles_shape[src][0] and 0 <= c < self.tiles_shape[src][1], (i, key)

    @classmethod
    def from_manager(cls, pm):
        """the edge table of a real manager (after `_edge_setup`), so that the stub can be held against it"""
        self = cls.__new__(cls)
        self.tiles_shape = [tuple(s) for s in pm.tiles_shape]
        self.n_inputs = pm.n_inputs
        self.grid_slice = list(range(pm.n_inputs))
        self._where = [{key: tuple(int(v) for v in pm._edge_line(i, key)) for key in SIDES + CORNERS} for i in range(pm.n_inputs)]
        self.edge_data = [{key: bool(pm.check_1overlap(pm.grid_slice[i], pm.edge_data[i][key])) for key in SIDES + CORNERS}
                          for i in range(pm.n_inputs)]
        return self

    def _edge_line(self, i, key):
        return self._where[i][key]

    @staticmethod
    def check_1overlap(out_slice, edge_slc):
        return bool(edge_slc)

    def side_neighbours(self, i):
        """tile i and the tiles its four sides read (what `_neighbours` is on a full grid)"""
        return sorted(set([i] + [self._where[i][key][0] for key in SIDES if self._where[i][key][0] >= 0]))


class _AllFinished(object):
    """the same tile with every neighbour cell finished: `_tile_metric` then counts the 'todo' cells (its denominator)"""

    def __init__(self, stub):
        self.stub = stub

    def _edge_line(self, i, key):
        return (FAR, OWN[key][0], 0) if key in SIDES else (FAR, 0, 0)


def _count_todo(stub, i, snap):
    n, m = stub.tiles_shape[i]
    s2 = {k: v for k, v in snap.items() if k[0] == i}
    s2[(FAR, 'edge_done', 0, 0)] = np.ones(m, bool)
    s2[(FAR, 'edge_done', 1, 0)] = np.ones(n, bool)
    return int(ProcessManager._tile_metric(_AllFinished(stub), i, s2)[1])


# ------------------------------------------------------------------------------------------------ layout and descriptors
class BoardPlan(object):
    """The line layout and the descriptors, built as `_process_uca_edges_pool_device` builds them."""

    def __init__(self, stub, shuffle=None):
        """shuffle: a seed; the lines of a tile then lie on the board in a shuffled order instead of the manager's sorted one"""
        self.stub = stub
        n_t = stub.n_inputs
        interest = {}
        for i in range(n_t):
            for req in ProcessManager._snapshot_requests(stub, i) | ProcessManager._metric_requests(stub, i):
                interest.setdefault(req[0], set()).add(req)
        self.order = {t: sorted(interest.get(t, ())) for t in range(n_t)}
        if shuffle is not None:
            rng = np.random.default_rng(shuffle)
            self.order = {t: [v[k] for k in rng.permutation(len(v))] for t, v in self.order.items()}
        length = lambda req: stub.tiles_shape[req[0]][1] if req[2] == 0 else stub.tiles_shape[req[0]][0]
        self.layout, self.start, self.size, off = {}, {}, {}, 0
        for t in range(n_t):
            self.start[t] = off
            for req in self.order[t]:
                self.layout[req] = off
                off += length(req)
            self.size[t] = off - self.start[t]
        self.total = off
        layout = self.layout
        self.readers = {t: set([t]) for t in range(n_t)}
        self.desc = []
        for i in range(n_t):
            o28, f8 = [], []
            srcs = [stub._edge_line(i, key) for key in SIDES]
            o28 += [layout[(i, 'edge_todo',) + OWN[key]] for key in SIDES]
            o28 += [layout[(i, 'edge_done',) + OWN[key]] for key in SIDES]
            for name in ('uca', 'edge_done', 'edge_todo'):
                o28 += [layout[(src, name, axis, idx)] if src >= 0 else -1 for src, axis, idx in srcs]
            f8 += [int(src == i) for src, _, _ in srcs]
            cd, cu, c1 = [], [], []
            for key in ('top-left', 'top-right', 'bottom-left', 'bottom-right'):
                src, lr, lc = stub._edge_line(i, key)
                ov1 = bool(stub.check_1overlap(stub.grid_slice[i], stub.edge_data[i][key]))
                cd.append(layout[(src, 'edge_done', 0, lr)] + lc if src >= 0 else -1)
                cu.append(layout[(src, 'uca', 0, lr)] + lc if (src >= 0 and ov1) else -1)
                c1.append(int(ov1))
                if src >= 0:
                    self.readers[src].add(i)
            for src, _, _ in srcs:
                if src >= 0:
                    self.readers[src].add(i)
            n, m = stub.tiles_shape[i]
            self.desc.append((n, m, o28 + cd + cu, f8 + c1))
            # nothing the evaluation kernel reads may lie beyond the board
            for k in range(20):
                assert o28[k] == -1 or 0 <= o28[k] and o28[k] + (n if k % 4 < 2 else m) <= self.total, (i, k)
            assert all(-1 <= v < self.total for v in cd + cu), i
        self.nbrs = {t: set(stub.side_neighbours(t)) for t in range(n_t)}

    def lines_of(self, t):
        """[(name, axis, index, offset relative to the tile's segment)] in the order of `set_lines`"""
        return [(req[1], req[2], req[3], self.layout[req] - self.start[t]) for req in self.order[t]]

    def register(self, tiles):
        """make every line of the layout exist on the hand-made tiles"""
        for req in self.layout:
            tiles[req[0]].line(req[1], req[2], req[3])

    def snap(self, tiles):
        """the dict of lines the rule functions read (the manager's `_edge_lines`): areas as float64, masks as bool"""
        return {req: tiles[req[0]].line(req[1], req[2], req[3]) for req in self.layout}

    def board(self, tiles):
        """the board as the device holds it: masks as 0.0 / 1.0"""
        out = np.zeros(self.total, np.float64)
        for req, off in self.layout.items():
            v = tiles[req[0]].line(req[1], req[2], req[3])
            out[off:off + v.size] = v
        return out

    def staging(self):
        """byte offset of every line in the staging buffer of the queued waves (pydem_board_prepare_waves): tiles in index
        order, lines in `set_lines` order, areas as doubles, masks as bytes, every line padded to 8 bytes"""
        st, out = 0, {}
        for t in range(self.stub.n_inputs):
            for req in self.order[t]:
                out[req] = st
                count = self.stub.tiles_shape[t][1] if req[2] == 0 else self.stub.tiles_shape[t][0]
                st += (count * (8 if req[1] == 'uca' else 1) + 7) & ~7
        return out, st


# ------------------------------------------------------------------------------------------------ the numbers of one evaluation


def mix64(x):
    x = x.astype(np.uint64)
    with np.errstate(over='ignore'):
        x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xff51afd7ed558ccd)
        x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xc4ceb9fe1a85ec53)
        x = x ^ (x >> np.uint64(33))
    return x


def _cat(v):
    if isinstance(v, dict):
        v = [v[k] for k in SIDES]
    if isinstance(v, (list, tuple)):
        return np.concatenate([np.asarray(a) for a in v])
    return np.asarray(v)


def strip_hash(n, m, data, done, todo_adopt):
    """The hash k_board_eval forms of a tile's strips, bit for bit: the sum over q (left n, right n, top m, bottom m) of
    mix64(bits(done ? data : 0.0) ^ q * 0x9E3779B97F4A7C15 ^ done << 1 ^ todo_adopt), in wrapping 64-bit arithmetic."""
    data = np.ascontiguousarray(_cat(data), np.float64)
    done = _cat(done).astype(bool)
    tda = _cat(todo_adopt).astype(bool)
    assert data.size == done.size == tda.size == 2 * n + 2 * m
    bits = np.where(done, data.view(np.uint64), np.uint64(0))          # (selects bit patterns: -0.0 and NaN keep theirs)
    q = np.arange(data.size, dtype=np.uint64)
    with np.errstate(over='ignore'):
        h = mix64(bits ^ (q * np.uint64(0x9E3779B97F4A7C15)) ^ (done.astype(np.uint64) << np.uint64(1)) ^ tda.astype(np.uint64))
        return int(np.add.reduce(h, dtype=np.uint64))


def expected_scalars(stub, i, snap, full):
    """[n_done, p_done, dropped_self, dropped_full, seeds, hash] of tile i as `check_against_host_rules` forms them; with
    full = 1 the strips (seeds, hash) are those of rule :274 applied everywhere."""
    PM = ProcessManager
    met = PM._tile_metric(stub, i, snap)
    d0, dn0, td0 = PM._edge_inputs(stub, i, snap, drop_mutual_todo='self')
    d1, dn1, td1 = PM._edge_inputs(stub, i, snap, drop_mutual_todo=True)
    dropped_self = PM._todo_dropped(stub, i, snap, td0)
    dropped_full = PM._todo_dropped(stub, i, snap, td1)
    data, done, todo = (d1, dn1, td1) if full else (d0, dn0, td0)
    tda = PM._adopt_finished(stub, i, snap, done, todo)
    seeds = sum(int(np.count_nonzero(done[k] & tda[k])) for k in SIDES)
    n, m = stub.tiles_shape[i]
    return [int(met[1]), _count_todo(stub, i, snap), int(dropped_self), int(dropped_full), seeds, strip_hash(n, m, data, done, tda)]


# ------------------------------------------------------------------------------------------------ the schedule
class ScheduleModel(object):
    """The wave loop of `_process_uca_edges_pool_device` for a pool at least as wide as the mosaic (every candidate runs),
    in batches like `pydem_board_run_waves`; the tiles' rounds are played by `script(tile_object, tile_index, times_run)`,
    which rewrites the tile's lines."""

    def __init__(self, plan, tiles, script):
        self.plan, self.stub, self.script = plan, plan.stub, script
        self.tiles = [t.copy() for t in tiles]
        self.n_t = self.stub.n_inputs
        self.runs = [0] * self.n_t
        snap = plan.snap(self.tiles)
        self.scal = [expected_scalars(self.stub, a, snap, 0) for a in range(self.n_t)]
        self.nd = [s[0] for s in self.scal]           # the metric as the schedule carries it
        self.pd = [s[1] for s in self.scal]
        self.last_hash = {}
        self.events = set()
        self.history = []                             # (members, tie-break) of every wave so far

    def candidates(self):
        return [a for a in range(self.n_t)
                if (self.nd[a] > 0 or self.scal[a][2] != 0) and self.last_hash.get(a) != self.scal[a][5]]

    def batch(self, k_waves, ok, limit):
        """up to k_waves waves; returns (n_waves, stop, log, n_tiebreaks, tiebreak bits)"""
        limit = min(limit, k_waves)
        log, ntb, tblog, stop, check = [], 0, 0, 0, set()
        for _ in range(k_waves):
            for a in check:                           # the tiles that ran and their side neighbours; a diagonal one keeps its numbers
                self.nd[a], self.pd[a] = self.scal[a][0], self.scal[a][1]
            check = set()
            if len(log) >= limit:
                stop = 3
                break
            for a in range(self.n_t):
                if (self.nd[a] > 0 or self.scal[a][2] != 0) and self.last_hash.get(a) == self.scal[a][5]:
                    self.events.add('suppressed')
                if self.nd[a] != self.scal[a][0]:
                    self.events.add('stale diagonal')
            wave, tb = self.candidates(), False
            if not wave:
                drops = [s[3] for s in self.scal]
                if max(drops) <= 0:
                    stop = 1
                    break
                wave, tb = [drops.index(max(drops))], True        # the most dropped pixels, lowest index first
            if any(not (ok >> a) & 1 for a in wave):
                stop = 2
                break
            for a in wave:
                if tb:
                    self.last_hash.pop(a, None)
                else:
                    self.last_hash[a] = self.scal[a][5]
                self.script(self.tiles[a], a, self.runs[a])
                self.runs[a] += 1
            if tb:
                tblog |= 1 << len(log); ntb += 1
            elif self.history and self.history[-1][1] and self.history[-1][0][0] in wave:
                self.events.add('tie-break then normal')
            if len(wave) >= 3:
                self.events.add('wide wave')
            affected = set()
            for a in wave:
                affected |= self.plan.readers[a]
                check |= self.plan.nbrs[a]
            snap = self.plan.snap(self.tiles)
            for a in sorted(affected):
                self.scal[a] = expected_scalars(self.stub, a, snap, 0)
            log.append(sum(1 << a for a in wave))
            self.history.append((wave, tb))
        for a in check:
            self.nd[a], self.pd[a] = self.scal[a][0], self.scal[a][1]
        if any(self.nd[a] != self.scal[a][0] or self.pd[a] != self.scal[a][1] for a in range(self.n_t)):
            self.events.add('stale at the end of a batch')       # (k_sched_settle must leave such a tile its old numbers)
        self.events.add('stop %d' % stop)
        if stop == 0 and len(log) == k_waves:
            self.events.add('full batch')
        return len(log), stop, log, ntb, tblog


# ------------------------------------------------------------------------------------------------ designed inputs
def mosaic(heights, widths, depth=1, border='self', one_overlap=True, holes=()):
    """A grid of len(heights) x len(widths) tiles, tile (r, c) of shape (heights[r], widths[c]), numbered row by row.  A side
    reads the neighbour's line `depth` cells inside it; at the mosaic border it reads its own line (border='self') or nothing;
    a corner reads the diagonal tile's pixel (with the one-overlap flag) or, at the border, a pixel of the tile itself.
    holes: tile numbers that are missing (their neighbours read nothing there; the tile stays in the list, unread)."""
    R, C = len(heights), len(widths)
    d = depth
    shapes, table = [], []
    num = lambda r, c: r * C + c
    for r in range(R):
        for c in range(C):
            n, m = heights[r], widths[c]
            shapes.append((n, m))
            e = {}
            for key, (dr, dc) in (('left', (0, -1)), ('right', (0, 1)), ('top', (-1, 0)), ('bottom', (1, 0))):
                rr, cc = r + dr, c + dc
                if not (0 <= rr < R and 0 <= cc < C):
                    e[key] = 'self' if border == 'self' else None
                elif num(rr, cc) in holes:
                    e[key] = None
                else:
                    axis = OWN[key][0]
                    lim = widths[cc] if axis == 1 else heights[rr]
                    dd = min(d, lim)
                    e[key] = (num(rr, cc), axis, -dd if key in ('left', 'top') else dd - 1)
            for key, (dr, dc) in (('top-left', (-1, -1)), ('top-right', (-1, 1)), ('bottom-left', (1, -1)), ('bottom-right', (1, 1))):
                rr, cc = r + dr, c + dc
                if 0 <= rr < R and 0 <= cc < C:
                    if num(rr, cc) in holes:
                        e[key] = None
                    else:
                        hh, ww = heights[rr], widths[cc]
                        e[key] = (num(rr, cc), hh - min(d, hh) if dr < 0 else min(d, hh) - 1, ww - min(d, ww) if dc < 0 else min(d, ww) - 1,
                                  one_overlap)
                elif border == 'self':
                    e[key] = (num(r, c), 0 if dr < 0 else n - 1, 0 if dc < 0 else m - 1, False)
                else:
                    e[key] = None
            table.append(e)
    return shapes, table


_DENSITIES = (0.0, 0.1, 0.5, 0.9, 1.0)


def random_fill(plan, tiles, rng):
    """every line with a mask density of its own; areas with the values a hash must take by their bits"""
    plan.register(tiles)
    for t in tiles:
        for (name, axis, j), arr in sorted(t.lines.items()):
            if name == 'uca':
                arr[:] = rng.uniform(1.0, 1e6, arr.size)
                k = rng.integers(0, 5, arr.size)
                arr[k == 0] = rng.uniform(0.9e15, 1.1e15, int((k == 0).sum()))
                special = np.array([-0.0, np.nan, 5e-324, 2.5e-310, 0.0, 1e15 + 0.125])
                pos = rng.integers(0, arr.size, special.size)
                arr[pos] = special
            else:
                arr[:] = rng.random(arr.size) < _DENSITIES[int(rng.integers(0, len(_DENSITIES)))]
        t.reconcile()


class Case(object):
    def __init__(self, name, shapes, table, seed, design=None):
        self.name = name
        self.stub = StubManager(shapes, table)
        self.plan = BoardPlan(self.stub)
        self.tiles = [SparseTile(s) for s in shapes]
        random_fill(self.plan, self.tiles, np.random.default_rng(seed))
        if design is not None:
            design(self)
        self.evaluate = list(range(len(shapes)))
        self.snap = self.plan.snap(self.tiles)
        self._expected = {}

    def expected(self, full):
        """{tile: the six words} of the tiles the case evaluates (computed once)"""
        if full not in self._expected:
            self._expected[full] = {a: expected_scalars(self.stub, a, self.snap, full) for a in self.evaluate}
        return self._expected[full]


EVAL_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (2, 5), (63, 65), (511, 513), (1024, 1024), (1025, 1024), (5000, 3300), (1, 20000)]

# corner -> (its top / bottom strip, its left / right strip, position on the former, on the latter, (row, col) of the own pixel)
CORNER_OF = {'top-left': ('top', 'left', 0, 0), 'top-right': ('top', 'right', -1, 0),
             'bottom-left': ('bottom', 'left', 0, -1), 'bottom-right': ('bottom', 'right', -1, -1)}


def _nb_cell(case, i, side, pos):
    """(tile, row, col) of the neighbour cell that position `pos` of tile i's `side` strip reads"""
    src, axis, idx = case.stub._edge_line(i, side)
    t = case.tiles[src]
    return (src, pos, t.norm(1, idx)) if axis == 1 else (src, t.norm(0, idx), pos)


def corner_design(strips, diagonal):
    """centre of a 3 x 3 mosaic (tile 4): at every corner the two neighbour cells finished as `strips` = (tb, lr) says and the
    diagonal pixel finished or not; the centre's own corner pixels are 'todo' and not finished"""
    def design(case):
        n, m = case.stub.tiles_shape[4]
        for key, (tb, lr, ptb, plr) in CORNER_OF.items():
            for side, pos, on in ((tb, ptb % m, strips[0]), (lr, plr % n, strips[1])):
                src, r, c = _nb_cell(case, 4, side, pos)
                case.tiles[src].set_cell('edge_done', r, c, on)
            src, r, c = case.stub._edge_line(4, key)
            case.tiles[src].set_cell('edge_done', r, c, diagonal)
            if case.stub.edge_data[4][key]:
                case.tiles[src].set_cell('uca', r, c, 4242.5 + len(key))
    return design


def adoption_design(case):
    """a lone tile that has no 'todo' cell and no finished cell of its own, beside finished neighbour cells"""
    for (name, axis, j), arr in case.tiles[4].lines.items():
        if name in MASKS:
            arr[:] = False
    for side in SIDES:
        src, axis, idx = case.stub._edge_line(4, side)
        case.tiles[src].set_line('edge_done', axis, idx, True)


@functools.lru_cache(maxsize=None)
def eval_cases():
    """The evaluation cases of tests/test_gpu_board_eval.py (their coverage is asserted in tests/test_board_model.py)."""
    cases = []
    for k, (n, m) in enumerate(EVAL_SHAPES):
        small = max(n, m) <= 100
        # the centre of a 3 x 3 neighbourhood: neighbours a few cells thick, lines one or two cells inside them
        for depth, ov in ((1, True), (2, False)) if small else ((1, True),):
            shapes, table = mosaic((3, n, 2), (2, m, 3), depth=depth, one_overlap=ov)
            cases.append(Case('nbhd_%dx%d_d%d' % (n, m, depth), shapes, table, seed=100 + 7 * k + depth))
        shapes, table = mosaic((n,), (m,), border='self')
        cases.append(Case('self_%dx%d' % (n, m), shapes, table, seed=300 + k))
        shapes, table = mosaic((n,), (m,), border='none')
        cases.append(Case('alone_%dx%d' % (n, m), shapes, table, seed=500 + k))
    # the corner hand-over, designed: both strips finished with the diagonal finished / not finished, one strip only
    for n, m in ((2, 5), (1, 1), (1, 7), (7, 1), (3, 1), (1, 2)):
        for strips, diag, tag in (((True, True), True, 'both_diag'), ((True, True), False, 'both_nodiag'),
                                  ((True, False), True, 'tb_only'), ((False, True), True, 'lr_only')):
            for ov in (True, False):
                shapes, table = mosaic((3, n, 2), (2, m, 3), depth=1, one_overlap=ov)
                cases.append(Case('corner_%dx%d_%s_ov%d' % (n, m, tag, ov), shapes, table, seed=700 + n * 31 + m + len(tag),
                                  design=corner_design(strips, diag)))
    # degenerate tiles between a finished and an unfinished neighbour, every combination of the four sides
    for n, m in ((1, 1), (1, 4), (4, 1)):
        for bits in range(16):
            def design(case, bits=bits):
                for b, side in enumerate(SIDES):
                    src, axis, idx = case.stub._edge_line(4, side)
                    case.tiles[src].set_line('edge_done', axis, idx, bool((bits >> b) & 1))
                for key in CORNERS:
                    src, r, c = case.stub._edge_line(4, key)
                    case.tiles[src].set_cell('edge_done', r, c, True)
            shapes, table = mosaic((3, n, 2), (2, m, 3), depth=1, one_overlap=True)
            cases.append(Case('thin_%dx%d_sides%x' % (n, m, bits), shapes, table, seed=900 + bits, design=design))
    shapes, table = mosaic((3, 6, 2), (2, 9, 3), depth=1)
    cases.append(Case('adoption', shapes, table, seed=11, design=adoption_design))
    # a hole beside the centre and a mosaic whose border reads nothing
    shapes, table = mosaic((4, 6, 5), (5, 9, 4), depth=2, border='none', holes=(1, 3, 8))
    cases.append(Case('holes', shapes, table, seed=12))
    return cases


@functools.lru_cache(maxsize=None)
def many_tiles_case():
    """70 small tiles in one board: more than one chunk of 64 in `refresh` and in `pydem_board_eval`"""
    heights = (1, 2, 3, 5, 4, 2, 6)
    widths = (3, 1, 2, 7, 4, 5, 2, 3, 6, 2)
    shapes, table = mosaic(heights, widths, depth=1, one_overlap=True)
    return Case('70_tiles', shapes, table, seed=70)


# ---- scheduler scripts: the contents of every tile's lines as a function of the cell and of the rounds the tile has run ----
def _cell_hash(t, rows, cols, salt):
    x = (np.asarray(rows, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(cols, np.uint64) * np.uint64(0x85EBCA77)
         + np.uint64(t * 0xC2B2AE3D + salt * 0x27D4EB2F + 1))
    return mix64(x)


class Script(object):
    """Monotone rounds: a cell finishes after `finish` rounds of its tile (or never), finished cells stop being 'todo', and
    after last[t] rounds tile t has no 'todo' cell left -- so every schedule ends.  p_todo[t]: how much of tile t starts as
    'todo'."""

    def __init__(self, seed, last, p_todo, p_never=0.3):
        self.seed, self.last, self.p_todo, self.p_never = seed, list(last), list(p_todo), p_never

    def cells(self, t, name, rows, cols, k):
        last = self.last[t]
        h = _cell_hash(t, rows, cols, self.seed)
        u1 = (h & np.uint64(0xFFFF)).astype(np.float64) / 65536.0
        u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.float64) / 65536.0
        finish = ((h >> np.uint64(32)) % np.uint64(last + 1)).astype(np.int64)
        finish[u2 < self.p_never] = 10 ** 6
        todo0 = u1 < self.p_todo[t]
        done = finish <= k
        if name == 'edge_done':
            return done
        if name == 'edge_todo':
            return todo0 & ~done & (k < last)
        return 1.0 + (h % np.uint64(1000)).astype(np.float64) + 0.5 * np.minimum(finish, k)

    def __call__(self, tile, t, times_run):
        """tile t runs its round number `times_run` (from 0)"""
        tile.generate(lambda name, rows, cols: self.cells(t, name, rows, cols, times_run + 1))

    def initial(self, plan, shapes):
        tiles = [SparseTile(s) for s in shapes]
        plan.register(tiles)
        for t, tile in enumerate(tiles):
            tile.generate(lambda name, rows, cols, t=t: self.cells(t, name, rows, cols, 0))
        return tiles


class ScheduleCase(object):
    """A mosaic, a script and the batches to run: [(k_waves, tiles allowed (bit mask), wave limit)], repeated from the last
    entry until the schedule stops with reason 1."""

    def __init__(self, name, heights, widths, script, batches, depth=1, one_overlap=True):
        self.name = name
        shapes, table = mosaic(heights, widths, depth=depth, one_overlap=one_overlap)
        self.shapes = shapes
        self.stub = StubManager(shapes, table)
        self.plan = BoardPlan(self.stub)
        self.script = script
        self.batches = batches
        self.n_t = len(shapes)

    def initial(self):
        return self.script.initial(self.plan, self.shapes)

    def steps(self):
        """the batches, the last one again and again (the caller stops at stop reason 1; at most 400)"""
        for k in range(400):
            yield self.batches[min(k, len(self.batches) - 1)]


@functools.lru_cache(maxsize=None)
def schedule_cases():
    ALL = lambda n: (1 << n) - 1
    cases = []

    def script(seed, n_t):
        # tiles that take 2 to 5 rounds and start with nothing, some or most of their cells 'todo': they fall out of step, so
        # waves of one tile, suppressed candidates and tie-breaks all occur (tests/test_board_model.py asserts which)
        return Script(seed, last=[2 + (seed + 3 * t) % 4 for t in range(n_t)], p_todo=[(0.0, 0.3, 0.6)[(seed // 2 + t) % 3] for t in range(n_t)],
                      p_never=0.4)
    # (k_waves, tiles whose rounds may be queued, wave limit): a batch that stops in front of a tile that may not run, full
    # batches of 1 and 3 waves, wave limits below the schedule's length (also 0), then to the end.  The third batch of the
    # first case ends after the wave that leaves tile 3, a diagonal neighbour of its only member, with a stale metric.
    cases.append(ScheduleCase('2x2', (6, 4), (9, 3), script(10, 4),
                              [(3, ALL(4) & ~8, 64), (3, ALL(4), 64), (16, ALL(4), 1), (1, ALL(4), 64)]))
    cases.append(ScheduleCase('2x3', (2, 40), (3, 60, 7), script(2, 6),
                              [(16, ALL(6) & ~(1 << 4), 64), (16, ALL(6), 5), (1, ALL(6), 0), (16, ALL(6), 64)], depth=2, one_overlap=False))
    cases.append(ScheduleCase('3x3', (5, 11, 2), (7, 12, 3), script(4, 9),
                              [(1, ALL(9), 64), (3, ALL(9) & ~1, 64), (3, ALL(9), 64), (16, ALL(9), 64)]))
    # perimeters of 16 600, 11 400, 8 000 and 2 800 cells: the queued evaluation (ceil(largest perimeter / 1024) blocks per
    # tile, at most 16) runs with 16 blocks, and the threads of tile 0 make a second trip
    cases.append(ScheduleCase('2x2_large', (5000, 700), (3300, 700), script(10, 4), [(16, ALL(4), 64)]))
    return cases
