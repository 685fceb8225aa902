"""Designed graphs for the cyutils boundary (pydem_amd.cyfuncs.cyutils, csrc/cyutils.hip): small generic sparse graphs in the
CSC / CSR form that drain_area / drain_connections take, each built to reach one thing that flow graphs of real terrain seeded
with "cells without in-edges" never reach -- a frontier whose members push into each other (loops and chains seeded at once,
as the reference's stall / re-seed loop does on level ground), the tile-edge rules on chosen cells, a CSR whose rows are
unsorted or list a source twice, a sum of 300 products whose order shows, a frontier wider than one launch of the kernels.

Every case is seeded and deterministic; weights, areas and taints are random doubles so that every sum rounds.  A case is a
dict of the call's arguments plus `expect`: lower bounds on the counters that the model below takes while it runs the case,
i.e. the fact that the case reaches its target (`missed_facts`).

The model is a plain Python restatement of the two Cython loops, written from their semantics: the frontier is walked in
ascending id, each push reads the CURRENT value of its source, `done` is set before a round's pushes, a target whose upstream
cells are all done joins the next frontier, and the loop ends when a round's new frontier equals its old one.  Those loops do
not end on every input (seed ONE member of a two-cell loop and the frontier alternates for ever), so the model stops at
ROUND_CAP rounds and returns None: such an input is not a case, and nothing that the model cannot finish goes to a device or
to compiled code.  `snapshot=True` is the mutant in which every push of a round reads the values of the round's start."""
import numpy as np

ROUND_CAP = 64

AREA_KEYS = ('area', 'done', 'ids', 'edge_todo', 'edge_todo_no_mask')


def on_edge(i, n_rows, n_cols):
    return i < n_cols or i >= n_cols * n_rows - n_cols or i % n_cols == 0 or i % n_cols == n_cols - 1


def csc_from_edges(N, edges):
    """(indptr, indices, data) with one column per source; a column keeps the order in which its edges were listed."""
    src = np.array([e[0] for e in edges], np.int64)
    order = np.argsort(src, kind='stable')
    indptr = np.zeros(N + 1, np.int32)
    indptr[1:] = np.cumsum(np.bincount(src, minlength=N))
    indices = np.array([edges[k][1] for k in order], np.int32)
    data = np.array([edges[k][2] for k in order], np.float64)
    return indptr, indices, data


def csr_of(indptr, indices):
    """The index structure of tocsr(): for every target its sources in ascending order, duplicates kept."""
    N = indptr.size - 1
    col_of = np.repeat(np.arange(N, dtype=np.int32), np.diff(indptr))
    order = np.argsort(indices, kind='stable')
    rp = np.zeros(N + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(indices, minlength=N))
    return rp, col_of[order].astype(np.int32)


# --- the model ------------------------------------------------------------------------------------------------------------

def model_drain_area(case, snapshot=False, cap=ROUND_CAP):
    """-> dict(area, done, ids, edge_todo, edge_todo_no_mask, rounds, stats), or None if `cap` rounds do not end the loop."""
    n_rows, n_cols = case['n_rows'], case['n_cols']
    N = n_rows * n_cols
    cp, ci, cd = case['cp'].tolist(), case['ci'].tolist(), case['cd'].tolist()
    rp, ri = case['rp'].tolist(), case['ri'].tolist()
    skip_edge = case['skip_edge']
    area = case['area'].tolist()
    et = None if case['edge_todo'] is None else case['edge_todo'].tolist()
    etn = None if case['edge_todo_no_mask'] is None else case['edge_todo_no_mask'].tolist()
    done = case['done'].astype(np.uint8)
    cur = case['ids'].astype(np.uint8)
    stats = dict(max_frontier=0, in_frontier=0, dirty_reads=0, edge_skipped=0, edge_received=0, corner_skipped=0,
                 corner_received=0, max_fan_in=0, repeat_rounds=0, pushes=0)
    corners = (0, n_cols - 1, N - n_cols, N - 1)
    for rounds in range(1, cap + 1):
        front = np.flatnonzero(cur).tolist()
        done[front] = 1
        old, cur = cur, np.zeros(N, np.uint8)
        stats['max_frontier'] = max(stats['max_frontier'], len(front))
        src_area, src_et, src_etn = (list(area), et and list(et), etn and list(etn)) if snapshot else (area, et, etn)
        written, fan = set(), {}
        for i in front:
            for j in range(cp[i], cp[i + 1]):
                row, w = ci[j], cd[j]
                if on_edge(row, n_rows, n_cols):
                    skipped = bool(skip_edge or done[row])
                    stats['edge_skipped' if skipped else 'edge_received'] += 1
                    if row in corners:
                        stats['corner_skipped' if skipped else 'corner_received'] += 1
                    if skipped:
                        continue
                stats['pushes'] += 1
                stats['in_frontier'] += int(old[row])
                stats['dirty_reads'] += i in written
                written.add(row)
                fan[row] = fan.get(row, 0) + 1
                area[row] += src_area[i] * w
                if et is not None:
                    et[row] += src_et[i] * w
                if etn is not None:
                    etn[row] += src_etn[i] * w
                if all(done[ri[k]] for k in range(rp[row], rp[row + 1])):
                    cur[row] = 1
        if fan:
            stats['max_fan_in'] = max(stats['max_fan_in'], max(fan.values()))
        stats['repeat_rounds'] += bool((cur & old).any())
        if np.array_equal(cur, old):
            f64 = lambda x: None if x is None else np.array(x, np.float64)
            return dict(area=f64(area), done=done.astype(bool), ids=cur.astype(bool), edge_todo=f64(et),
                        edge_todo_no_mask=f64(etn), rounds=rounds, stats=stats)
    return None


def model_drain_connections(case, cap=ROUND_CAP):
    """-> dict(arr, ids, rounds, stats), or None if `cap` rounds do not end the loop."""
    ip, ix = case['indptr'].tolist(), case['indices'].tolist()
    N = len(ip) - 1
    set_to = int(bool(case['set_to']))
    arr = case['arr'].astype(np.uint8)
    cur = case['ids'].astype(np.uint8)
    stats = dict(max_frontier=0, changed=0, already_set=0)
    for rounds in range(1, cap + 1):
        front = np.flatnonzero(cur).tolist()
        old, cur = cur, np.zeros(N, np.uint8)
        stats['max_frontier'] = max(stats['max_frontier'], len(front))
        for i in front:
            for j in range(ip[i], ip[i + 1]):
                row = ix[j]
                if arr[row] != set_to:
                    cur[row] += 1
                    stats['changed'] += 1
                else:
                    stats['already_set'] += 1
                arr[row] = set_to
        if np.array_equal(cur, old):
            return dict(arr=arr.astype(bool), ids=cur.astype(bool), rounds=rounds, stats=stats)
    return None


def run_model(case, **kw):
    return model_drain_area(case, **kw) if case['kind'] == 'area' else model_drain_connections(case, **kw)


def missed_facts(case, result):
    """The counters of `expect` that the model's run did not reach (empty: the case reaches its target)."""
    if result is None:
        return ['the model does not finish within %d rounds' % ROUND_CAP]
    out = []
    for key, want in case['expect'].items():
        got = result['rounds'] if key == 'rounds' else result['stats'][key]
        ok = got == want[1] if isinstance(want, tuple) else got >= want
        if not ok:
            out.append('%s = %r, wanted %r' % (key, got, want))
    return out


# --- the cases ------------------------------------------------------------------------------------------------------------

def _area_case(shape, edges, ids, seed, done=(), taints=True, skip_edge=0, expect=None):
    """edges: (source, target) pairs, weighted here with seeded random doubles in (0.1, 0.9)"""
    n_rows, n_cols = shape
    N = n_rows * n_cols
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.1, 0.9, len(edges))
    cp, ci, cd = csc_from_edges(N, [(s, t, w[k]) for k, (s, t) in enumerate(edges)])
    rp, ri = csr_of(cp, ci)
    m = lambda cells: np.isin(np.arange(N), list(cells))
    return dict(kind='area', n_rows=n_rows, n_cols=n_cols, cp=cp, ci=ci, cd=cd, rp=rp, ri=ri,
                area=rng.uniform(1.0, 100.0, N), done=m(done) | m(ids), ids=m(ids),
                edge_todo=rng.uniform(0.0, 1.0, N) if taints else None,
                edge_todo_no_mask=rng.uniform(0.0, 1.0, N) if taints else None, skip_edge=skip_edge, expect=expect or {})


def _chain(cells):
    return list(zip(cells[:-1], cells[1:]))


def loop2_plain():
    """two interior cells of a 5 x 5 grid that drain into each other, a tail, both seeded: round numbers, for reading"""
    c = _area_case((5, 5), [(11, 12), (12, 11), (12, 13)], [11, 12], seed=0, taints=False,
                   expect=dict(dirty_reads=2, in_frontier=4, rounds=('==', 2)))
    c['cd'] = np.array([1.0, 0.5, 0.5])
    c['area'] = np.arange(1.0, 26.0)
    c['done'] = c['ids'].copy()
    return c


def loop2_seeded():
    return _area_case((5, 5), [(11, 12), (12, 11), (12, 13)], [11, 12], seed=1,
                      expect=dict(dirty_reads=2, in_frontier=4, repeat_rounds=2))


def loop3_seeded():
    # (2,2) -> (2,3) -> (3,3) -> back to (2,2), and a tail out of (3,3) that runs on for two cells
    return _area_case((6, 6), [(14, 15), (15, 21), (21, 14), (21, 22), (22, 28)], [14, 15, 21], seed=2,
                      expect=dict(dirty_reads=4, in_frontier=6, repeat_rounds=2))


def two_loops():
    a, b, c, d = 2 * 10 + 2, 2 * 10 + 3, 5 * 10 + 6, 6 * 10 + 6
    return _area_case((9, 10), [(a, b), (b, a), (b, 33), (c, d), (d, c), (d, 76), (33, 43), (43, 76)], [a, b, c, d], seed=3,
                      expect=dict(dirty_reads=4, in_frontier=8, repeat_rounds=2))


def _loop_fed_edges():
    # 7 x 7, the loop 24 <-> 25 with the tail 25 -> 32 -> 39; the chain 8 -> 9 -> 16 ends in BOTH loop cells, the shorter
    # chain 36 -> 30 in 24 and the single cell 10 in 25
    return _chain([8, 9, 16, 24]) + [(16, 25)] + _chain([36, 30, 24]) + [(24, 25), (25, 24), (25, 32), (32, 39), (10, 25)]


def loop_fed():
    """the loop 24 <-> 25 is seeded together with the heads of the chains that feed it: both members wait for cell 16, drop out
    of the frontier, take the shorter chain's push meanwhile, and come back together when 16 pushes into both.  (Fed through
    one member only, the loop would re-enter the frontier one cell at a time and the reference would alternate for ever.)"""
    return _area_case((7, 7), _loop_fed_edges(), [8, 36, 10, 24, 25], seed=4,
                      expect=dict(dirty_reads=2, in_frontier=4, repeat_rounds=2, max_fan_in=2, rounds=5))


def chain_up():
    cells = [k * 8 + k for k in range(1, 7)]
    return _area_case((8, 8), _chain(cells), cells, seed=5, expect=dict(dirty_reads=4, in_frontier=5))


def chain_down():
    cells = [k * 8 + k for k in range(6, 0, -1)]
    return _area_case((8, 8), _chain(cells), cells, seed=6, expect=dict(dirty_reads=('==', 0), in_frontier=5, rounds=6))


def edge_rules(skip_edge):
    """6 x 7: the interior cells 8 and 33 and the edge cell 3 are seeded.  8 pushes into the corner 0, the top-edge cell 1,
    the left-edge cell 7 (done) and the interior; 33 into the corner 41 (done), the bottom-edge cell 40, the right-edge cell
    34 (done) and the interior; the edge cells that take a push pass it on, one of them to another edge cell."""
    edges = [(8, 0), (8, 1), (8, 7), (8, 16), (33, 41), (33, 40), (33, 34), (33, 25), (3, 10), (1, 9), (1, 2), (40, 32),
             (0, 15), (16, 15), (25, 24), (24, 21), (7, 15)]
    exp = dict(edge_skipped=7, corner_skipped=2, edge_received=('==', 0)) if skip_edge else \
        dict(edge_skipped=3, edge_received=4, corner_skipped=1, corner_received=1)
    return _area_case((6, 7), edges, [8, 33, 3], seed=7, done=[7, 41, 34], skip_edge=skip_edge, expect=exp)


def edge_line(shape, skip_edge):
    """1 x 9 or 9 x 1: every cell is on the edge.  0 -> 1 -> 2 -> 3 and 6 -> 5 -> 4 (done) -> 3"""
    exp = dict(edge_skipped=2, edge_received=('==', 0)) if skip_edge else dict(edge_skipped=1, edge_received=4)
    return _area_case(shape, _chain([0, 1, 2, 3]) + _chain([6, 5, 4, 3]), [0, 6], seed=8 + shape[0], done=[4],
                      skip_edge=skip_edge, expect=exp)


FAN_IN_SEED = 12          # (9, 10, 11: numpy adds the 300 products to the same double in either order)


def fan_in_300(taints):
    """18 x 18: the first 300 cells but the target are seeded and push into the interior cell 9 * 18 + 9 in one round; the
    target passes its sum on to a cell that is no source"""
    t = 9 * 18 + 9
    src = [i for i in range(18 * 18) if i != t][:300]
    return _area_case((18, 18), [(s, t) for s in src] + [(t, 16 * 18 + 14)], src, seed=FAN_IN_SEED, taints=taints,
                      expect=dict(max_fan_in=('==', 300), dirty_reads=('==', 0), in_frontier=('==', 0)))


def fan_in_products(case):
    """the 300 products that fan_in_300 adds into its target, in ascending source order"""
    t = 9 * 18 + 9
    src = np.flatnonzero(case['ids'])
    assert np.array_equal(case['ci'][case['cp'][src]], np.full(300, t))
    return case['area'][src] * case['cd'][case['cp'][src]]


def csr_unsorted():
    c = loop_fed()
    rng = np.random.default_rng(10)
    ri = c['ri'].copy()
    for r in range(c['n_rows'] * c['n_cols']):
        a, b = c['rp'][r], c['rp'][r + 1]
        if b - a > 1:
            ri[a:b] = ri[a:b][::-1] if b - a == 2 else np.roll(rng.permutation(ri[a:b]), 1)
    assert any((np.diff(ri[c['rp'][r]:c['rp'][r + 1]]) < 0).any() for r in range(49))
    c['ri'] = ri
    return c


def csr_duplicates():
    """6 x 6: the column of 14 lists the target 21 twice and the column of 9 lists 14 twice, with different weights; 21 also
    takes a push from 20 in the round in which 14 pushes: the chains 8 -> 9 -> 14 and 18 -> 19 -> 20 are equally long"""
    edges = [(8, 9), (9, 14), (9, 15), (9, 14), (14, 21), (14, 22), (14, 21), (18, 19), (19, 20), (13, 20), (20, 21), (21, 27)]
    c = _area_case((6, 6), edges, [8, 18, 13], seed=11, expect=dict(max_fan_in=3, dirty_reads=('==', 0)))
    assert np.array_equal(c['ri'][c['rp'][21]:c['rp'][22]], [14, 14, 20])
    return c


WIDE_SHAPE = (2050, 512)
WIDE_FRONTIER = 1025 * 512            # 524 800; one launch of the kernels covers 2048 * 256 = 524 288 entries


def _wide_graph():
    N = WIDE_SHAPE[0] * WIDE_SHAPE[1]
    src = np.arange(WIDE_FRONTIER, dtype=np.int32)
    cp = np.concatenate([np.arange(WIDE_FRONTIER + 1), np.full(N - WIDE_FRONTIER, WIDE_FRONTIER)]).astype(np.int32)
    rp = np.concatenate([np.zeros(WIDE_FRONTIER + 1), np.arange(1, WIDE_FRONTIER + 1)]).astype(np.int32)
    return N, cp, src + WIDE_FRONTIER, rp, src


def wide_frontier():
    """2050 x 512: the upper 1025 rows are seeded and every seeded cell pushes into the cell 1025 rows below it"""
    N, cp, ci, rp, ri = _wide_graph()
    rng = np.random.default_rng(12)
    ids = np.arange(N) < WIDE_FRONTIER
    return dict(kind='area', n_rows=WIDE_SHAPE[0], n_cols=WIDE_SHAPE[1], cp=cp, ci=ci, cd=rng.uniform(0.1, 0.9, WIDE_FRONTIER),
                rp=rp, ri=ri, area=rng.uniform(1.0, 100.0, N), done=ids.copy(), ids=ids, edge_todo=rng.uniform(0.0, 1.0, N),
                edge_todo_no_mask=rng.uniform(0.0, 1.0, N), skip_edge=0,
                expect=dict(max_frontier=('==', WIDE_FRONTIER), pushes=('==', WIDE_FRONTIER), in_frontier=('==', 0),
                            dirty_reads=('==', 0), rounds=('==', 3)))


def _conn_case(N, edges, ids, seed, set_to, preset=(), expect=None):
    indptr, indices, _ = csc_from_edges(N, [(s, t, 0.0) for s, t in edges])
    rng = np.random.default_rng(seed)
    arr = np.full(N, not set_to)
    arr[rng.random(N) < 0.2] = set_to
    touched = np.unique(np.array(edges).ravel())
    arr[touched] = not set_to
    arr[list(preset)] = set_to
    return dict(kind='conn', arr=arr, ids=np.isin(np.arange(N), list(ids)), indptr=indptr, indices=indices, set_to=set_to,
                expect=expect or {})


def conn_cycles(set_to):
    """36 cells: the seed 14 sits on the loop 14 -> 15 -> 21 -> 14, which sheds a tail; a second loop 3 <-> 4 is seeded on both
    members; the seed 30 pushes into 31, which is set already and passes nothing on to 32"""
    edges = [(14, 15), (15, 21), (21, 14), (21, 22), (22, 28), (3, 4), (4, 3), (4, 10), (30, 31), (31, 32)]
    return _conn_case(36, edges, [14, 3, 4, 30], seed=13 + int(set_to), set_to=set_to, preset=[31],
                      expect=dict(changed=8, already_set=3, rounds=4))


def conn_wide():
    N, cp, ci, _, _ = _wide_graph()
    rng = np.random.default_rng(15)
    return dict(kind='conn', arr=rng.random(N) < 0.5, ids=np.arange(N) < WIDE_FRONTIER, indptr=cp, indices=ci, set_to=True,
                expect=dict(max_frontier=('==', WIDE_FRONTIER), changed=200000, already_set=200000))


CASES = {
    'loop2_plain': loop2_plain,
    'loop2_seeded': loop2_seeded,
    'loop3_seeded': loop3_seeded,
    'two_loops': two_loops,
    'loop_fed': loop_fed,
    'chain_up': chain_up,
    'chain_down': chain_down,
    'edge_rules_skip0': lambda: edge_rules(0),
    'edge_rules_skip1': lambda: edge_rules(1),
    'edge_rules_1x9_skip0': lambda: edge_line((1, 9), 0),
    'edge_rules_1x9_skip1': lambda: edge_line((1, 9), 1),
    'edge_rules_9x1_skip0': lambda: edge_line((9, 1), 0),
    'edge_rules_9x1_skip1': lambda: edge_line((9, 1), 1),
    'fan_in_300_taints': lambda: fan_in_300(True),
    'fan_in_300_plain': lambda: fan_in_300(False),
    'csr_unsorted': csr_unsorted,
    'csr_duplicates': csr_duplicates,
    'wide_frontier': wide_frontier,
    'conn_cycles_set0': lambda: conn_cycles(False),
    'conn_cycles_set1': lambda: conn_cycles(True),
    'conn_wide': conn_wide,
}
LARGE = ('wide_frontier', 'conn_wide')          # not in the fixture: the model is held to the oracle instead
SMALL = tuple(n for n in CASES if n not in LARGE)
INPUT_KEYS = {'area': ('n_rows', 'n_cols', 'cp', 'ci', 'cd', 'rp', 'ri', 'area', 'done', 'ids', 'edge_todo', 'edge_todo_no_mask',
                       'skip_edge'),
              'conn': ('arr', 'ids', 'indptr', 'indices', 'set_to')}


def area_args(case):
    """fresh copies of what the call updates in place, and the argument tuple of drain_area"""
    a, d, i = case['area'].copy(), case['done'].copy(), case['ids'].copy()
    e = None if case['edge_todo'] is None else case['edge_todo'].copy()
    f = None if case['edge_todo_no_mask'] is None else case['edge_todo_no_mask'].copy()
    return (a, d, i, case['cp'], case['ci'], case['cd'], case['rp'], case['ri'], case['n_rows'], case['n_cols'], e, f,
            case['skip_edge'])


def conn_args(case):
    return (case['arr'].copy(), case['ids'].copy(), case['indptr'], case['indices'], case['set_to'])


def call(module, case):
    """Run a case through `module`.drain_area / drain_connections (the oracle, the shim or the reference's module) ->
    (dict of the arrays after the call, what the call returned)"""
    if case['kind'] == 'area':
        args = area_args(case)
        ret = module.drain_area(*args)
        return dict(area=args[0], done=args[1], ids=args[2], edge_todo=args[10], edge_todo_no_mask=args[11]), ret
    args = conn_args(case)
    ret = module.drain_connections(args[0], args[1], args[2], args[3], set_to=args[4])
    return dict(arr=args[0], ids=args[1]), ret


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and np.array_equal(a, b))


# --- the reference's call sequence around drain_area ----------------------------------------------------------------------

def model_as_drain_area(area, done, ids, cp, ci, cd, rp, ri, n_rows, n_cols, edge_todo=None, edge_todo_no_mask=None, skip_edge=0):
    """the capped model behind the signature of drain_area (in place); an input that it does not finish is an error"""
    case = dict(kind='area', n_rows=n_rows, n_cols=n_cols, cp=cp, ci=ci, cd=cd, rp=rp, ri=ri, area=area, done=done, ids=ids,
                edge_todo=edge_todo, edge_todo_no_mask=edge_todo_no_mask, skip_edge=skip_edge)
    res = model_drain_area(case)
    if res is None:
        raise RuntimeError("drain_area does not end on this input within %d rounds" % ROUND_CAP)
    for key, arr in (('area', area), ('done', done), ('ids', ids), ('edge_todo', edge_todo), ('edge_todo_no_mask', edge_todo_no_mask)):
        if arr is not None:
            arr[:] = res[key]
    return area, done, edge_todo, edge_todo_no_mask


def uca_chunk_driver(o, csr, drain_area, circular_ref_maxcount=50):
    """The stall / re-seed loop of the reference's UCA chunk around a pluggable drain_area: drain from the cells without
    in-edges; while cells are left, the last call got somewhere and the count allows it, seed every cell that is not done and
    lies within 1 % of the highest not-done elevation, and drain again.  `o`: an OracleDEM after build_graph, whose
    uca_drain_state() supplies area, ids and taints.  -> (uca, edge_todo, edge_done, number of drain_area calls)"""
    n, m = o.elev.shape
    cp, ci, cd = o.A
    rp, ri = csr
    st = o.uca_drain_state()
    area, et, etn = st['area'], st['edge_todo'], st['edge_todo_no_mask']
    ids = st['ids'].copy()
    done = ids.copy()
    elev = o.elev.ravel()
    count, done_sum, calls = 1, 0, 0
    while (~done).any() and count < circular_ref_maxcount and done_sum != int(done.sum()):
        done_sum = int(done.sum())
        count += 1
        drain_area(area, done, ids, cp, ci, cd, rp, ri, n, m, et, etn)
        calls += 1
        left = elev * (~done)
        top = left.max()
        with np.errstate(invalid='ignore', divide='ignore'):
            ids = (left - top) / top > -0.01
    uca = area.copy()
    uca[np.asarray(o.flats, bool).ravel()] = np.nan
    edge_done = ~(et != 0) | np.isnan(elev)
    return uca.reshape(n, m), st['edge_todo_i'].reshape(n, m), edge_done.reshape(n, m), calls


def sequence_field(name, built=True):
    """-> an OracleDEM after build_graph and its CSR: three level 9 x 10 fields with cells that drain into each other (the loops
    that make the chunk stall and re-seed), and a 120 x 90 fractal with pits.  built=False: the OracleDEM before build_graph
    (calc_uca builds the graph itself, and building it patches flats and slopes in place: not twice on one object)"""
    from oracle import oracle as O
    if name == 'fractal_pits':
        from pydem_amd import synth
        o = O.OracleDEM(synth.fractal(120, 90, seed=51, top_shift=6, n_octaves=6), dX=30.0, dY=30.0, drain_pits=True)
        o.calc_slopes_directions()
    else:
        n, m = 9, 10
        E, N, W, S = 0.0, 0.5 * np.pi, np.pi, 1.5 * np.pi
        direction = np.full((n, m), S)
        if name == 'two_cells':
            direction[3, 3] = E; direction[3, 4] = W
        elif name == 'three_cells':
            direction[3, 3] = E; direction[3, 4] = S; direction[4, 4] = 0.75 * np.pi
        else:
            direction[2, 2] = E; direction[2, 3] = W
            direction[5, 6] = S; direction[6, 6] = N
        o = O.OracleDEM(np.full((n, m), 10.0), dX=2.0, dY=3.0)
        o.mag, o.direction, o.flats = np.ones((n, m)), direction, np.zeros((n, m), np.uint8)
    if not built:
        return o
    o.build_graph()
    return o, O.tocsr(o.A[0], o.A[1], o.elev.size)


SEQUENCE_FIELDS = ('two_cells', 'three_cells', 'two_loops', 'fractal_pits')
