"""CPU tier of the edge-board tests: the model in tests/board_model.py is a faithful stand-in for the manager, its hash is a
sufficient witness of a tile's strips, and the designed inputs of tests/test_gpu_board_eval.py and
tests/test_gpu_board_schedule.py reach the branches they were designed for.  (Conditions on the INPUTS: they are asserted on
the model alone, so they run here; the GPU tier then compares the kernels with the same model on the same inputs.)"""
import warnings

import numpy as np
import pytest

import board_model as B
from conftest import load_golden
from oracle_processor import OracleProcessor
from pydem_amd.process_manager import CORNERS, SIDES, ProcessManager
from test_process_manager_grid import write_tiles

PM = ProcessManager


# ---------------------------------------------------------------------------------------------- harness faithfulness
def _same(a, b):
    return all(np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=(np.asarray(x[k]).dtype.kind == 'f'))
               for x, y in zip(a, b) for k in SIDES)


@pytest.mark.parametrize('name', ['pm_cone32_4x5_ov3', 'pm_nansea_2x2_ov2', 'pm_cone32_3x3_ov1'])
def test_stub_manager_answers_like_the_manager(name, tmp_path):
    """An oracle-backed manager (as in tests/test_process_manager_pool.py), stopped after process_uca and again after the
    fix-up: `StubManager.from_manager` carries nothing but its edge table, and the rule functions give the same strips,
    metric and dropped pixels on it as on the manager itself -- for every tile, in all three `drop_mutual_todo` modes."""
    from pydem_amd import process_manager
    g = load_golden(name)
    dkw = {k: v for k, v in g['kwargs'].items() if k not in ('ny_grid', 'nx_grid', 'overlap')}
    write_tiles(g, str(tmp_path), key='elev')
    process_manager.DEBUG = True
    try:
        pm = process_manager.ProcessManager(in_path=str(tmp_path), dem_proc_kwargs=dkw, elev_conditioned=True,
                                            processor_cls=OracleProcessor, n_workers=8)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            pm.compute_grid(); pm.process_elevation(); pm.process_aspect_slope(); pm.process_uca()
            seen_1ov = False
            for stage in ('first pass', 'fixed up'):
                if stage == 'fixed up':
                    pm.process_uca_edges()
                pm._edge_setup()
                stub = B.StubManager.from_manager(pm)
                plan = B.BoardPlan(stub)
                for i in range(pm.n_inputs):
                    reqs = sorted(pm._snapshot_requests(i) | pm._metric_requests(i))
                    assert reqs == sorted(PM._snapshot_requests(stub, i) | PM._metric_requests(stub, i))
                    assert all(r in plan.layout for r in reqs)
                    snap = dict(zip(reqs, pm._edge_lines(reqs)))
                    seen_1ov = seen_1ov or any(stub.edge_data[i][key] for key in CORNERS)
                    assert PM._tile_metric(stub, i, snap) == pm._tile_metric(i, snap), (stage, i)
                    for mode in (True, False, 'self'):
                        mine = PM._edge_inputs(stub, i, snap, drop_mutual_todo=mode)
                        theirs = pm._edge_inputs(i, snap, drop_mutual_todo=mode)
                        assert _same(mine, theirs), (stage, i, mode)
                        assert PM._todo_dropped(stub, i, snap, mine[2]) == pm._todo_dropped(i, snap, theirs[2]), (stage, i, mode)
                    # the denominator of the metric, counted by the manager's own function
                    frac, n_done = pm._tile_metric(i, snap)
                    p_done = B._count_todo(stub, i, snap)
                    assert frac == n_done / (1e-16 + p_done), (stage, i)
    finally:
        process_manager.DEBUG = False
    # (of the pm_* fixtures only those cut with overlap 1 have corners that pass check_1overlap: the third one is here for them)
    assert seen_1ov == name.endswith('ov1')


def test_mosaic_builder_builds_the_managers_descriptor_order():
    """offsets28 = own_todo, own_done, nb_uca, nb_done, nb_todo (sides left, right, top, bottom), cnr_done, cnr_uca (corners tl,
    tr, bl, br); flags8 = nb_self, one-overlap.  Checked on a 2 x 2 mosaic by reading the cells back through the offsets."""
    shapes, table = B.mosaic((4, 3), (5, 2), depth=1, one_overlap=True)
    case = B.Case('probe', shapes, table, seed=1)
    mb = case.plan.board(case.tiles)
    n, m, o, f = case.plan.desc[0]
    assert (n, m) == (4, 5) and f == [1, 0, 1, 0, 0, 0, 0, 1]
    t = case.tiles
    assert np.array_equal(mb[o[0]:o[0] + n], t[0].line('edge_todo', 1, 0)) and np.array_equal(mb[o[3]:o[3] + m], t[0].line('edge_todo', 0, -1))
    assert np.array_equal(mb[o[4 + 1]:o[4 + 1] + n], t[0].line('edge_done', 1, -1))
    assert np.array_equal(mb[o[8 + 1]:o[8 + 1] + n], t[1].line('uca', 1, 0), equal_nan=True)           # right: tile 1's first column
    assert np.array_equal(mb[o[12 + 3]:o[12 + 3] + m], t[2].line('edge_done', 0, 0))                    # bottom: tile 2's first row
    assert np.array_equal(mb[o[16 + 0]:o[16 + 0] + n], t[0].line('edge_todo', 1, 0))                    # left: the tile's own line
    assert mb[o[20 + 3]] == t[3].line('edge_done', 0, 0)[0] and o[24:27] == [-1, -1, -1]
    assert np.array_equal(mb[o[24 + 3]], t[3].line('uca', 0, 0)[0], equal_nan=True)
    assert case.plan.readers[3] == {0, 1, 2, 3} and case.plan.nbrs[0] == {0, 1, 2}


# ---------------------------------------------------------------------------------------------- hash sensitivity
def _strips(rng, n, m):
    tot = 2 * n + 2 * m
    data = rng.uniform(1.0, 1e6, tot)
    data[rng.integers(0, tot, 4)] = [-0.0, np.nan, 5e-324, 1e15]
    return data, rng.random(tot) < 0.5, rng.random(tot) < 0.5


@pytest.mark.parametrize('n,m', [(1, 1), (1, 7), (7, 1), (5, 9), (64, 33)])
def test_strip_hash_sees_every_element(n, m):
    rng = np.random.default_rng(n * 100 + m)
    data, done, tda = _strips(rng, n, m)
    done[:2] = True
    h = B.strip_hash(n, m, data, done, tda)
    assert h == B.strip_hash(n, m, {k: v for k, v in zip(SIDES, np.split(data, [n, 2 * n, 2 * n + m]))}, done, tda)
    for q in range(data.size):
        for which in range(3):
            d2, dn2, t2 = data.copy(), done.copy(), tda.copy()
            if which == 0:
                d2.view(np.uint64)[q] ^= np.uint64(1) << np.uint64(q % 52)     # one bit of the value
            elif which == 1:
                dn2[q] = not dn2[q]
            else:
                t2[q] = not t2[q]
            h2 = B.strip_hash(n, m, d2, dn2, t2)
            if which == 0 and not done[q]:
                assert h2 == h, q                             # the value of an unfinished neighbour cell never enters a round
            else:
                assert h2 != h, (q, which)
    for q1 in range(data.size):
        q2 = (q1 * 7 + 3) % data.size
        a = (done[q1] and data[q1].tobytes() or b'', done[q1], tda[q1])
        b = (done[q2] and data[q2].tobytes() or b'', done[q2], tda[q2])
        perm = np.arange(data.size); perm[[q1, q2]] = perm[[q2, q1]]
        h2 = B.strip_hash(n, m, data[perm], done[perm], tda[perm])
        assert (h2 == h) == (a == b), (q1, q2)


def test_strip_hash_takes_values_by_their_bits():
    done, tda = np.ones(4, bool), np.zeros(4, bool)
    nan2 = np.array([0x7ff8000000000001], np.uint64).view(np.float64)[0]
    base = B.strip_hash(1, 1, np.array([0.0, 1.0, np.nan, 2.0]), done, tda)
    assert base != B.strip_hash(1, 1, np.array([-0.0, 1.0, np.nan, 2.0]), done, tda)
    assert base != B.strip_hash(1, 1, np.array([0.0, 1.0, nan2, 2.0]), done, tda)
    assert base != B.strip_hash(1, 1, np.array([5e-324, 1.0, np.nan, 2.0]), done, tda)


# ---------------------------------------------------------------------------------------------- coverage of the evaluation cases
def _corner_state(case, i):
    """per corner of tile i: (top / bottom strip finished there, left / right strip finished there, one-overlap, diagonal finished)"""
    stub, snap = case.stub, case.snap
    out = {}
    for key, (tb, lr, ptb, plr) in B.CORNER_OF.items():
        fin = []
        for side, pos in ((tb, ptb), (lr, plr)):
            src, axis, idx = stub._edge_line(i, side)
            fin.append(bool(src >= 0 and snap[(src, 'edge_done', axis, idx)][pos]))
        src, r, c = stub._edge_line(i, key)
        out[key] = (fin[0], fin[1], bool(stub.edge_data[i][key]), bool(src >= 0 and snap[(src, 'edge_done', 0, r)][c]))
    return out


def test_evaluation_cases_reach_the_branches_they_were_designed_for():
    seen = set()
    shapes_3x3, shapes_self, shapes_alone = set(), set(), set()
    for case in B.eval_cases() + [B.many_tiles_case()]:
        for i in case.evaluate:
            n, m = case.stub.tiles_shape[i]
            where = [case.stub._edge_line(i, key) for key in SIDES]
            if all(src >= 0 and src != i for src, _, _ in where) and all(case.stub._edge_line(i, key)[0] >= 0 for key in CORNERS):
                shapes_3x3.add((n, m))
            if all(src == i for src, _, _ in where):
                shapes_self.add((n, m))
            if all(src < 0 for src, _, _ in where):
                shapes_alone.add((n, m))
            for key, (tb, lr, ov, diag) in _corner_state(case, i).items():
                thin = 'thin' if min(n, m) == 1 else 'wide'
                if tb and lr and ov and diag:
                    seen.add((key, 'both, diagonal finished', thin))
                if tb and lr and not diag:
                    seen.add((key, 'both, diagonal unfinished', thin))
                if tb != lr:
                    seen.add((key, 'one strip', thin))
                    seen.add((key, 'only ' + ('tb' if tb else 'lr'), thin))
            for key, (src, _, _) in zip(SIDES, where):
                if src == i:
                    seen.add((key, 'self'))
                if src < 0:
                    seen.add((key, 'none'))
            e0, e1 = case.expected(0)[i], case.expected(1)[i]
            if e0[2] != e0[3]:
                seen.add('dropped_self != dropped_full')
            if e0[2] != 0:
                seen.add('dropped_self != 0')
            if e0[5] != e1[5]:
                seen.add('rule :274 changes the strips')
            d, dn, td = PM._edge_inputs(case.stub, i, case.snap, drop_mutual_todo='self')
            if e0[4] > 0 and not any((dn[k] & td[k]).any() for k in SIDES):
                seen.add('seeds by adoption alone')
    for key in CORNERS:
        for what in ('both, diagonal finished', 'both, diagonal unfinished', 'one strip', 'only tb', 'only lr'):
            for thin in ('thin', 'wide'):
                assert (key, what, thin) in seen, (key, what, thin)
    for key in SIDES:
        assert (key, 'self') in seen and (key, 'none') in seen, key
    for what in ('dropped_self != dropped_full', 'dropped_self != 0', 'rule :274 changes the strips', 'seeds by adoption alone'):
        assert what in seen, what
    want = set(B.EVAL_SHAPES)
    assert want <= shapes_3x3 and want <= shapes_self and want <= shapes_alone
    # the launch shapes of pydem_board_eval (ceil(perimeter / 4096) blocks of 1024 threads, at most 16) and of the queued
    # evaluation (ceil(perimeter / 1024), at most 16): one block / two blocks / every thread a second trip
    per = sorted(2 * n + 2 * m for n, m in want)
    assert 4096 in per and 4098 in per and 2048 in per and max(per) > 16 * 1024 and sum(p > 16 * 1024 for p in per) >= 2


def test_the_host_rules_on_the_smallest_thin_board():
    """What the specification says for the board that showed the kernel's disagreement (a 1 x 1 tile between finished right
    and top neighbours, everything else unfinished): the top strip gives its only cell up to the top-RIGHT rule, because
    index -1 is index 0.  A kernel that lets 'the lower end's rule win' keeps it finished."""
    case = {c.name: c for c in B.eval_cases()}['thin_1x1_sides6']          # sides: bit 1 = right, bit 2 = top
    d, dn, td = PM._edge_inputs(case.stub, 4, case.snap, drop_mutual_todo='self')
    assert dn['right'][0] and not dn['left'][0] and not dn['bottom'][0]
    assert not dn['top'][0]
    src, r, c = case.stub._edge_line(4, 'top-right')
    v = case.snap[(src, 'uca', 0, r)][c]
    assert d['top'][0] == v and d['right'][0] == v


# ---------------------------------------------------------------------------------------------- coverage of the scheduler scripts
def run_model(case):
    model = B.ScheduleModel(case.plan, case.initial(), case.script)
    outs = []
    for k, ok, limit in case.steps():
        out = model.batch(k, ok, limit)
        outs.append(out)
        if out[1] == 1:
            break
    return model, outs


def test_scheduler_scripts_produce_the_events_they_were_designed_for():
    events = set()
    for case in B.schedule_cases():
        model, outs = run_model(case)
        assert outs[-1][1] == 1, case.name                    # every script ends
        assert all(not any(t.line(nm, ax, j).any() for (nm, ax, j) in t.lines if nm == 'edge_todo') for t in model.tiles)
        events |= model.events
        assert case.n_t in (4, 6, 9)
    for what in ('wide wave', 'suppressed', 'tie-break then normal', 'stop 1', 'stop 2', 'stop 3', 'full batch', 'stale diagonal',
                 'stale at the end of a batch'):
        assert what in events, what


def test_scheduler_scripts_are_monotone():
    for case in B.schedule_cases():
        tiles = case.initial()
        for t, tile in enumerate(tiles):
            before = tile.copy()
            for k in range(max(case.script.last) + 1):
                case.script(tile, t, k)
                for key, arr in tile.lines.items():
                    if key[0] == 'edge_done':
                        assert not (before.lines[key] & ~arr).any()
                    if key[0] == 'edge_todo':
                        assert not (arr & ~before.lines[key]).any()
                        assert not (arr & tile.lines[('edge_done',) + key[1:]]).any() if ('edge_done',) + key[1:] in tile.lines else True
                before = tile.copy()
