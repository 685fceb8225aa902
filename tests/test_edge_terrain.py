"""The conditions tests/test_gpu_edge_forms.py rests on, on the CPU (numpy and the oracle): the ridge tiles of
tests/edge_terrain.py leave the counts of unfinished cells the forms of the edge fix-up are chosen by, and their round
programs have cascades whose frontiers pass the one-workgroup caps of csrc/uca_edge.hip (4096 cells, 1024 records) in
both directions.  If the recipe drifts (the generator, the oracle, the graph), this says so before a GPU is involved."""
import numpy as np
import pytest

import edge_terrain as T

CAP, CCAP = T.SMALL_CAP, T.CINC_CAP


def _show(tname, pname, rnd, w):
    print('%s / %s round %d: %d levels, first %d, max %d, min %d; crosses %d up at %s, down at %s; crosses %d up at %s, down at %s'
          % ((tname, pname, rnd, len(w), w[0], max(w), min(w), CAP) + T.crossings(w, CAP) + (CCAP,) + T.crossings(w, CCAP)))
    for cap in (CAP, CCAP):
        for k in sorted(sum(T.crossings(w, cap), [])):
            print('    widths of levels %d..%d: %s' % (k - 2, k + 1, w[k - 2:k + 2]))


def _widths(tname, pname, rnd):
    w = T.oracle_rounds(tname, pname)[rnd].widths
    _show(tname, pname, rnd, w)
    return w


def test_first_pass_leaves_every_form_its_tile():
    s, r = T.first_pass('ridge_smooth'), T.first_pass('ridge_rough')
    assert s.uca.shape == T.SHAPE
    # nothing is finished on the smooth ridge (every cell lies below the top line), one sweep without a re-seed
    assert int((~s.edge_done).sum()) == 768000
    assert int(s.edge_todo.sum()) == 6086
    assert s.stats[0] == 1
    assert int((~r.edge_done).sum()) == 701787
    assert len(r.pit_i) > 1000 and not np.isnan(r.uca).any()          # (measured: 8483 pit -> drain edges, every pit drained)
    # below 2^20 records the condensed form is built; the compact one holds up to 6 Mi (ND_COMPACT_MAX)
    assert int((~s.edge_done).sum()) < 1 << 20 and int((~r.edge_done).sum()) < 1 << 20


def test_frontier_grows_by_at_most_two_cells_per_level_on_the_smooth_ridge():
    for pname in ('outer2000_then_all', 'outer5000_then_all'):
        for rnd in (0, 1):
            w = np.array(T.oracle_rounds('ridge_smooth', pname)[rnd].widths)
            assert len(w) == 128 and np.abs(np.diff(w)).max() <= 2


def test_smooth_outer2000():
    w0 = _widths('ridge_smooth', 'outer2000_then_all', 0)
    # wider than the compact form's workgroup, narrower than the cell-indexed one's: measured 2000 down to 1764
    assert w0[0] == 2000 and all(a >= b for a, b in zip(w0, w0[1:]))
    assert CCAP < min(w0) and max(w0) < CAP
    w1 = _widths('ridge_smooth', 'outer2000_then_all', 1)
    # measured: 4000 at level 0, past 4096 at level 50, 4236 at the last of 128 levels
    assert w1[0] == 4000 and len(w1) == 128 and max(w1) > CAP
    up, down = T.crossings(w1, CAP)
    assert len(up) == 1 and not down and up[0] > 1 and len(w1) - up[0] > 16


def test_smooth_outer5000_crosses_1024_upward():
    w1 = _widths('ridge_smooth', 'outer5000_then_all', 1)
    # measured: 1000 at level 0, 14 levels up to 1024, then 114 above (max 1233)
    assert w1[0] == 1000 and max(w1) < CAP
    up, down = T.crossings(w1, CCAP)
    assert len(up) == 1 and not down
    assert sum(x <= CCAP for x in w1) >= 2 and sum(x > CCAP for x in w1) > 16


def test_smooth_all_at_once_is_wide_throughout():
    w = _widths('ridge_smooth', 'all_at_once', 0)
    assert w[0] == 6000 and all(x > CAP for x in w[:-1])


def test_rough_cascades_cross_both_caps_in_both_directions():
    # measured: inner4200 round 0 starts at 4200 and passes 4096 down at levels 30, 89 and 128, up at 73 and 107 (135
    # levels, the last 4 up to 1024 wide); outer2000 round 1 up at 107, down at 128; outer5000 round 1 starts at 1000 and
    # passes 1024 up at 14, 71 and 95, down at 30, 90 and 129
    wi = _widths('ridge_rough', 'inner4200_then_all', 0)
    assert wi[0] == 4200
    up, down = T.crossings(wi, CAP)
    assert len(up) >= 1 and len(down) >= 2
    wo = _widths('ridge_rough', 'outer2000_then_all', 1)
    up, down = T.crossings(wo, CAP)
    assert wo[0] == 4000 and len(up) >= 1 and len(down) >= 1
    ups = downs = 0
    for pname in ('outer2000_then_all', 'inner4200_then_all', 'outer5000_then_all'):
        for rnd in (0, 1):
            up, down = T.crossings(T.oracle_rounds('ridge_rough', pname)[rnd].widths, CCAP)
            ups += len(up); downs += len(down)
    _widths('ridge_rough', 'outer5000_then_all', 1)
    assert ups >= 1 and downs >= 1


@pytest.mark.parametrize('pname,rnd,cap,least', [('inner4200_then_all', 0, CAP, 2), ('outer2000_then_all', 1, CAP, 1),
                                                 ('outer5000_then_all', 1, CCAP, 2)])
def test_rough_cascades_change_hands_whatever_the_batch(pname, rnd, cap, least):
    """The GPU tests ask for hand-overs between the one-workgroup kernel and the level kernels without knowing how many
    levels the host launches per look: they ask for as many as the widths give with every batch of up to 32 levels.  That
    is two where the frontier stays below the cap for longer than a batch (inner4200: levels 30-72; outer5000 under the
    cap of 1024: levels 0-13 and 30-70), and one in outer2000's second round, whose only stretch below 4096 after the wide
    levels is the tail (levels 128-134), which a batch of 16 started at level 107 runs past."""
    w = T.oracle_rounds('ridge_rough', pname)[rnd].widths
    assert max(w) > cap
    assert T.least_handovers(w, cap) >= least
    print('%s round %d, cap %d, batches of 16: %d levels by the level kernels, %d hand-overs' % ((pname, rnd, cap) + T.schedule(w, cap)))


def test_schedule_and_crossings_on_a_hand_made_cascade():
    w = [3, 5, 9, 9, 9, 4, 2, 8, 1]
    assert T.crossings(w, 4) == ([1, 7], [5, 8])
    assert T.schedule(w, 4, batch=1) == (5, 4)          # small 0, wide 1-4, small 5-6, wide 7, small 8
    assert T.schedule(w, 4, batch=4) == (8, 3)          # small 0, wide 1-4, small 5-6, wide 7-10 (overshoots the end)
    assert T.schedule([9, 9, 1], 4, batch=16) == (16, 0)


def test_level_widths_on_a_hand_made_graph():
    # 0 -> 1 -> 3, 2 -> 3, 3 -> 4, 5 -> 4 with 5 outside the set: levels {0, 2}, {1}, {3}, {4}
    indptr = np.array([0, 1, 2, 3, 4, 4, 5], np.int32)
    indices = np.array([1, 3, 3, 4, 4], np.int32)
    newly = np.array([[1, 1, 1, 1, 1, 0]], bool)
    assert T.level_widths((indptr, indices, None), newly) == [2, 1, 1, 1]


def test_classic_round_floods_and_sweeps():
    """The classic round's floods start from every inlet at once (more than 4096 in every first round), and
    its sweep runs over everything below the seeds, finished or not, with every seed at level 0: on the rough ridge it
    changes hands at least twice in three rounds (measured with batches of 16: outer2000 round 1 starts at 8235, 48 levels
    by the level kernels, 2 hand-overs; inner4200 round 0 96 and 3; outer5000 round 0 112 and 2)."""
    for tname in ('ridge_smooth', 'ridge_rough'):
        for pname in ('outer2000_then_all', 'inner4200_then_all', 'outer5000_then_all', 'all_at_once'):
            for rnd, r in enumerate(T.oracle_rounds(tname, pname)):
                assert r.inlets > CAP or rnd == 1, (tname, pname, rnd)
                print('%s / %s round %d: %d inlets; sweep %d levels, first %d, max %d, %d by the level kernels and %d hand-overs with batches of 16'
                      % ((tname, pname, rnd, r.inlets, len(r.sweep_widths), r.sweep_widths[0], max(r.sweep_widths)) + T.schedule(r.sweep_widths, CAP)))
    for pname, rnd in (('outer2000_then_all', 1), ('inner4200_then_all', 0), ('outer5000_then_all', 0)):
        assert T.least_handovers(T.oracle_rounds('ridge_rough', pname)[rnd].sweep_widths, CAP) >= 2


def test_condensed_interior_cascade_changes_hands_on_the_rough_ridge():
    """The condensed form's catch-up starts from every newly finished perimeter cell at once: wider than 1024 at level 0 in
    every round of every program; on the rough ridge outer5000's second round then passes 1024 up at levels 14, 71 and 95
    and down at 1, 30, 90 and 128 (measured; with batches of 16: 96 levels by the level kernels, 2 hand-overs)."""
    for tname in ('ridge_smooth', 'ridge_rough'):
        for pname in ('outer2000_then_all', 'inner4200_then_all', 'outer5000_then_all', 'all_at_once'):
            for r in T.oracle_rounds(tname, pname):
                assert r.interior_widths[0] > CCAP
    w = T.oracle_rounds('ridge_rough', 'outer5000_then_all')[1].interior_widths
    print('interior cascade of ridge_rough / outer5000_then_all round 1: %d levels, crosses 1024 up at %s, down at %s' % ((len(w),) + T.crossings(w, CCAP)))
    assert T.least_handovers(w, CCAP) >= 2


@pytest.mark.parametrize('tname', ['ridge_smooth', 'ridge_rough'])
def test_condensed_operator_overflows_the_device_builds_pool(tname):
    """Why the GPU tests expect the device build of the condensed operator to hand over to the host build on these ridges:
    the vectors hold about three times what its merge pool does (measured: 44.5 M entries against 12.5 M on the smooth
    ridge, where the host build itself counts 42.2 M; 35.5 M against 11.5 M on the rough one)."""
    entries, records = T.operator_entries(tname)
    print('%s: about %d vector entries, pool %d' % (tname, entries, 16 * (records + 16384)))
    assert entries > 2 * 16 * (records + 16384)
