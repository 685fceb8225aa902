"""Every form of the cross-tile edge fix-up (csrc/uca_edge.hip) at frontiers wider than one workgroup, against the oracle's
plain rounds, cell by cell: the classic round, the incremental rounds on cells, on compact records and on the condensed
operator (the default build, which on these tiles hands over from the device to the host, and the host build asked for).  The tiles and round programs are those of tests/edge_terrain.py (128 x
6000 ridges whose cascades pass the one-workgroup caps in both directions; tests/test_edge_terrain.py holds them to that
on the CPU).  Every case reads from the PYDEM_EDGE_DEBUG lines that the device ran the requested form, that the level
kernels ran where the oracle's frontier widths say so, and how often the cascade changed hands."""
import re
import warnings

import numpy as np
import pytest

import edge_terrain as T
from test_gpu_parity import _close

pytestmark = pytest.mark.gpu

TERRAINS = ('ridge_smooth', 'ridge_rough')
PROGRAMS = ('outer2000_then_all', 'inner4200_then_all', 'outer5000_then_all', 'all_at_once')
FORMS = {'classic': {},
         'cell-indexed': {'PYDEM_EINC_COMPACT_MAX': '0'},
         'compact': {'PYDEM_EDGE_COND_MAX': '0'},
         'condensed-device': {},                    # (the default; on these ridges the device build hands over to the host build)
         'condensed-host': {'PYDEM_COND_BUILD': 'host'}}
SWITCHES = ('PYDEM_EINC_COMPACT_MAX', 'PYDEM_EDGE_COND_MAX', 'PYDEM_COND_BUILD')
CAP = {'classic': T.SMALL_CAP, 'cell-indexed': T.SMALL_CAP, 'compact': T.CINC_CAP}

RE_CLASSIC = re.compile(r'edge round: (\d+) seeds, .*levels: floods (\d+) \((\d+) wide\), sweep (\d+) \((\d+) wide\); hand-overs (\d+) \+ (\d+);')
RE_INC = re.compile(r'incremental edge round \(([a-z-]+)\): (\d+) levels, (\d+) by the level kernels, (\d+) hand-overs')
RE_INC_FLUSH = re.compile(r'incremental edge rounds \(([a-z-]+)\): flush (\d+) levels, (\d+) by the level kernels, (\d+) hand-overs')
RE_COND = re.compile(r'condensed edge round: (\d+) levels on (\d+) nodes')
RE_CATCHUP = re.compile(r'condensed edge catch-up \(interior cascade\): (\d+) levels, (\d+) by the level kernels, (\d+) hand-overs')
RE_COND_FLUSH = re.compile(r'condensed edge rounds: flush .*; (\d+) rounds ran on the watched graph, .*; interior: (\d+) \+ (\d+) levels, (\d+) by the level kernels, (\d+) hand-overs')
BUILT_ON_DEVICE = re.compile(r'condensed edge rounds \(device build\): \d+ records -> \d+ watched nodes')
DEVICE_GAVE_UP = 'condensed edge rounds (device build): gave up'
BUILT_ON_HOST = re.compile(r'condensed edge rounds: \d+ records -> \d+ watched nodes')


def _form(monkeypatch, form):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)
    monkeypatch.setenv('PYDEM_EDGE_DEBUG', '1')


def _said(capfd):
    """What the library wrote since the last look (shown again, so that a failure's report holds it)."""
    got = capfd.readouterr()
    print(got.out + got.err, end='')
    return got.err


def _tile(tname):
    """A tile after its first pass on the device, masks as the oracle's."""
    from pydem_amd import DEMProcessor
    o = T.first_pass(tname)
    dp = DEMProcessor(elev=T.terrain(tname), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
    dp.run_uca()
    assert np.array_equal(dp.edge_done, o.edge_done)
    assert np.array_equal(dp.edge_todo, o.edge_todo)
    return dp


def _incremental(dp, r):
    dp.run_uca(edge_init_data=[r.value, r.done, r.todo], uca_resident=True, incremental=True)


def _check_masks_and_lines(dp, r, what):
    """The bars of test_incremental_edge_rounds_vs_oracle_rounds: masks exactly, areas of the finished perimeter cells."""
    assert np.array_equal(dp.edge_todo, r.edge_todo), what
    assert np.array_equal(dp.edge_done, r.edge_done), what
    for k, sl in T.SIDES.items():
        line = dp.get_line('uca', 1 if k in ('left', 'right') else 0, 0 if k in ('left', 'top') else -1)
        ok = r.edge_done[sl]
        assert np.array_equal(np.isnan(line[ok]), np.isnan(r.uca[sl][ok])), (what, k)
        assert np.allclose(line[ok], r.uca[sl][ok], rtol=1e-9, atol=1e-12, equal_nan=True), (what, k)


def _check_cascade(wide, handovers, widths, cap, what):
    """Level kernels where the oracle's widths pass the cap, and the hand-overs these widths give with any batch."""
    assert (wide > 0) == (max(widths) > cap), (what, wide, max(widths))
    assert handovers >= T.least_handovers(widths, cap), (what, handovers)


# Where the condensed operator of a ridge is built when nothing is asked for.  On a plane the water of a cell fans out over
# one more watched cell of the bottom line per row, so the operator's vectors hold 42 M entries on the smooth ridge (the host
# build's own count) and about 35 M on the rough one (the same count on the oracle's graph), against a merge pool of 16 x
# (records + 16384) = 12 M entries: the device build fills its pool in the middle of its sweep, gives up, and the host build
# takes the tile.  So 'condensed-device' here is the default path THROUGH that hand-over, asserted as such; this file does
# not reach a device-built operator (tests/test_gpu_process_manager.py compares that one with the host build node by node).
DEVICE_BUILD_COMPLETES = {'ridge_smooth': False, 'ridge_rough': False}


def _check_operator_build(form, tname, err, what):
    on_device, gave_up, on_host = bool(BUILT_ON_DEVICE.search(err)), DEVICE_GAVE_UP in err, bool(BUILT_ON_HOST.search(err))
    if form == 'condensed-host':
        assert (on_device, gave_up, on_host) == (False, False, True), (what, err)
    elif DEVICE_BUILD_COMPLETES[tname]:
        assert (on_device, gave_up, on_host) == (True, False, False), (what, err)
    else:
        assert (on_device, gave_up, on_host) == (False, True, True), (what, err)


def _check_incremental_branch(form, tname, r, err, what, first):
    if form in ('cell-indexed', 'compact'):
        m = RE_INC.search(err)
        assert m and m.group(1) == form, (what, err)
        assert not RE_COND.search(err) and not RE_CLASSIC.search(err), what
        _check_cascade(int(m.group(3)), int(m.group(4)), r.widths, CAP[form], what)
        return
    assert RE_COND.search(err) and not RE_INC.search(err) and not RE_CLASSIC.search(err), (what, err)
    if first:
        _check_operator_build(form, tname, err, what)
    # the interior catches up when the masks are read: k_cinc_small / k_cinc_level below the watched cells this round finished
    m = RE_CATCHUP.search(err)
    assert m, (what, err)
    _check_cascade(int(m.group(2)), int(m.group(3)), r.interior_widths, T.CINC_CAP, what)


@pytest.mark.parametrize('pname', PROGRAMS)
@pytest.mark.parametrize('tname', TERRAINS)
@pytest.mark.parametrize('form', list(FORMS))
def test_edge_forms_vs_oracle_rounds(form, tname, pname, monkeypatch, capfd):
    rounds = T.oracle_rounds(tname, pname)
    _form(monkeypatch, form)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = _tile(tname)
        _said(capfd)
        if form == 'classic':
            uca = dp.uca
            for k, r in enumerate(rounds):
                what = (form, tname, pname, k)
                uca = dp.calc_uca(uca_init=uca, edge_init_data=[r.value, r.done, r.todo_oracle])
                _close(uca, r.uca, 'uca after classic round %d' % k)
                assert np.array_equal(dp.edge_todo, r.edge_todo), what
                assert np.array_equal(dp.edge_done, r.edge_done), what
                m = RE_CLASSIC.search(_said(capfd))
                assert m, what
                _, _, flood_wide, _, sweep_wide, _, sweep_handovers = map(int, m.groups())
                assert flood_wide > 0 or r.inlets <= T.SMALL_CAP, what      # the floods start from every inlet at once
                _check_cascade(sweep_wide, sweep_handovers, r.sweep_widths, T.SMALL_CAP, what)
            return
        for k, r in enumerate(rounds):
            what = (form, tname, pname, k)
            _incremental(dp, r)
            _check_masks_and_lines(dp, r, what)
            _check_incremental_branch(form, tname, r, _said(capfd), what, k == 0)
        dp.flush_edge_rounds()
        _close(dp.uca, rounds[-1].uca, 'uca after the flush')
        _said(capfd)


@pytest.mark.parametrize('tname', TERRAINS)
@pytest.mark.parametrize('form', ['condensed-device', 'condensed-host'])
def test_condensed_rounds_without_a_host_read_in_between(form, tname, monkeypatch, capfd):
    """The situation of the queued waves: round after round on the watched graph, nothing downloaded in between, so no
    catch-up of the interior before the flush, which then has the cells of both rounds to finish in one cascade.  The
    rounds run without the debug switch (with it every round waits for the stream and reads its counters); the operator is
    built in the first of them, so where it was built is not shown here.  The flush runs with the switch: it reports two
    rounds on the watched graph and an interior cascade over the cells of both."""
    rounds = T.oracle_rounds(tname, 'outer2000_then_all')
    o = T.first_pass(tname)
    _form(monkeypatch, form)
    monkeypatch.delenv('PYDEM_EDGE_DEBUG')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = _tile(tname)
        for r in rounds:
            _incremental(dp, r)
        assert 'edge round' not in _said(capfd)
        monkeypatch.setenv('PYDEM_EDGE_DEBUG', '1')
        dp.flush_edge_rounds()
        err = _said(capfd)
        m = RE_COND_FLUSH.search(err)
        assert m and not RE_CATCHUP.search(err), err
        assert int(m.group(1)) == 2 + 1, err            # (the flush lets the remaining inlets go in a round of its own)
        both = T.interior_widths(o.A, rounds[-1].edge_done & ~o.edge_done)
        _check_cascade(int(m.group(4)), int(m.group(5)), both, T.CINC_CAP, (form, tname))
        _close(dp.uca, rounds[-1].uca, 'uca after the flush')
        assert np.array_equal(dp.edge_todo, rounds[-1].edge_todo)
        assert np.array_equal(dp.edge_done, rounds[-1].edge_done)


@pytest.mark.parametrize('tname', TERRAINS)
@pytest.mark.parametrize('form', ['cell-indexed', 'compact', 'condensed-device'])
def test_second_series_after_a_flush(form, tname, monkeypatch, capfd):
    """The flush drops the incremental state: a round, the flush (cells below the inlets that stay 'todo' get the partial
    sums of the plain round), then a new series on the same tile, which starts from the masks again."""
    rounds = T.oracle_rounds(tname, 'outer2000_then_all')
    _form(monkeypatch, form)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = _tile(tname)
        _said(capfd)
        for k, r in enumerate(rounds):
            what = (form, tname, 'series %d' % k)
            _incremental(dp, r)
            _check_masks_and_lines(dp, r, what)
            _check_incremental_branch(form, tname, r, _said(capfd), what, True)
            dp.flush_edge_rounds()
            err = _said(capfd)
            assert (RE_COND_FLUSH if form == 'condensed-device' else RE_INC_FLUSH).search(err), (what, err)
            _close(dp.uca, r.uca, 'uca after the flush of series %d' % k)
            assert np.array_equal(dp.edge_todo, r.edge_todo), what
            assert np.array_equal(dp.edge_done, r.edge_done), what


@pytest.mark.parametrize('resident', [True, False])
@pytest.mark.parametrize('form', ['cell-indexed', 'condensed-device'])
def test_classic_round_after_an_incremental_one(form, resident, monkeypatch, capfd):
    """An incremental round leaves deltas waiting and the classic round's zeroed state gone.  On the resident plane the
    classic round flushes first (stage_edge_update); calc_uca(uca_init=tile.uca, ...) settles them with the download."""
    rounds = T.oracle_rounds('ridge_rough', 'outer2000_then_all')
    _form(monkeypatch, form)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = _tile('ridge_rough')
        _incremental(dp, rounds[0])
        _check_masks_and_lines(dp, rounds[0], (form, 'incremental round'))
        _said(capfd)
        r = rounds[1]
        if resident:
            dp.run_uca(edge_init_data=[r.value, r.done, r.todo_oracle], uca_resident=True)
            uca = dp.uca
        else:
            uca = dp.calc_uca(uca_init=dp.uca, edge_init_data=[r.value, r.done, r.todo_oracle])
        err = _said(capfd)
        assert (RE_COND_FLUSH if form == 'condensed-device' else RE_INC_FLUSH).search(err), err
        m = RE_CLASSIC.search(err)
        assert m and int(m.group(5)) > 0, err
    _close(uca, r.uca, 'uca after the classic round')
    assert np.array_equal(dp.edge_todo, r.edge_todo)
    assert np.array_equal(dp.edge_done, r.edge_done)


NAN_AT = 3000


@pytest.mark.parametrize('form', ['cell-indexed', 'compact'])
def test_nan_seed_in_a_wide_round(form, monkeypatch, capfd):
    """One NaN among 6000 seeds: the NaN flood runs below a cascade that the level kernels carry from its first level.
    The NaN pattern is the oracle's, where NaN is absorbing in area_edges - uca; every other cell is held to the bars."""
    r, = T.oracle_rounds('ridge_smooth', 'all_at_once', NAN_AT)
    clean, = T.oracle_rounds('ridge_smooth', 'all_at_once')
    nan = np.isnan(r.uca)
    assert 100 < nan.sum() < nan.size // 2 and not np.isnan(clean.uca).any()        # (the flood has somewhere to go)
    assert np.array_equal(r.uca[~nan], clean.uca[~nan])
    _form(monkeypatch, form)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = _tile('ridge_smooth')
        _said(capfd)
        _incremental(dp, r)
        _check_masks_and_lines(dp, r, (form, 'NaN seed'))
        _check_incremental_branch(form, 'ridge_smooth', r, _said(capfd), (form, 'NaN seed'), True)
        dp.flush_edge_rounds()
        _close(dp.uca, r.uca, 'uca after the flush')
