"""The edge board's kernels (pydem_amd/csrc/comm.hip) against the host strip rules, without a mosaic.

k_board_scatter / the segment table: lines written through `Board.refresh(None, tiles, host_sum=fill)` must come back from
`Board.download()` bit for bit.  k_board_eval: the six words of a tile (n_done, p_done, dropped_self, dropped_full, seeds,
hash) must equal `board_model.expected_scalars`, which calls the manager's own `_edge_inputs`, `_todo_dropped`,
`_adopt_finished` and `_tile_metric` on the same lines; the hash is the witness of the strips the kernel writes
(tests/test_board_model.py shows that it notices any single wrong element).  k_board_pack: resident tiles whose rows and
columns are gathered from device memory.  Every comparison is integer or bitwise equality.

The inputs are `board_model.eval_cases()`; tests/test_board_model.py asserts, on the CPU, which branches they reach."""
import numpy as np
import pytest

import board_model as B
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _field(name):
    from pydem_amd import _ffi
    return {'uca': _ffi.UCA, 'edge_todo': _ffi.EDGE_TODO, 'edge_done': _ffi.EDGE_DONE}[name]


def make_board(plan, resident=None):
    """the board of a plan; resident: {tile index: _ffi.Tile} (every other tile is 'remote': layout only)"""
    from pydem_amd import _ffi
    resident = resident or {}
    board = _ffi.Board(0, plan.stub.n_inputs, plan.total)
    for i, (n, m, o28, f8) in enumerate(plan.desc):
        board.set_desc(i, n, m, o28, f8, resident.get(i))
    for t in range(plan.stub.n_inputs):
        board.set_lines(t, plan.start[t], plan.size[t], resident.get(t), [(_field(nm), ax, ix, rel) for nm, ax, ix, rel in plan.lines_of(t)])
    return board


def write_lines(board, plan, want, tiles):
    """file the lines of `tiles` from the board image `want`: `refresh` stages them (nothing, for remote tiles) in parts of at
    most 64 tiles and hands each part to `host_sum`, which overwrites it"""
    tiles = sorted(tiles)
    parts = iter([tiles[k:k + 64] for k in range(0, len(tiles), 64)])

    def fill(buf):
        off = 0
        for t in next(parts):
            buf[off:off + plan.size[t]] = want[plan.start[t]:plan.start[t] + plan.size[t]]
            off += plan.size[t]
        assert off == buf.size
    board.refresh(None, tiles, host_sum=fill)
    assert next(parts, None) is None


def check_case(case, problems):
    plan, n_t = case.plan, case.stub.n_inputs
    want = plan.board(case.tiles)
    board = make_board(plan)
    try:
        write_lines(board, plan, want, range(n_t))
        if not np.array_equal(_bits(board.download()), _bits(want)):
            problems.append((case.name, 'board differs after refresh'))
            return
        everyone = list(range(n_t))
        got0 = board.eval(everyone, [0] * n_t).copy()
        for a in everyone:
            exp = case.expected(0)[a]
            if [int(v) for v in got0[a, :6]] != exp:
                problems.append((case.name, case.stub.tiles_shape[a], 'tile %d full=0' % a, [int(v) for v in got0[a, :6]], exp))
        # rule :274 everywhere for every second tile; the tiles that are not listed keep their words
        some = everyone[::2]
        got1 = board.eval(some, [1] * len(some)).copy()
        for a in everyone:
            exp = case.expected(1)[a] if a in some else [int(v) for v in got0[a, :6]]
            if [int(v) for v in got1[a, :6]] != exp:
                problems.append((case.name, case.stub.tiles_shape[a], 'tile %d full=1' % a if a in some else 'tile %d not listed' % a,
                                 [int(v) for v in got1[a, :6]], exp))
        if not np.array_equal(_bits(board.download()), _bits(want)):
            problems.append((case.name, 'the evaluation wrote to the board'))
    finally:
        board.close()


GROUPS = ['nbhd_', 'self_', 'alone_', 'corner_', 'thin_', 'adoption', 'holes']


@pytest.mark.parametrize('group', GROUPS)
def test_board_evaluation_equals_the_host_rules(group):
    """All tiles remote.  Shapes from 1 x 1 to a perimeter of 40 002 cells: one block of 1024 threads up to a perimeter of
    4096 ((1024, 1024)), two for (1025, 1024), and for (5000, 3300) and (1, 20000) more than 4 cells per thread of the 16 x
    1024 the launch is capped at (4 + a second grid-stride trip); 1-wide and 1-high tiles follow the host rules, where
    index -1 is index 0."""
    cases = [c for c in B.eval_cases() if c.name.startswith(group)]
    assert cases
    problems = []
    for case in cases:
        check_case(case, problems)
    assert not problems, problems[:6]


def test_seventy_tiles_in_one_board():
    """more tiles than one chunk of `refresh` and of pydem_board_eval (64) holds"""
    problems = []
    check_case(B.many_tiles_case(), problems)
    assert not problems, problems[:6]


def test_refresh_of_some_tiles_leaves_the_others():
    """a second refresh with new lines for two tiles: their segments change, every other cell of the board stays"""
    case = {c.name: c for c in B.eval_cases()}['holes']
    plan, n_t = case.plan, case.stub.n_inputs
    want = plan.board(case.tiles)
    board = make_board(plan)
    try:
        write_lines(board, plan, want, range(n_t))
        tiles = [t.copy() for t in case.tiles]
        for t in (2, 4):
            for key, arr in tiles[t].lines.items():
                arr[:] = arr[::-1].copy() if key[0] == 'uca' else ~arr
            tiles[t].reconcile()
        want2 = plan.board(tiles)
        assert not np.array_equal(_bits(want2), _bits(want))
        write_lines(board, plan, want2, [4, 2])
        assert np.array_equal(_bits(board.download()), _bits(want2))
        snap = plan.snap(tiles)
        got = board.eval(list(range(n_t)), [0] * n_t)
        for a in range(n_t):
            assert [int(v) for v in got[a, :6]] == B.expected_scalars(case.stub, a, snap, 0), a
    finally:
        board.close()


# ---------------------------------------------------------------------------------------------- resident tiles
def _resident_setup():
    shapes = [(37, 53), (53, 37), (130, 3)]
    own = 'self'
    table = [
        # rows of one tile feed the left / right strips of another, columns its top / bottom strips; negative indices
        {'left': (1, 0, 5), 'right': (1, 0, -2), 'top': (1, 1, 3), 'bottom': own,
         'top-left': (1, 10, 11, True), 'top-right': (2, 129, 0, True), 'bottom-left': None, 'bottom-right': (1, 0, 36, False)},
        {'left': (0, 0, -1), 'right': (0, 0, 7), 'top': (0, 1, -3), 'bottom': (0, 1, 20),
         'top-left': (0, 36, 52, True), 'top-right': (0, 0, 0, False), 'bottom-left': (2, 64, 1, True), 'bottom-right': (1, 52, 36, True)},
        {'left': own, 'right': (2, 1, -1), 'top': None, 'bottom': (2, 0, 64),
         'top-left': (0, 3, 4, True), 'top-right': None, 'bottom-left': (1, 52, 0, True), 'bottom-right': (2, 128, 1, True)},
    ]
    return shapes, table


def _host_fields(shapes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for t, (n, m) in enumerate(shapes):
        uca = rng.uniform(1.0, 1e6, (n, m))
        uca[rng.random((n, m)) < 0.2] *= 1e9
        for v in (-0.0, np.nan, 5e-324, 1e15 + 0.125):
            uca[rng.integers(0, n), rng.integers(0, m)] = v
            uca[(0, -1)[t % 2], rng.integers(0, m)] = v                # ... and on the lines that are read
        out.append({'uca': uca, 'edge_todo': rng.random((n, m)) < (0.5, 0.9, 0.3)[t], 'edge_done': rng.random((n, m)) < (0.5, 0.2, 0.8)[t]})
    return out


def _take_lines(plan, fields):
    tiles = [B.SparseTile(f['uca'].shape) for f in fields]
    plan.register(tiles)
    for t, tile in enumerate(tiles):
        for (nm, axis, j), arr in tile.lines.items():
            arr[:] = fields[t][nm][j, :] if axis == 0 else fields[t][nm][:, j]
    return tiles


def test_resident_tiles_pack_and_strips():
    """Three resident tiles whose planes are uploaded from numpy (the pipeline does not run: `upload` makes a field resident,
    which is all `set_lines` and `refresh` ask for while the tile has no fix-up state).  The board lines are in a shuffled
    order, not grouped by field.  k_board_pack's strided column gather and its mask -> 0.0 / 1.0 conversion: the board equals
    the numpy lines; k_board_eval writing the strips into the tiles' buffers: all six words equal the model; the staged
    refresh (`refresh_stage` / `refresh_unstage`) with an identity `host_sum` restores a board that was overwritten; one
    line changed on the device and one tile refreshed."""
    from pydem_amd import _ffi
    shapes, table = _resident_setup()
    stub = B.StubManager(shapes, table)
    plan = B.BoardPlan(stub, shuffle=5)
    assert [nm for nm, _, _, _ in plan.lines_of(0)] != sorted(nm for nm, _, _, _ in plan.lines_of(0))
    assert any(ax == 1 for t in range(3) for _, ax, _, _ in plan.lines_of(t)) and any(ix < 0 for t in range(3) for _, _, ix, _ in plan.lines_of(t))
    fields = _host_fields(shapes, 9)
    dev = []
    board = None
    try:
        for t, (n, m) in enumerate(shapes):
            tile = _ffi.Tile(n, m, 0)
            dev.append(tile)
            tile.upload(_ffi.UCA, fields[t]['uca'])
            tile.upload(_ffi.EDGE_TODO, fields[t]['edge_todo'].astype(np.uint8))
            tile.upload(_ffi.EDGE_DONE, fields[t]['edge_done'].astype(np.uint8))
        board = make_board(plan, resident=dict(enumerate(dev)))

        def check(what):
            tiles = _take_lines(plan, fields)
            want = plan.board(tiles)
            assert np.array_equal(_bits(board.download()), _bits(want)), what
            snap = plan.snap(tiles)
            for full in (0, 1):
                got = board.eval([0, 1, 2], [full] * 3)
                for a in range(3):
                    assert [int(v) for v in got[a, :6]] == B.expected_scalars(stub, a, snap, full), (what, a, full)
            return want
        board.refresh(None, [0, 1, 2])
        want = check('pack and scatter')

        def spoil(buf):
            buf[:] = -7.0
        board.refresh(None, [0, 1, 2], host_sum=spoil)
        assert not np.array_equal(_bits(board.download()), _bits(want))
        board.refresh(None, [2, 0, 1], host_sum=lambda buf: None)
        check('staged refresh')
        # a watched row and a watched column of tile 1 change on the device; only tile 1 is refreshed
        fields[1]['edge_done'][5, :] = ~fields[1]['edge_done'][5, :]
        dev[1].set_line(_ffi.EDGE_DONE, 0, 5, fields[1]['edge_done'][5, :].astype(np.uint8))
        fields[1]['uca'][:, 3] = fields[1]['uca'][::-1, 3].copy()
        dev[1].set_line(_ffi.UCA, 1, 3, fields[1]['uca'][:, 3])
        board.refresh(None, [1])
        assert not np.array_equal(_bits(check('one tile refreshed')), _bits(want))
    finally:
        if board is not None:
            board.close()
        for tile in dev:
            tile.close()


# ---------------------------------------------------------------------------------------------- the shipped cross-check
@pytest.mark.parametrize('name', ['pm_cone32_4x5_ov3', 'pm_nansea_2x2_ov2'])
def test_pool_mode_with_the_board_check_switched_on(name, tmp_path, monkeypatch):
    """The device flow of test_pool_mode_device_matches_oracle_backed_flow with PYDEM_BOARD_CHECK=1: after every wave the
    manager compares the evaluation's numbers of every tile with its own rules (`check_against_host_rules`); the queue is off
    on this path, so every wave is host-driven.  Same waves, same masks, same areas as the oracle-backed flow."""
    from oracle_processor import OracleProcessor
    from test_process_manager_cpu import run_pm
    monkeypatch.setenv('PYDEM_BOARD_CHECK', '1')
    g = load_golden(name)
    pm, compact, _ = run_pm(g, str(tmp_path / 'dev'), n_workers=8, tiles_in_flight=2)
    assert pm.edge_queued_batches == 0 and pm.edge_waves > 0
    monkeypatch.delenv('PYDEM_BOARD_CHECK')
    po, compact_o, _ = run_pm(g, str(tmp_path / 'ora'), n_workers=8, processor_cls=OracleProcessor)
    assert (pm.edge_waves, pm.edge_rounds, pm.edge_tiebreaks) == (po.edge_waves, po.edge_rounds, po.edge_tiebreaks)
    for i in range(pm.n_inputs):
        assert np.array_equal(pm.tile_result(i, 'edge_todo'), po.tile_result(i, 'edge_todo')), i
        assert np.array_equal(pm.tile_result(i, 'edge_done'), po.tile_result(i, 'edge_done')), i
        a, b = pm.tile_result(i, 'uca_total'), po.tile_result(i, 'uca_total')
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a, b, rtol=1e-9, atol=1e-12, equal_nan=True), i
    for key in ('uca', 'twi'):
        a, b = compact[key], compact_o[key]
        finite = np.isfinite(a) & np.isfinite(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        assert np.allclose(a[finite], b[finite], rtol=1e-9, atol=1e-12), key
