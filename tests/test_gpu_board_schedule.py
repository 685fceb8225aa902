"""The wave selection on the device (k_sched_select, k_sched_settle, the gated copy kernels and the evaluation between two
waves; pydem_amd/csrc/comm.hip) against `board_model.ScheduleModel`, the host wave loop of
`_process_uca_edges_pool_device` restated on the numbers of the host strip rules.

All tiles are remote and the test plays the ranks that own them: `Board.run_waves(None, k, state, exchange=obj)` hands `obj`
the member word of every wave and the staging buffer, and `obj` writes the members' new lines into it -- the tile's next
round according to the case's script.  After every batch the schedule words, the scalars of all tiles and the board must
equal the model exactly.  tests/test_board_model.py asserts, on the CPU, that the scripts produce wide waves, suppressed
candidates, tie-breaks, all three stop reasons, full batches and a stale diagonal metric."""
import numpy as np
import pytest

import board_model as B
from test_gpu_board_eval import _bits, make_board, write_lines

pytestmark = pytest.mark.gpu


class Owner(object):
    """The ranks that own the tiles.  The staging layout is the one pydem_board_prepare_waves builds and the ranks exchange
    (tiles in index order, lines in `set_lines` order, every line padded to 8 bytes, areas as doubles, masks as bytes), so
    a caller that sums the buffer may rely on it -- `BoardPlan.staging` restates it."""

    def __init__(self, case):
        self.case = case
        self.tiles = case.initial()
        self.runs = [0] * case.n_t
        self.where, self.n_bytes = case.plan.staging()
        self.members = 0
        self.waves = []

    def max_inplace(self, probe):
        # (members low / high half, waves so far, stop reason -- and their negatives: one rank, nothing to reduce)
        assert probe.size == 8 and all(probe[q] == -probe[q + 1] for q in range(0, 8, 2))
        self.members = int(probe[0]) | (int(probe[2]) << 32)

    def sum_bytes_inplace(self, buf):
        assert buf.dtype == np.uint8 and buf.size == self.n_bytes
        assert not buf.any()                          # nobody on this device owns a tile
        if self.members:
            self.waves.append(self.members)
        for t in range(self.case.n_t):
            if not (self.members >> t) & 1:
                continue
            self.case.script(self.tiles[t], t, self.runs[t])
            self.runs[t] += 1
            for req in self.case.plan.order[t]:
                v = self.tiles[t].line(req[1], req[2], req[3])
                raw = np.ascontiguousarray(v, np.float64).view(np.uint8) if req[1] == 'uca' else v.astype(np.uint8)
                buf[self.where[req]:self.where[req] + raw.size] = raw


@pytest.mark.parametrize('name', [c.name for c in B.schedule_cases()])
def test_queued_waves_equal_the_host_schedule(name):
    from pydem_amd import _ffi
    S = _ffi.Board
    case = {c.name: c for c in B.schedule_cases()}[name]
    plan, n_t = case.plan, case.n_t
    owner = Owner(case)
    model = B.ScheduleModel(plan, case.initial(), case.script)
    board = make_board(plan)
    try:
        write_lines(board, plan, plan.board(owner.tiles), range(n_t))
        scal = board.eval(list(range(n_t)), [0] * n_t).copy()
        assert [[int(v) for v in scal[a, :6]] for a in range(n_t)] == model.scal
        state = np.zeros(S.SCH_WORDS, np.uint64)
        for a in range(n_t):                          # as the manager sets them
            state[S.SCH_READERS + a] = sum(1 << r for r in plan.readers[a])
            state[S.SCH_NBRS + a] = sum(1 << r for r in plan.nbrs[a])
            state[S.SCH_ND + a], state[S.SCH_PD + a] = model.nd[a], model.pd[a]
        stops = []
        for k, ok, limit in case.steps():
            state[S.SCH_OK], state[S.SCH_LIMIT] = ok, limit
            seen = len(owner.waves)
            before_board, before_scal = board.download(), scal
            n_waves, stop, log, ntb, tblog = model.batch(k, ok, limit)
            scal = board.run_waves(None, k, state, exchange=owner).copy()
            what = (name, len(stops), k, ok, limit)
            assert (int(state[S.SCH_NWAVES]), int(state[S.SCH_STOP])) == (n_waves, stop), what
            assert [int(state[S.SCH_LOG + w]) for w in range(n_waves)] == log == owner.waves[seen:], what
            assert (int(state[S.SCH_NTB]), int(state[S.SCH_TBLOG])) == (ntb, tblog), what
            assert [int(state[S.SCH_ND + a]) for a in range(n_t)] == model.nd, what
            assert [int(state[S.SCH_PD + a]) for a in range(n_t)] == model.pd, what
            assert [a for a in range(n_t) if int(state[S.SCH_HAS + a])] == sorted(model.last_hash), what
            assert all(int(state[S.SCH_HASH + a]) == h for a, h in model.last_hash.items()), what
            assert [[int(v) for v in scal[a, :6]] for a in range(n_t)] == model.scal, what
            after = board.download()
            assert np.array_equal(_bits(after), _bits(plan.board(model.tiles))), what
            if n_waves == 0:                          # a batch that stops at once leaves everything as it was
                assert np.array_equal(_bits(after), _bits(before_board)) and np.array_equal(scal, before_scal), what
            stops.append(stop)
            if stop == 1:
                break
        assert stops[-1] == 1 and owner.runs == model.runs
    finally:
        board.close()
