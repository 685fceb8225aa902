"""What a tile holds on the device after its buffers regrew (csrc/tile_mem.h) against a tile that allocated them once.

Field A is a 64 x 64 cone with one single-cell pit, field B is A with 224 more isolated single-cell pits, so B needs at least
what A needs of every buffer.  One handle runs A and then B (its raw pit views regrow), a second handle runs B only.  Both
must compute the same bytes and report the same pydem_tile_device_bytes: every growth policy is a function of the need
alone, and a regrown block's old size leaves the count."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 64
PITS = [(r, c) for r in range(2, N - 2, 4) for c in range(2, N - 2, 4)]     # 15 x 15 cells, four apart: isolated
PIT_A = PITS[len(PITS) // 2]


def fields():
    r, c = np.mgrid[0:N, 0:N].astype(np.float64)
    cone = 100.0 - np.hypot(r - (N - 1) / 2.0, c - (N - 1) / 2.0)          # falls by at most sqrt(2) per cell, stays above 50
    a, b = cone.copy(), cone.copy()
    a[PIT_A] -= 3.0                                                          # below all eight neighbours
    for p in PITS:
        b[p] -= 3.0
    return a, b


def options(_ffi):
    o = _ffi.Options()
    o.drain_pits = 1
    o.drain_pits_min_border = 0
    o.drain_pits_max_iter = 300
    o.drain_pits_max_dist = 32
    o.drain_pits_max_dist_XY = float('nan')
    o.apply_uca_limit_edges = 0
    o.apply_twi_limits = 0
    o.apply_twi_limits_on_uca = 0
    o.circular_ref_maxcount = 50
    o.uca_saturation_limit = 32.0
    o.twi_min_slope = 1e-3
    o.twi_min_area = float('inf')
    return o


def run(_ffi, tile, z):
    tile.upload(_ffi.ELEV, z)
    tile.set_spacing(np.full(N - 1, 30.0), np.full(N - 1, 30.0), np.full(N, 30.0), np.full(N, 30.0))
    tile.slopes_directions()
    tile.uca(options(_ffi))
    return tile.timings()['n_pits'], tile.download(_ffi.UCA), tile.device_bytes()


def test_regrown_tile_matches_a_fresh_one():
    from pydem_amd import _ffi
    a, b = fields()
    assert len(PITS) - 1 >= 200 and (b <= a).all() and int((b < a).sum()) == len(PITS) - 1
    grown, fresh = _ffi.Tile(N, N), _ffi.Tile(N, N)
    pits_a, _, bytes_a = run(_ffi, grown, a)
    pits_b, uca_grown, bytes_grown = run(_ffi, grown, b)
    pits_f, uca_fresh, bytes_fresh = run(_ffi, fresh, b)
    print('n_pits A %d, B %d (fresh handle %d); device_bytes after A %d, after A then B %d, after B alone %d (difference %d)'
          % (pits_a, pits_b, pits_f, bytes_a, bytes_grown, bytes_fresh, bytes_grown - bytes_fresh))
    assert pits_b > pits_a >= 1 and pits_f == pits_b          # the raw pit views of the first handle regrew
    assert uca_grown.tobytes() == uca_fresh.tobytes()
    assert bytes_grown == bytes_fresh
    grown.close(); fresh.close()
