"""GPU tier: pydem_fill_depressions and pydem_depressions above the sizes that the small tiles of tests/test_gpu_fill_depressions.py and
tests/test_gpu_depressions.py never reach, against the exact references of tests/large_depression_fields.py (held against the host
twins by tests/test_large_depression_fields.py).  One tile size, chosen so that the kernels launched on the capped grid of 8192
workgroups (k_fd_init, k_fd_final, k_dp_init, k_dp_stats) take three trips, the last one partial, and the fixed-point sums have
B = 39 fraction bits instead of 40.  The mosaic brings tens of thousands of depressions at every phase of the 32 x 32 blocks, the
great lake one depression of 4.4 M cells whose integer area sum passes 2**60.  Bytes and array_equal throughout."""
import math

import numpy as np
import pytest

import large_depression_fields as L
from depression_checks import same

pytestmark = pytest.mark.gpu

N, M = 2100, 2100
CAP = 8192 * 256            # cells of one trip of the capped grid (depressions.hip, fill_depressions.hip: gcells)
SMALL_LAKE = (300, 300)     # the lake the host twin follows (the outlet case)


def tile_shape():
    """the size, with the thresholds the tests below depend on"""
    assert 2 * CAP < N * M < 3 * CAP and (N * M) % CAP % 256 != 0       # three trips, the last partial down to its last workgroup
    assert N * M > 2 ** 22                                               # B = 62 - 23 = 39
    return N, M


def quanta_b39(ra, depth_max):
    """the quanta of B = 39 fraction bits, written out"""
    amax = float(ra.max())
    return (math.ldexp(1.0, math.frexp(amax)[1] - 39), math.ldexp(1.0, math.frexp(depth_max * amax)[1] - 39))


def device_fill(z, eps):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0)
    W, depth = dp.calc_fill_depressions(eps, return_depth=True)
    return W, depth, dp.fill_depressions_stats


def device_inventory(z, outlets=None, **kw):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=z, **L.spacing(z.shape[0]))
    res = dp.calc_depressions(outlets, **kw)
    return res, dp.depressions_stats


def check_fill(z, want, eps_used, W, depth, st):
    assert st['epsilon'] == eps_used
    assert W.dtype == np.float64 and W.tobytes() == want.tobytes()
    d = want - z
    assert depth.tobytes() == d.tobytes()
    with np.errstate(invalid='ignore'):
        up = want > z
    assert st['n_raised'] == int(up.sum()) and st['max_depth'] == float(d[up].max())
    assert st['passes'] >= 2


# 1. the mosaic
@pytest.mark.parametrize('eps', [0.0, None])
def test_fill_on_the_mosaic(eps):
    mo = L.mosaic(*tile_shape())
    W, depth, st = device_fill(mo.z, eps)
    check_fill(mo.z, mo.fill(eps), mo.epsilon(eps), W, depth, st)
    assert st['n_raised'] >= 400000                     # the input has not silently become trivial


def test_inventory_on_the_mosaic():
    mo = L.mosaic(*tile_shape())
    ra = L.row_area(N)
    want = mo.inventory(ra)
    K = len(want[1])
    assert K >= 20000 and K == mo.labels()[1]
    assert len(mo.placements) >= 400 and len({(r % 32, c % 32) for _, r, c in mo.placements}) >= 200
    res, st = device_inventory(mo.z)
    same(res, want, st)
    assert st['n_found'] == K
    with np.errstate(invalid='ignore'):
        assert st['quanta'] == quanta_b39(ra, float((mo.fill(0.0) - mo.z)[want[0] > 0].max()))


def test_inventory_on_the_mosaic_without_the_local_step(monkeypatch):
    mo = L.mosaic(*tile_shape())
    want = mo.inventory(L.row_area(N))
    monkeypatch.setenv('PYDEM_DEPR_LOCAL', '0')
    res, st = device_inventory(mo.z)
    same(res, want, st)
    assert st['n_found'] == len(want[1])


def test_filters_on_the_mosaic():
    mo = L.mosaic(*tile_shape())
    full = mo.inventory(L.row_area(N))
    kw = dict(min_depth=2.0, min_cells=2)
    want = L.filtered(full, **kw)
    assert 0 < len(want[1]) < len(full[1])
    res, st = device_inventory(mo.z, **kw)
    same(res, want, st)
    assert st['n_found'] == len(full[1])
    kw = dict(min_depth=0.0, min_cells=2)               # a lookup with many kept ids
    want = L.filtered(full, **kw)
    assert 1000 < len(want[1]) < len(full[1])
    res, st = device_inventory(mo.z, **kw)
    same(res, want, st)
    assert st['n_found'] == len(full[1])


# 2. the great lake
def test_inventory_of_the_great_lake():
    n, m = tile_shape()
    lake = L.great_lake(n, m)
    ra = L.row_area(n)
    want = lake.inventory(ra)
    area_sum, volume_sum, quanta = lake.sums(ra)
    assert 2 ** 60 < area_sum < 2 ** 62 and volume_sum < 2 ** 62        # the no-overflow argument, at scale
    assert quanta == quanta_b39(ra, lake.S - float(lake.z.min()))
    res, st = device_inventory(lake.z)
    same(res, want, st)
    t = res['table']
    assert st['n_found'] == 1 and len(t) == 1 and t['cells'][0] == (n - 2) * (m - 2)
    assert t['area'].tobytes() == np.float64(float(area_sum) * quanta[0]).tobytes()
    assert t['volume'].tobytes() == np.float64(float(volume_sum) * quanta[1]).tobytes()
    for col, terms, q in zip(('area', 'volume'), lake.terms(ra), quanta):
        assert abs(t[col][0] - math.fsum(terms.tolist())) <= lake.cells * q / 2, col


def test_fill_of_the_great_lake():
    n, m = tile_shape()
    lake = L.great_lake(n, m)
    W, depth, st = device_fill(lake.z, 0.0)
    check_fill(lake.z, lake.W, 0.0, W, depth, st)
    assert st['n_raised'] == (n - 2) * (m - 2) and st['max_depth'] == lake.S - float(lake.z.min())


def test_an_outlet_at_the_bottom_of_a_lake():
    """The closed form does not hold with an outlet inside the lake: the host twin is the reference, on a lake it can follow."""
    from pydem_amd import conditioning
    n, m = SMALL_LAKE
    lake = L.great_lake(n, m)
    ra = L.row_area(n)
    b = lake.inventory(ra)[1]
    bottom = (int(b['bottom_row'][0]), int(b['bottom_col'][0]))
    out = np.zeros((n, m), bool)
    out[bottom] = True
    want = conditioning.label_depressions(lake.z, out, dX2dY2=ra)
    res, st = device_inventory(lake.z, [bottom])
    same(res, want, st)
    assert res['label'][bottom] == 0 and len(res['table']) > 1 and res['table']['cells'].sum() < lake.cells
