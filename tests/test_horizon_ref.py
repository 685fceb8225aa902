"""CPU tier: the ray table (horizon.ray_table) and the numpy twin of pydem_horizon (horizon.horizon_ref) against answers that do
not come from them: the cell sequences of the axes and diagonals, a turned table, an inclined integer plane, a flat tile, a wall, a
tower's shadow, no data, the border bands of edge_nan, and a rotated field."""
import math

import numpy as np
import pytest

from pydem_amd import horizon as H


def _dir(table, d):
    lo, hi = int(table.start[d]), int(table.start[d + 1])
    return table.dr[lo:hi].astype(int), table.dc[lo:hi].astype(int), table.w[lo:hi]


def _dist(dr, dc, gx, gy):
    return np.sqrt((dc * gx) ** 2 + (dr * gy) ** 2)


# ---- the table ----

def test_eight_rays_on_square_cells_are_the_axes_and_diagonals():
    g = 4.0
    t = H.ray_table(8, 0.0, 10 * g, g, g)
    assert t.start.dtype == np.int32 and t.dr.dtype == np.int16 and t.dc.dtype == np.int16 and t.w.dtype == np.float64
    assert list(t.azimuths) == [0.0, 45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0]
    unit = [(-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1)]       # N NE E SE S SW W NW as (row, column)
    for d, (ur, uc) in enumerate(unit):
        dr, dc, w = _dir(t, d)
        steps = 10 if 0 in (ur, uc) else 7                          # 7 * sqrt(2) < 10 < 8 * sqrt(2)
        k = np.arange(1, steps + 1)
        assert np.array_equal(dr, k * ur) and np.array_equal(dc, k * uc), d
        if 0 in (ur, uc):
            assert np.array_equal(w, 1.0 / (k * g)), d
        else:
            assert np.allclose(1.0 / w, k * g * math.sqrt(2.0), rtol=4e-16, atol=0), d
    assert int(t.start[-1]) == 4 * 10 + 4 * 7 == t.w.size


@pytest.mark.parametrize('n_dir, az0', [(5, 11.25), (16, 0.0), (3, -30.0), (7, 22.5)])
def test_a_table_turned_by_90_degrees_is_the_turned_table(n_dir, az0):
    a, b = H.ray_table(n_dir, az0, 37.0, 1.5, 1.5, 2.0), H.ray_table(n_dir, az0 + 90.0, 37.0, 1.5, 1.5, 2.0)
    assert np.array_equal(a.start, b.start) and a.start[-1] > 20 * n_dir
    assert np.array_equal(b.dr, a.dc) and np.array_equal(b.dc, -a.dr)
    assert a.w.tobytes() == b.w.tobytes()


def test_steps_stop_at_max_dist_and_the_next_one_would_pass_it():
    gx, gy, md = 3.0, 2.0, 50.0
    short, long_ = H.ray_table(16, 7.0, md, gx, gy), H.ray_table(16, 7.0, 2 * md, gx, gy)
    for d in range(16):
        dr, dc, w = _dir(short, d)
        Dr, Dc, W = _dir(long_, d)
        cnt = dr.size
        assert cnt >= 10 and Dr.size > cnt
        assert np.array_equal(Dr[:cnt], dr) and np.array_equal(Dc[:cnt], dc) and np.array_equal(W[:cnt], w)
        dist = _dist(Dr, Dc, gx, gy)
        assert (dist[:cnt] <= md).all() and dist[cnt] > md
        assert np.array_equal(W, 1.0 / dist)
        assert (np.diff(dist) >= 0).all() and (np.abs(np.diff(Dr)) <= 1).all() and (np.abs(np.diff(Dc)) <= 1).all()
        assert np.maximum(np.abs(Dr), np.abs(Dc)).tolist() == list(range(1, Dr.size + 1))


def test_default_max_dist_and_z_factor():
    t = H.ray_table(4, 0.0, None, 3.0, 2.0, 0.5)
    assert np.diff(t.start).tolist() == [100, 66, 100, 66]         # 100 * min(gx, gy) = 200 ground units
    dr, dc, w = _dir(t, 1)
    assert np.array_equal(w, 0.5 / (3.0 * np.arange(1, 67)))


def test_wide_cells_take_two_rows_per_column_at_45_degrees():
    t = H.ray_table(1, 45.0, 30.0, 2.0, 1.0)
    dr, dc, w = _dir(t, 0)
    k = np.arange(1, dr.size + 1)
    assert dr.size >= 12
    assert np.array_equal(dr, -k) and np.array_equal(dc, (k + 1) // 2)      # halves round away from zero: 1 1 2 2 3 3 ...
    west = _dir(H.ray_table(1, 225.0, 30.0, 2.0, 1.0), 0)
    assert np.array_equal(west[0], k) and np.array_equal(west[1], -((k + 1) // 2))


def test_the_step_limit():
    t = H.ray_table(1, 0.0, 1024.0, 1.0, 1.0)
    assert int(t.start[-1]) == 1024
    with pytest.raises(ValueError):
        H.ray_table(1, 0.0, 1025.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        H.ray_table(8, 0.0, 1500.0, 1.0, 1.0)                       # the diagonals fit (1060 cells), the axes do not
    assert int(H.ray_table(4, 45.0, 1440.0, 1.0, 1.0).start[-1]) == 4 * 1018
    none = H.ray_table(8, 0.0, 0.5, 1.0, 1.0)
    assert none.start.tolist() == [0] * 9 and none.w.size == 0
    out, count = H.horizon_ref(np.arange(12.0).reshape(3, 4), none)
    assert (out['horizon'] == 0).all() and (out['svf'] == 1.0).all() and count == 12


# ---- the twin ----

def test_inclined_integer_plane():
    """z = a * col + b * row on cells of 2 x 2: the step k of a ray rises k times the first step's rise over k times its distance.
    On the axes the distance k g and the rise are exact, every sample's product gives the slope a / g or b / g exactly for the
    eleven steps used here, and so does their maximum.  On the diagonals the distance k g sqrt(2) is rounded: a product carries the
    roundings of the square root, of the division that makes the weight and of the multiplication, 3 * 2^-53 at most, and the closed
    form the test compares with another three (square root, product, division): 6 * 2^-53 < 7e-16 in all, which bounds how far the
    maximum of the products may stand from it."""
    a, b, g = 3.0, -5.0, 2.0
    n, m = 24, 28
    z = a * np.arange(m)[None, :] + b * np.arange(n)[:, None]
    one = H.ray_table(8, 0.0, 1.5 * g, g, g)
    far = H.ray_table(8, 0.0, 8.0 * g * math.sqrt(2.0), g, g)
    assert np.diff(one.start).tolist() == [1] * 8 and np.diff(far.start).tolist() == [11, 8] * 4
    near_planes = H.horizon_ref(z, one, edge_nan=False)[0]['horizon']
    far_planes = H.horizon_ref(z, far, edge_nan=False)[0]['horizon']
    closed = {0: -b / g, 2: a / g, 4: b / g, 6: -a / g}             # north (row falls), east, south, west
    for d in range(8):
        ur, uc, w1 = int(one.dr[d]), int(one.dc[d]), float(one.w[d])
        want = max(0.0, (a * uc + b * ur) * w1)
        inner = (slice(1, n - 1), slice(1, m - 1))                  # every cell there has its first step on the tile
        assert (near_planes[d][inner] == want).all(), d
        if d in closed:
            assert want == max(0.0, closed[d])
            assert (far_planes[d][inner] == want).all(), d
        else:
            slope = max(0.0, (a * uc + b * ur) / (g * math.sqrt(2.0)))
            assert slope > 0 or (far_planes[d][inner] == 0).all(), d
            assert np.allclose(far_planes[d][inner], slope, rtol=7e-16, atol=0), d
            assert (far_planes[d][8:-8, 8:-8] == far_planes[d][8, 8]).all(), d     # the same eight samples, the same maximum
    # a cell in the far corner of a direction has no sample at all: 0, not NaN, without edge_nan
    assert far_planes[0][0, 5] == 0 and far_planes[2][5, m - 1] == 0


def test_flat_tile():
    z = np.full((20, 31), 7.0)
    for edge_nan in (False, True):
        out, count = H.horizon_ref(z, H.ray_table(16, 3.0, 6.0, 1.0, 2.0), edge_nan)
        T, svf = out['horizon'], out['svf']
        ok = ~np.isnan(svf)
        assert (T[:, ok] == 0).all() and (svf[ok] == 1.0).all() and count == ok.sum()
        assert ok.all() if not edge_nan else (ok[6:-6, 6:-6].all() and not ok[0].any())


def _wall(nan_at=None):
    H_, g, c0 = 8.0, 3.0, 30
    z = np.zeros((9, 40))
    z[:, c0] = H_
    if nan_at is not None:
        z[nan_at] = np.nan
    return z, H_, g, c0


def test_wall():
    z, H_, g, c0 = _wall()
    t = H.ray_table(4, 0.0, 10 * g, g, g)
    T = H.horizon_ref(z, t, edge_nan=False)[0]['horizon']
    east = T[1]
    for c in range(z.shape[1]):
        want = H_ / ((c0 - c) * g) if 1 <= c0 - c <= 10 else 0.0
        assert (east[:, c] == want).all(), c
    assert (T[3][:, c0 + 1:c0 + 10] > 0).all() and (T[3][:, :c0 + 1] == 0).all()       # looking west from east of the wall
    assert (T[0][1:] == 0).all() and (T[2][:-1] == 0).all()


def test_no_data_does_not_obstruct_and_is_nan_itself():
    z, H_, g, c0 = _wall(nan_at=(4, 28))
    t = H.ray_table(4, 0.0, 10 * g, g, g)
    out, count = H.horizon_ref(z, t, edge_nan=False)
    east = out['horizon'][1]
    assert east[4, 25] == H_ / (5 * g) and east[4, 27] == H_ / (3 * g)
    assert np.isnan(out['horizon'][:, 4, 28]).all() and np.isnan(out['svf'][4, 28])
    assert np.isnan(out['horizon']).sum() == 4 and np.isnan(out['svf']).sum() == 1 and count == z.size - 1
    plain = H.horizon_ref(_wall()[0], t, edge_nan=False)[0]['horizon']
    keep = np.ones(z.shape, bool)
    keep[4, 28] = False
    # the NaN is lower than nothing and hides nothing: every other cell is what it is without it, except that the cells beside
    # it no longer see the zero plane there, which never raised a tangent anyway
    assert np.array_equal(out['horizon'][:, keep], plain[:, keep])


def test_edge_nan_bands():
    n, m, gx, gy = 40, 50, 2.0, 3.0
    rng = np.random.default_rng(5)
    z = rng.random((n, m)) * 30.0
    z[7, 9] = np.nan
    t = H.ray_table(16, 0.0, 20.0, gx, gy)
    out, count = H.horizon_ref(z, t, edge_nan=True)
    union = np.isnan(z)
    rows, cols = np.arange(n)[:, None, None], np.arange(m)[None, :, None]
    for d in range(16):
        dr, dc, _ = _dir(t, d)
        top, bottom, left, right = max(0, -dr.min()), max(0, dr.max()), max(0, -dc.min()), max(0, dc.max())
        assert 6 <= max(top, bottom, left, right) <= 10             # 20 ground units: 10 cells of 2 east, 6 cells of 3 north
        band = np.zeros((n, m), bool)
        band[:top] = True
        band[n - bottom:] = True
        band[:, :left] = True
        band[:, m - right:] = True
        # the same band, cell by cell and step by step
        leaves = ((rows + dr < 0) | (rows + dr >= n) | (cols + dc < 0) | (cols + dc >= m)).any(axis=2)
        assert np.array_equal(band, leaves), d
        assert np.array_equal(np.isnan(out['horizon'][d]), band | np.isnan(z)), d
        union |= band
    assert np.array_equal(np.isnan(out['svf']), union) and count == (~union).sum() > 0
    off, count = H.horizon_ref(z, t, edge_nan=False)
    assert np.array_equal(np.isnan(off['svf']), np.isnan(z)) and count == z.size - 1
    assert all(np.array_equal(np.isnan(p), np.isnan(z)) for p in off['horizon'])
    # where a direction is complete, both settings agree
    ok = ~np.isnan(out['horizon'])
    assert np.array_equal(out['horizon'][ok], off['horizon'][ok])


def test_defined_cells_without_an_svf_are_those_with_every_tangent_finite():
    z = np.random.default_rng(2).random((30, 30))
    z[3, 4] = np.nan
    t = H.ray_table(8, 0.0, 5.0)
    both, c_both = H.horizon_ref(z, t)
    hor, c_hor = H.horizon_ref(z, t, want_svf=False)
    svf, c_svf = H.horizon_ref(z, t, want_horizon=False)
    assert list(hor) == ['horizon'] and list(svf) == ['svf'] and c_both == c_hor == c_svf == 20 * 20
    assert np.array_equal(hor['horizon'], both['horizon'], equal_nan=True) and np.array_equal(svf['svf'], both['svf'], equal_nan=True)
    assert c_hor == np.isfinite(both['horizon']).all(axis=0).sum()


def test_svf_is_the_mean_of_cos2_summed_in_ascending_direction():
    z = np.random.default_rng(11).random((25, 27)) * 40.0
    t = H.ray_table(5, 10.0, 9.0, 1.0, 1.5)
    out, _ = H.horizon_ref(z, t, edge_nan=False)
    acc = np.zeros(z.shape)
    for d in range(5):
        acc = acc + 1.0 / (1.0 + out['horizon'][d] * out['horizon'][d])
    assert np.array_equal(out['svf'], acc / 5.0)
    assert np.allclose(out['svf'], (np.cos(np.arctan(out['horizon'])) ** 2).mean(axis=0), rtol=1e-13)
    assert (out['svf'] < 1).any() and (out['svf'] > 0).all() and (out['horizon'] >= 0).all()


def test_tower_shadow():
    Ht, alt, r0, c0 = 10.0, 30.0, 3, 10
    z = np.zeros((7, 60))
    z[r0, c0] = Ht
    reach = Ht / math.tan(math.radians(alt))                        # 17.32 cells of 1 x 1
    shadow = H.cast_shadow_ref(z, 270.0, alt, 40.0, 1.0, 1.0, edge_nan=False)     # the sun due west: shadows fall to the east
    want = np.ones(z.shape)
    for c in range(z.shape[1]):
        if 0 < c - c0 < reach:
            want[r0, c] = 0.0
    assert want[r0].tolist().count(0.0) == 17
    assert np.array_equal(shadow, want)
    # a sun too high for the second cell; a ray too short for the shadow's end; no data
    assert H.cast_shadow_ref(z, 270.0, 85.0, 40.0, edge_nan=False).sum() == z.size - 0
    assert (H.cast_shadow_ref(z, 270.0, alt, 5.0, edge_nan=False) == 0).sum() == 5
    z[r0, c0 + 2] = np.nan
    s = H.cast_shadow_ref(z, 270.0, alt, 40.0, edge_nan=False)
    assert np.isnan(s[r0, c0 + 2]) and (s == 0).sum() == 16 and s[r0, c0 + 3] == 0
    edge = H.cast_shadow_ref(z, 270.0, alt, 40.0, edge_nan=True)
    assert np.isnan(edge[:, :40]).all() and np.array_equal(edge[:, 40:], s[:, 40:], equal_nan=True)


@pytest.mark.parametrize('edge_nan', [False, True])
def test_a_rotated_field_rotates_the_stack(edge_nan):
    rng = np.random.default_rng(9)
    z = rng.random((23, 31)) * 50.0
    z[5, 6] = z[17, 20] = np.nan
    t = H.ray_table(8, 0.0, 6.5, 2.0, 2.0)
    plain, c_plain = H.horizon_ref(z, t, edge_nan)
    turned, c_turned = H.horizon_ref(np.rot90(z), t, edge_nan)
    assert c_plain == c_turned > 0
    for d in range(8):
        # np.rot90 turns the field counter-clockwise: what lay at the azimuth a + 90 now lies at a
        assert np.array_equal(turned['horizon'][d], np.rot90(plain['horizon'][(d + 2) % 8]), equal_nan=True), d
    ok = ~np.isnan(turned['svf'])
    assert np.array_equal(ok, ~np.isnan(np.rot90(plain['svf'])))
    assert np.allclose(turned['svf'][ok], np.rot90(plain['svf'])[ok], rtol=1e-15)       # (the sum starts at another direction)
