"""GPU tier: pydem_terrain_attributes (csrc/terrain.hip) through DEMProcessor.calc_terrain_attributes against its numpy twin
(pydem_amd/terrain.py: terrain_attributes_ref), for half widths 1 (the marching kernel), 2 and 7 (the LDS kernel at its smallest
and largest window).

What is compared how: dzdx, dzdy, the NaN pattern of every plane and n_defined exactly; the aspect, which passes through atan2,
within 4 ulp and exactly -1 where the twin is -1; the planes that pass through sqrt (gradient, the curvatures, hillshade) bit
for bit -- the build has no fast-math and no contraction, and fp64 division and square root are correctly rounded.

Then the same bytes from a second call, from one plane at a time, from k = 1 through the general path (PYDEM_TA_GENERIC=1) and
from a child process under PYDEM_MEM_POISON; the tile's fields, graph and timings unchanged by the call and calc_uca after it
giving the bits it gives without it; the argument errors, which allocate and launch nothing.

The library holds no tile under 3 x 3, so the shape (2k, 9) at k = 1 -- two rows -- is answered by DEMProcessor without a launch
(all NaN, n_defined 0); at k = 2 and 7 the same case runs on the device."""
import functools

import numpy as np
import pytest

import flowgraph_kit as K
from flowgraph_kit import assert_same_bits, bits

pytestmark = pytest.mark.gpu

HALF_WIDTHS = (1, 2, 7)
SEED = 7
STEP = 100.0            # the terrace height: coarse enough for windows of 15 x 15 equal cells on the larger tiles
BIG = ((96, 80), (70, 130))     # last blocks partly filled in both directions; windows straddle the block seams


def _shapes(k):
    return ((2 * k + 1, 2 * k + 1), (2 * k, 9), (5, 7), (64, 64)) + BIG


def _spacing(n, varying):
    if not varying:
        return dict(dX=30.0, dY=20.0)
    row = np.arange(n, dtype=np.float64)
    dX2 = 30.0 * np.cos(np.radians(40.0 + 0.01 * row))              # a geographic tile: the cell narrows with the latitude
    return dict(dX=(dX2[:-1] + dX2[1:]) / 2, dY=np.full(n - 1, 20.0), dX2=dX2, dY2=np.full(n, 20.0))


@functools.lru_cache(maxsize=None)
def _field(shape, kind, k):
    from pydem_amd import synth
    n, m = shape
    z = synth.fractal(n, m, seed=SEED, top_shift=7, n_octaves=7)
    if kind == 'terraced':
        z = np.floor(z / STEP) * STEP
    if kind == 'specks':
        rng = np.random.default_rng(3)
        z[rng.integers(0, n, 6), rng.integers(0, m, 6)] = np.nan
        # the corner of a block of either kernel: 64 columns x (30 - 2k) rows, and 62 columns x 64 rows
        for cell in ((30 - 2 * k, 64), (64, 62), (0, 0), (n - 1, m - 1)):
            if cell[0] < n and cell[1] < m:
                z[cell] = np.nan
    z.setflags(write=False)
    return z


def _dp(z, varying=False):
    from pydem_amd import DEMProcessor
    return DEMProcessor(elev=z, fill_flats=False, drain_pits_path=False, **_spacing(z.shape[0], varying))


@functools.lru_cache(maxsize=None)
def _twin(shape, kind, k, varying=False):
    """the twin's planes and count for all nine attributes, computed once per case"""
    from pydem_amd import terrain as T
    z = _field(shape, kind, k)
    dp = _dp(z, varying)
    out, count = T.terrain_attributes_ref(z, dp.dX2, dp.dY2, 2 * k + 1, T.ATTRIBUTES, T.light_vector(300.0, 35.0), 1.5)
    for v in out.values():
        v.setflags(write=False)
    return out, count


def _device(z, k, which=None, varying=False):
    from pydem_amd import terrain as T
    dp = _dp(z, varying)
    out = dp.calc_terrain_attributes(which or T.ATTRIBUTES, 2 * k + 1, azimuth=300.0, altitude=35.0, z_factor=1.5)
    assert out is dp.terrain_attributes and dp.terrain_attributes_stats['window'] == 2 * k + 1
    return dp, out


def _hold(out, stats, ref, count, what):
    assert stats['n_defined'] == count, (what, stats['n_defined'], count)
    for nm, want in ref.items():
        if nm not in out:
            continue
        got = out[nm]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), "%s %s: NaN patterns differ" % (what, nm)
        if nm == 'aspect':
            ok = ~np.isnan(want)
            flat = ok & (want == -1)
            assert (got[flat] == -1).all() and not (got[ok & ~flat] == -1).any(), "%s: the flats of the aspect differ" % what
            err = np.abs(got[ok] - want[ok])
            assert (err <= 4 * np.spacing(np.abs(want[ok]))).all(), "%s aspect: worst %.3g ulp" % (what, (err / np.spacing(np.abs(want[ok]))).max())
        else:
            assert_same_bits(got, want, "%s %s" % (what, nm))
    assert int((~np.isnan(next(iter(out.values())))).sum()) == count


@pytest.mark.parametrize('k', HALF_WIDTHS)
def test_fractal_tiles_of_every_shape(k):
    for shape in _shapes(k):
        ref, count = _twin(shape, 'fractal', k)
        dp, out = _device(_field(shape, 'fractal', k), k)
        _hold(out, dp.terrain_attributes_stats, ref, count, "fractal %r k=%d" % (shape, k))
        if shape == (2 * k + 1, 2 * k + 1):
            assert count == 1
        if shape in ((2 * k, 9), (5, 7)) and min(shape) < 2 * k + 1:
            assert count == 0 and dp.terrain_attributes_stats['n_defined'] == 0


@pytest.mark.parametrize('k', HALF_WIDTHS)
@pytest.mark.parametrize('shape', BIG)
def test_no_data_specks(shape, k):
    ref, count = _twin(shape, 'specks', k)
    assert np.isnan(_field(shape, 'specks', k)).sum() >= 8 and 0 < count < (shape[0] - 2 * k) * (shape[1] - 2 * k)
    dp, out = _device(_field(shape, 'specks', k), k)
    _hold(out, dp.terrain_attributes_stats, ref, count, "specks %r k=%d" % (shape, k))


@pytest.mark.parametrize('k', HALF_WIDTHS)
@pytest.mark.parametrize('shape', BIG)
def test_terraces_have_flat_windows(shape, k):
    ref, count = _twin(shape, 'terraced', k)
    flat = ref['aspect'] == -1
    assert flat.any() and (ref['gradient'][flat] == 0).all() and (ref['profile'][flat] == 0).all()      # the twin takes the branch
    assert (ref['aspect'] >= 0).any()
    dp, out = _device(_field(shape, 'terraced', k), k)
    _hold(out, dp.terrain_attributes_stats, ref, count, "terraced %r k=%d" % (shape, k))
    for nm in ('gradient', 'profile', 'plan', 'tangential'):
        assert (out[nm][flat] == 0).all()


@pytest.mark.parametrize('k', HALF_WIDTHS)
def test_spacing_that_varies_per_row(k):
    shape = BIG[0]
    ref, count = _twin(shape, 'fractal', k, True)
    assert not np.array_equal(ref['dzdx'], _twin(shape, 'fractal', k)[0]['dzdx'], equal_nan=True)
    dp, out = _device(_field(shape, 'fractal', k), k, varying=True)
    _hold(out, dp.terrain_attributes_stats, ref, count, "varying spacing k=%d" % k)


@pytest.mark.parametrize('k', HALF_WIDTHS)
def test_same_bytes_again_and_plane_by_plane(k):
    from pydem_amd import terrain as T
    shape = BIG[1]
    z = _field(shape, 'specks', k)
    dp, out = _device(z, k)
    first = {nm: bits(v) for nm, v in out.items()}
    held = dp._tile.device_bytes()
    again = dp.calc_terrain_attributes(T.ATTRIBUTES, 2 * k + 1, azimuth=300.0, altitude=35.0, z_factor=1.5)
    assert {nm: bits(v) for nm, v in again.items()} == first
    assert dp._tile.device_bytes() == held                          # the block is kept, not taken again
    for nm in T.ATTRIBUTES:
        one = dp.calc_terrain_attributes((nm,), 2 * k + 1, azimuth=300.0, altitude=35.0, z_factor=1.5)
        assert list(one) == [nm] and bits(one[nm]) == first[nm], nm
    assert dp._tile.device_bytes() == held


@pytest.mark.parametrize('kind', ['specks', 'terraced'])
def test_both_kernels_give_the_same_bits_at_k_1(kind, monkeypatch):
    for shape in BIG + ((3, 3), (5, 7)):
        z = _field(shape, kind, 1)
        monkeypatch.delenv('PYDEM_TA_GENERIC', raising=False)
        dp, march = _device(z, 1)
        march = {nm: bits(v) for nm, v in march.items()}
        n_march = dp.terrain_attributes_stats['n_defined']
        monkeypatch.setenv('PYDEM_TA_GENERIC', '1')
        dp, window = _device(z, 1)
        assert {nm: bits(v) for nm, v in window.items()} == march, shape
        assert dp.terrain_attributes_stats['n_defined'] == n_march
        ref, count = _twin(shape, kind, 1)
        _hold(window, dp.terrain_attributes_stats, ref, count, "general path at k=1 %r" % (shape,))


def test_same_bytes_in_a_child_under_poison():
    want = {}
    for k in HALF_WIDTHS:
        _, out = _device(_field(BIG[1], 'specks', k), k)
        want[k] = sorted((nm, bits(v)) for nm, v in out.items())
    body = "\n".join(["import test_gpu_terrain as G",
                      "from pydem_amd import _ffi",
                      "for k in G.HALF_WIDTHS:",
                      "    _, out = G._device(G._field(G.BIG[1], 'specks', k), k)",
                      "    print('BITS', k, sorted((nm, bits(v)) for nm, v in out.items()))",
                      "assert _ffi.poison_stats()[0] > 0",
                      "print('CHILD-OK')"])
    r = K.run_child(body, env={'PYDEM_MEM_POISON': '0xA5'}, timeout=300)
    for k in HALF_WIDTHS:
        assert "BITS %d %r" % (k, want[k]) in r.stdout, k


def test_the_call_leaves_the_tile_alone():
    import warnings
    z = _field(BIG[0], 'fractal', 1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = _dp(z)
        plain.calc_slopes_directions()
        plain.calc_uca()
        before = K._snapshot(plain)
        for k in HALF_WIDTHS:
            plain.calc_terrain_attributes(('gradient', 'mean', 'hillshade'), 2 * k + 1)
        K._same_snapshot(before, K._snapshot(plain))
        # on the elevation alone, before the slopes exist; what follows is what it would have been
        early = _dp(z)
        out = early.calc_terrain_attributes(window=5)
        assert early._on_device == {'elev'} and not early._has('mag')
        assert_same_bits(out['gradient'], _twin(BIG[0], 'fractal', 2)[0]['gradient'], 'before the slopes')
        early.calc_slopes_directions()
        early.calc_uca()
    for nm in ('mag', 'direction', 'uca'):
        assert_same_bits(getattr(early, nm), getattr(plain, nm), nm)


def test_conditioned_elevation_is_the_one_that_counts():
    from pydem_amd import terrain as T
    z = np.array(_field((64, 64), 'fractal', 1))
    z[30:34, 30:34] -= 50.0                                         # a pit the fill raises
    dp = _dp(z)
    dp.calc_fill_depressions()
    filled = np.array(dp.elev)
    assert not np.array_equal(filled, z)
    out = dp.calc_terrain_attributes(('dzdx', 'mean'), 5)
    ref, count = T.terrain_attributes_ref(filled, dp.dX2, dp.dY2, 5, ('dzdx', 'mean'))
    for nm in ref:
        assert_same_bits(out[nm], ref[nm], nm)
    assert dp.terrain_attributes_stats['n_defined'] == count


def test_argument_errors_allocate_and_launch_nothing():
    import ctypes as C
    from pydem_amd import _ffi
    n, m = 12, 10
    t = _ffi.Tile(n, m)
    plane = np.full((n, m), 123.0)
    light = np.array([0.0, 0.0, 1.0])
    nine = len(_ffi.Tile.TERRAIN_ATTRS)

    def call(k=1, outs=(2,), lv=light, zf=1.0):
        arr = (C.c_void_p * nine)(*[plane.ctypes.data if a in (outs or ()) else None for a in range(nine)])
        ms, cnt = C.c_double(-1.0), C.c_int64(-1)
        rc = t.lib.pydem_terrain_attributes(t._h, k, _ffi._ptr(lv), zf, arr if outs is not None else None, C.byref(ms), C.byref(cnt))
        return rc, ms.value, cnt.value

    held = t.device_bytes()
    assert call()[0] == -3                                          # no spacing, no elevation
    t.set_spacing(np.ones(n - 1), np.ones(n - 1), np.ones(n), np.ones(n))
    assert call()[0] == -3                                          # no elevation
    t.upload(_ffi.ELEV, np.arange(n * m, dtype=np.float64).reshape(n, m))
    held = t.device_bytes()
    for kw in (dict(k=0), dict(k=8), dict(k=-1), dict(outs=()), dict(outs=None), dict(outs=(8,), lv=None), dict(zf=0.0), dict(zf=-2.0),
               dict(zf=float('nan')), dict(zf=float('inf'))):
        assert call(**kw) == (-2, -1.0, -1), kw
        assert 'pydem_terrain_attributes' in t.lib.pydem_hip_last_error().decode()
    assert t.device_bytes() == held and (plane == 123.0).all()
    rc, ms, cnt = call(k=1, outs=(0, 8))                            # one array for two planes: the last download stays
    assert rc == 0 and ms >= 0 and cnt == (n - 2) * (m - 2)
    assert t.device_bytes() == held + 8192 + 2 * 8 * n * m
    assert call(k=7, outs=(2,), lv=None)[0] == 0                    # no hillshade asked: no light needed; the tile is under 15 x 15
    assert np.isnan(plane).all() and t.device_bytes() == held + 8192 + 2 * 8 * n * m
    t.close()


def test_a_tile_under_three_rows_is_all_nan():
    dp = _dp(np.ones((2, 9)))
    out = dp.calc_terrain_attributes(('gradient', 'aspect'), 3)
    assert all(v.shape == (2, 9) and np.isnan(v).all() for v in out.values())
    assert dp.terrain_attributes_stats == dict(ms=0.0, n_defined=0, window=3) and dp._tile is None
