"""GPU tier: pydem_horizon (csrc/horizon.hip) through DEMProcessor.calc_horizon against its numpy twin (pydem_amd/horizon.py:
horizon_ref).  A horizon tangent is a maximum over a fixed set of products and the sky-view factor a fixed sequence of * + /, so
everything is compared exactly: the NaN patterns first, then the bytes of the other cells, and n_defined.

The shapes are the smallest at which a kernel of 32 x 64 blocks that walks a ray in segments of 32 steps can go wrong: the smallest
tile the library holds; tiles thinner than a block and longer than a wavefront; one cell past a block and a wavefront; rays of 40
cells (two segments, several blocks in both directions) and of 60 (more steps than one launch takes); and rays of 200 cells on a tile of 64,
where every ray leaves the tile.  Each with edge_nan on and off, with 'horizon' and 'svf' together and each alone.

Then: the same bytes before and after other analyses have used the tile's memory, and theirs untouched; the same bytes in a child
under PYDEM_MEM_POISON; the cast shadow of a tower; the argument errors, which allocate, launch and write nothing."""
import functools

import numpy as np
import pytest

import flowgraph_kit as K
from flowgraph_kit import assert_same_bits, bits

pytestmark = pytest.mark.gpu

SEED = 11
# shape, n_dir, azimuth0, max_dist in cells of the smaller size, gx, gy, z_factor
CASES = {
    'smallest': ((3, 3), 8, 0.0, 1.5, 30.0, 30.0, 1.0),
    'flat_wide': ((5, 70), 16, 0.0, 2.0, 30.0, 30.0, 1.0),
    'thin_tall': ((70, 5), 5, 11.25, 2.0, 30.0, 30.0, 1.0),
    'past_a_block': ((33, 65), 16, 0.0, 10.0, 30.0, 20.0, 1.0),
    'one_direction': ((33, 65), 1, 200.0, 12.0, 30.0, 30.0, 1.0),
    'two_segments': ((97, 130), 8, 0.0, 40.0, 30.0, 30.0, 0.5),
    'several_launches': ((97, 130), 16, 11.25, 60.0, 20.0, 30.0, 1.0),
    'every_ray_leaves': ((64, 64), 5, 0.0, 200.0, 30.0, 30.0, 1.0),
}


@functools.lru_cache(maxsize=None)
def _field(shape):
    """a fractal with a few no-data cells -- the corners of the tile and of a kernel block among them -- and one blob"""
    from pydem_amd import synth
    n, m = shape
    z = synth.fractal(n, m, seed=SEED, top_shift=7, n_octaves=7)
    rng = np.random.default_rng(3)
    if n * m > 9:
        z[rng.integers(0, n, 5), rng.integers(0, m, 5)] = np.nan
        for cell in ((0, 0), (n - 1, m - 1), (32, 64), (31, 63)):
            if cell[0] < n and cell[1] < m:
                z[cell] = np.nan
        if n > 20 and m > 20:
            z[n // 2 - 3:n // 2 + 2, m // 3:m // 3 + 6] = np.nan
    else:
        z[0, 2] = np.nan
    z.setflags(write=False)
    return z


def _table(name):
    from pydem_amd import horizon as H
    shape, n_dir, az0, cells, gx, gy, zf = CASES[name]
    return H.ray_table(n_dir, az0, cells * min(gx, gy), gx, gy, zf)


@functools.lru_cache(maxsize=None)
def _twin(name, edge_nan):
    """the twin's planes and counts of a case, computed once"""
    from pydem_amd import horizon as H
    out, count = H.horizon_ref(_field(CASES[name][0]), _table(name), edge_nan)
    _, count_hor = H.horizon_ref(_field(CASES[name][0]), _table(name), edge_nan, True, False)
    for v in out.values():
        v.setflags(write=False)
    return out, count, count_hor


def _dp(z, gx=30.0, gy=30.0):
    from pydem_amd import DEMProcessor
    return DEMProcessor(elev=z, dX=gx, dY=gy, fill_flats=False, drain_pits_path=False)


def _device(name, edge_nan, which=('horizon', 'svf'), dp=None):
    shape, n_dir, az0, cells, gx, gy, zf = CASES[name]
    dp = dp or _dp(_field(shape), gx, gy)
    out = dp.calc_horizon(n_dir, cells * min(gx, gy), az0, zf, edge_nan, which)
    return dp, out


def _hold(out, stats, name, edge_nan):
    ref, count, count_hor = _twin(name, edge_nan)
    what = "%s edge_nan=%r" % (name, edge_nan)
    for nm in ('horizon', 'svf'):
        if nm in out:
            assert out[nm].dtype == np.float64 and out[nm].shape == ref[nm].shape
            assert_same_bits(out[nm], ref[nm], "%s %s" % (what, nm))
    assert stats['n_defined'] == (count if 'svf' in out else count_hor), (what, stats['n_defined'], count, count_hor)
    assert stats['steps'] == int(_table(name).start[-1]) and stats['n_dir'] == CASES[name][1]


@pytest.mark.parametrize('edge_nan', [True, False])
@pytest.mark.parametrize('name', list(CASES))
def test_the_device_gives_the_twins_bytes(name, edge_nan):
    ref, count, _ = _twin(name, edge_nan)
    dp, both = _device(name, edge_nan)
    _hold(both, dp.horizon_stats, name, edge_nan)
    held = dp._tile.device_bytes()
    # each plane alone: the same bytes, from the block the call before left behind
    _, hor = _device(name, edge_nan, ('horizon',), dp)
    assert list(hor) == ['horizon', 'azimuths'] and bits(hor['horizon']) == bits(both['horizon'])
    _hold(hor, dp.horizon_stats, name, edge_nan)
    _, svf = _device(name, edge_nan, ('svf',), dp)
    assert list(svf) == ['svf', 'azimuths'] and bits(svf['svf']) == bits(both['svf'])
    _hold(svf, dp.horizon_stats, name, edge_nan)
    assert dp._tile.device_bytes() == held
    # and alone on a fresh tile, whose block is smaller
    fresh, svf = _device(name, edge_nan, ('svf',))
    assert bits(svf['svf']) == bits(both['svf']) and fresh._tile.device_bytes() < held
    if name == 'every_ray_leaves':
        assert np.isnan(both['svf']).all() == edge_nan and (count == 0) == edge_nan
        assert edge_nan or count == (~np.isnan(_field(CASES[name][0]))).sum()
    if name == 'smallest' and edge_nan:
        assert count == 1 and not np.isnan(both['svf'][1, 1])


def test_the_cases_cover_what_they_are_named_for():
    tables = {name: _table(name) for name in CASES}
    per_dir = {name: np.diff(t.start) for name, t in tables.items()}
    assert per_dir['two_segments'].max() == 40 and per_dir['two_segments'].min() > 20
    assert int(tables['several_launches'].start[-1]) > 512          # more steps than one launch takes
    assert per_dir['every_ray_leaves'].min() > 64 * 1.5 and per_dir['every_ray_leaves'].max() == 200
    assert {CASES[name][1] for name in CASES} >= {1, 5, 8, 16}
    assert any(c[2] == 11.25 for c in CASES.values()) and any(c[4] != c[5] for c in CASES.values()) and any(c[6] == 0.5 for c in CASES.values())
    for name in ('two_segments', 'several_launches', 'past_a_block'):
        ref, count, _ = _twin(name, True)
        assert 0 < count < np.prod(CASES[name][0]) and (ref['horizon'][~np.isnan(ref['horizon'])] > 0).any()
        assert (ref['svf'][~np.isnan(ref['svf'])] < 1).any()


def test_the_tiles_memory_disturbs_nothing_and_nothing_disturbs_it():
    import warnings
    name = 'several_launches'
    shape, n_dir, az0, cells, gx, gy, zf = CASES[name]
    z = _field(shape)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fresh = _dp(z, gx, gy)
        want_ta = fresh.calc_terrain_attributes(('gradient', 'mean', 'hillshade'), 5)
        fresh.calc_slopes_directions()
        fresh.calc_uca()
        want_uca = np.array(fresh.uca)
        dp, first = _device(name, True)
        first = {nm: bits(first[nm]) for nm in ('horizon', 'svf')}
        ta = dp.calc_terrain_attributes(('gradient', 'mean', 'hillshade'), 5)
        dp.calc_slopes_directions()
        dp.calc_uca()
        uca = np.array(dp.uca)
        before = K._snapshot(dp)
        _, again = _device(name, True, dp=dp)
        K._same_snapshot(before, K._snapshot(dp))
    assert {nm: bits(again[nm]) for nm in ('horizon', 'svf')} == first
    _hold(again, dp.horizon_stats, name, True)
    for nm in want_ta:
        assert_same_bits(ta[nm], want_ta[nm], nm)
    assert_same_bits(uca, want_uca, 'uca')
    for nm in ('mag', 'direction'):
        assert_same_bits(getattr(dp, nm), getattr(fresh, nm), nm)


def test_same_bytes_in_a_child_under_poison():
    names = ('thin_tall', 'several_launches')
    want = {}
    for name in names:
        _, out = _device(name, False)
        want[name] = sorted((nm, bits(out[nm])) for nm in ('horizon', 'svf'))
    body = "\n".join(["import test_gpu_horizon as G",
                      "from pydem_amd import _ffi",
                      "for name in %r:" % (names,),
                      "    _, out = G._device(name, False)",
                      "    print('BITS', name, sorted((nm, bits(out[nm])) for nm in ('horizon', 'svf')))",
                      "assert _ffi.poison_stats()[0] > 0",
                      "print('CHILD-OK')"])
    r = K.run_child(body, env={'PYDEM_MEM_POISON': '0xA5'}, timeout=300)
    for name in names:
        assert "BITS %s %r" % (name, want[name]) in r.stdout, name


def test_the_cast_shadow_of_a_tower():
    from pydem_amd import horizon as H
    z = np.zeros((40, 90))
    z[20, 10] = 300.0
    z[7, 33] = np.nan
    dp = _dp(z)
    for az, alt, edge_nan in ((270.0, 30.0, False), (270.0, 30.0, True), (247.5, 20.0, False), (300.0, 55.0, False)):
        shadow = dp.calc_cast_shadow(az, alt, 1500.0, edge_nan=edge_nan)
        want = H.cast_shadow_ref(z, az, alt, 1500.0, 30.0, 30.0, edge_nan=edge_nan)
        assert shadow.dtype == np.float64 and np.array_equal(shadow, want, equal_nan=True), (az, alt, edge_nan)
        assert dp.horizon_stats['n_dir'] == 1
    east = dp.calc_cast_shadow(270.0, 30.0, 1500.0, edge_nan=False)
    # 300 / tan(30 degrees) = 519.6 ground units = 17.3 cells of 30: the seventeen cells east of the tower, and nothing else
    assert np.argwhere(east == 0).tolist() == [[20, c] for c in range(11, 28)]
    assert np.isnan(east).sum() == 1 and np.isnan(east[7, 33])
    half = dp.calc_cast_shadow(270.0, 30.0, 1500.0, z_factor=0.5, edge_nan=False)
    assert np.argwhere(half == 0).tolist() == [[20, c] for c in range(11, 19)]


def test_a_maximum_among_zeros_is_plus_zero():
    """(-0.0) - (+0.0) is -0.0 and so is its product with a weight: not greater than the 0.0 a tangent starts from"""
    from pydem_amd import horizon as H
    rng = np.random.default_rng(8)
    z = np.where(rng.random((40, 70)) < 0.5, -0.0, 0.0)
    z[5, 5] = 2.0
    z[30, 60] = -3.0
    assert np.signbit(z).sum() > 1000
    for edge_nan in (False, True):
        out = _dp(z).calc_horizon(8, 6 * 30.0, 0.0, 1.0, edge_nan, ('horizon', 'svf'))
        ref, _ = H.horizon_ref(z, H.ray_table(8, 0.0, 6 * 30.0, 30.0, 30.0), edge_nan)
        assert not np.signbit(ref['horizon'][~np.isnan(ref['horizon'])]).any() and (ref['horizon'] == 0).sum() > 8 * 1000
        assert_same_bits(out['horizon'], ref['horizon'], 'zeros: horizon')
        assert_same_bits(out['svf'], ref['svf'], 'zeros: svf')


def test_argument_errors_allocate_launch_and_write_nothing():
    import ctypes as C
    from pydem_amd import _ffi, horizon as H
    n, m = 12, 10
    t = _ffi.Tile(n, m)
    plane = np.full((n, m), 123.0)
    good = H.ray_table(4, 0.0, 3.0)

    def call(n_dir=4, start=good.start, dr=good.dr, dc=good.dc, w=good.w, hor=False, svf=True, holes=()):
        start, dr, dc, w = (None if a is None else np.ascontiguousarray(a, tp)
                            for a, tp in ((start, np.int32), (dr, np.int16), (dc, np.int16), (w, np.float64)))
        planes = (C.c_void_p * max(n_dir, 1))(*[None if d in holes else plane.ctypes.data for d in range(max(n_dir, 1))]) if hor else None
        ms, cnt = C.c_double(-1.0), C.c_int64(-1)
        rc = t.lib.pydem_horizon(t._h, n_dir, _ffi._ptr(start), _ffi._ptr(dr), _ffi._ptr(dc), _ffi._ptr(w), 1, planes,
                                 _ffi._ptr(plane if svf else None), C.byref(ms), C.byref(cnt))
        return rc, ms.value, cnt.value

    assert call()[0] == -3                                          # no spacing, no elevation
    t.set_spacing(np.ones(n - 1), np.ones(n - 1), np.ones(n), np.ones(n))
    assert call()[0] == -3                                          # no elevation
    t.upload(_ffi.ELEV, np.arange(n * m, dtype=np.float64).reshape(n, m))
    held = t.device_bytes()
    long_ = H.ray_table(1, 0.0, 1024.0)
    too_long = np.arange(1, 1026)
    w_bad = [good.w.copy() for _ in range(4)]
    w_bad[0][1] = np.nan; w_bad[1][0] = 0.0; w_bad[2][2] = np.inf; w_bad[3][1] = w_bad[3][0] * 2
    jump = good.dr.copy()
    jump[2] = 40                                                    # 32 steps may not span more than 32 cells
    for kw in [dict(n_dir=0), dict(n_dir=65), dict(n_dir=-1), dict(start=None), dict(dr=None), dict(dc=None), dict(w=None),
               dict(svf=False), dict(hor=True, holes=(2,)), dict(start=good.start + 1), dict(start=good.start[::-1]),
               dict(n_dir=1, start=[0, 1025], dr=-too_long, dc=0 * too_long, w=1.0 / too_long), dict(dr=jump), dict(dc=jump)] + \
              [dict(w=w) for w in w_bad]:
        assert call(**kw) == (-2, -1.0, -1), kw
        assert 'pydem_horizon' in t.lib.pydem_hip_last_error().decode()
    assert t.device_bytes() == held and (plane == 123.0).all()
    rc, ms, cnt = call(n_dir=1, start=long_.start, dr=long_.dr, dc=long_.dc, w=long_.w)     # 1024 steps are allowed
    assert rc == 0 and ms >= 0 and cnt == 0 and np.isnan(plane).all()
    assert t.device_bytes() == held + 8192 + 1024 * 16 + 32 * 32 + 256 + 8 * n * m
    rc, ms, cnt = call(hor=True, svf=False)                         # one array for the four planes: the last download stays
    assert rc == 0 and cnt == (n - 6) * (m - 6)
    assert t.device_bytes() == held + 8192 + 1024 * 16 + 32 * 32 + 256 + 8 * n * m        # a smaller request: the block stays
    t.close()
