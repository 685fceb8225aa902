"""GPU tier: pydem_fill_depressions (csrc/fill_depressions.hip) against the host priority flood (pydem_amd/conditioning.py:
fill_depressions, itself held bit for bit against a Jacobi iteration by tests/test_fill_depressions_ref.py): elevation and depth
with tobytes(), counts and maxima exactly; the schedules; the pass limit; the pipeline the stage exists for; dtypes; hygiene."""
import warnings

import numpy as np
import pytest

import fill_fields as F

pytestmark = pytest.mark.gpu

_REF = {}


def ref(name, z, eps, outlets=None):
    """(W, depth, eps used) of the host flood, computed once per case"""
    key = (name, eps, outlets is not None)
    if key not in _REF:
        from pydem_amd import conditioning
        _REF[key] = conditioning.fill_depressions(z, eps, outlets)
    return _REF[key]


def device_fill(z, eps, outlets=None, **kw):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, **kw)
    W, depth = dp.calc_fill_depressions(eps, outlets, return_depth=True)
    return dp, W, depth, dp.fill_depressions_stats


def check(name, z, eps, outlets=None):
    rW, rdepth, reps = ref(name, z, eps, outlets)
    dp, W, depth, st = device_fill(z, eps, outlets)
    assert st['epsilon'] == reps
    assert W.dtype == np.float64 and W.tobytes() == rW.tobytes()
    assert depth.tobytes() == rdepth.tobytes()
    with np.errstate(invalid='ignore'):
        up = rdepth > 0
    assert st['n_raised'] == int(up.sum())
    assert st['max_depth'] == (float(rdepth[up].max()) if up.any() else 0.0)
    if min(z.shape) >= 3:
        assert st['passes'] >= 1 and st['ms'] > 0
    return dp, st


# 1. fractal tiles
@pytest.mark.parametrize('shape', [(300, 260), (96, 80)])
@pytest.mark.parametrize('eps', [0.0, None])
@pytest.mark.parametrize('nan_rect', [False, True])
def test_fractal_tiles(shape, eps, nan_rect):
    z = F.fractal(shape[0], shape[1], nan_rect)
    _, st = check('fractal%r%r' % (shape, nan_rect), z, eps)
    if shape == (96, 80):
        assert st['n_raised'] >= 500          # the input has not silently become trivial
    if eps is None:
        assert st['epsilon'] == 2.0 ** -22
    assert st['passes'] >= 2 and st['ms'] > 0


# 2. shapes
@pytest.mark.parametrize('name', sorted(F.designed()))
@pytest.mark.parametrize('eps', [0.0, None])
def test_designed_fields(name, eps):
    z = F.designed()[name]()
    _, st = check(name, z, eps)
    if name == 'serpentine':
        assert st['passes'] >= 3              # (one or two passes: the multi-pass path was not reached)
    if name.startswith('corner_spill') and eps == 0.0:
        assert st['n_raised'] == 144 and st['max_depth'] == 20.0


@pytest.mark.parametrize('shape', [(33, 65), (64, 64), (3, 3), (1, 7), (65, 33), (32, 97)])
@pytest.mark.parametrize('eps', [0.0, None])
def test_block_shapes(shape, eps):
    from pydem_amd import synth
    z = synth.fractal(shape[0], shape[1], seed=11, top_shift=4, n_octaves=4)
    if min(shape) >= 3:
        z[1:-1, 1:-1] -= 300.0                # everything inside the border ring is one depression with relief
    _, st = check('shape%r' % (shape,), z, eps)
    if shape == (1, 7):
        assert st['passes'] == 0              # the host path


# 3. schedule independence
@pytest.mark.parametrize('name', ['fractal96', 'serpentine'])
@pytest.mark.parametrize('eps', [0.0, None])
def test_one_step_visits_give_the_same_bytes(monkeypatch, name, eps):
    z = F.fractal(96, 80) if name == 'fractal96' else F.serpentine()
    _, W0, d0, st0 = device_fill(z, eps)
    monkeypatch.setenv('PYDEM_FILL_LOCAL', '0')
    _, W1, d1, st1 = device_fill(z, eps)
    assert W1.tobytes() == W0.tobytes() and d1.tobytes() == d0.tobytes()
    assert (st1['n_raised'], st1['max_depth']) == (st0['n_raised'], st0['max_depth'])
    assert st1['passes'] > st0['passes']      # it really was another schedule
    monkeypatch.setenv('PYDEM_FILL_LOCAL', '1')
    monkeypatch.setenv('PYDEM_FILL_CHECK_EVERY', '1')
    _, W2, _, st2 = device_fill(z, eps)
    assert W2.tobytes() == W0.tobytes() and st2['passes'] == st0['passes']


# 4. pass limit
def test_pass_limit_is_an_error_and_leaves_the_surface(monkeypatch):
    from pydem_amd import DEMProcessor, _ffi
    z = F.serpentine()
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0)
    dp._ensure_tile()
    dp._push('elev')
    monkeypatch.setenv('PYDEM_FILL_MAX_PASSES', '2')
    with pytest.raises(_ffi.HipError, match='error -5'):
        dp._tile.fill_depressions(0.0)
    assert dp._tile.download(_ffi.ELEV).tobytes() == z.tobytes()
    with pytest.raises(_ffi.HipError, match='error -5'):
        dp.calc_fill_depressions(None)
    assert dp._tile.download(_ffi.ELEV).tobytes() == z.tobytes()
    monkeypatch.delenv('PYDEM_FILL_MAX_PASSES')
    W = dp.calc_fill_depressions(0.0)
    assert W.tobytes() == ref('serpentine', z, 0.0)[0].tobytes()


def test_bad_arguments_are_minus_two_and_leave_the_surface():
    from pydem_amd import _ffi
    z = F.bowl()
    t = _ffi.Tile(*z.shape)
    t.upload(_ffi.ELEV, z)
    for eps in (float('nan'), float('inf'), 2.0 ** -45):
        with pytest.raises(_ffi.HipError, match='error -2'):
            t.fill_depressions(eps)
    assert t.download(_ffi.ELEV).tobytes() == z.tobytes()
    bad = z.copy()
    bad[50, 50] = -np.inf
    t.upload(_ffi.ELEV, bad)
    with pytest.raises(_ffi.HipError, match='error -2'):
        t.fill_depressions(0.0)
    assert t.download(_ffi.ELEV).tobytes() == bad.tobytes()
    t.upload(_ffi.ELEV, z)
    depth, eps, n_raised, max_depth, passes, ms = t.fill_depressions(-3.0, None, True)       # < 0 at the C-ABI: automatic
    assert eps == 2.0 ** -22 and depth.tobytes() == ref('bowl', z, None)[1].tobytes()


# 5. the pipeline: the point of the feature
def _ring(shape):
    ring = np.zeros(shape, bool)
    ring[0, :] = ring[-1, :] = True
    ring[:, 0] = ring[:, -1] = True
    return ring


def test_pipeline_drains_the_bowl():
    from pydem_amd import DEMProcessor
    z = F.bowl()
    ring = _ring(z.shape)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, drain_pits_max_dist=4)
        dp.calc_uca()
        assert dp.timings['n_pits_undrained'] > 0
        d = dp.calc_dist_down(target=ring, kind='h', stat='min')
        assert np.isnan(d[F.BOWL_BOTTOM])

        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, drain_pits_max_dist=4, fill_depressions=True)
        dp.calc_uca()
        assert dp.timings['n_pits_undrained'] == 0 and dp.timings['n_flats'] == 0
        assert dp.fill_depressions_stats['epsilon'] == 2.0 ** -22 and dp.fill_depressions_stats['n_raised'] > 0
        d = dp.calc_dist_down(target=ring, kind='h', stat='min')
        assert np.isfinite(d).all()

        # the classic fill: the lake is a flat, and flats do not drain
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, drain_pits_max_dist=4, fill_depressions=True, fill_depressions_epsilon=0.0)
        dp.calc_uca()
        assert dp.timings['n_flats'] > 0


# 6. dtypes
def test_int16_terraces_keep_their_dtype_with_the_classic_fill():
    t = F.terraces()
    assert t.dtype == np.int16
    rW, _, _ = ref('terraces', t.astype(np.float64), 0.0)
    dp, W, depth, st = device_fill(t, 0.0)
    assert W.dtype == np.int16 and np.array_equal(W, rW) and st['n_raised'] > 0
    rW, rdepth, _ = ref('terraces', t.astype(np.float64), None)
    dp, W, depth, st = device_fill(t, None)
    assert W.dtype == np.float64 and W.tobytes() == rW.tobytes() and depth.tobytes() == rdepth.tobytes()


def test_float32_upload_keeps_float32_with_the_classic_fill():
    z32 = F.fractal(96, 80).astype(np.float32)
    rW, rdepth, _ = ref('fractal96_f32', z32.astype(np.float64), 0.0)
    dp, W, depth, st = device_fill(z32, 0.0)
    assert W.dtype == np.float32 and W.astype(np.float64).tobytes() == rW.tobytes()
    assert depth.tobytes() == rdepth.tobytes() and st['n_raised'] >= 500
    dp, W, depth, st = device_fill(z32, None)
    assert W.dtype == np.float64 and W.tobytes() == ref('fractal96_f32', z32.astype(np.float64), None)[0].tobytes()


# 7. hygiene
def test_idempotent_and_deterministic_on_the_device():
    z = F.fractal(300, 260, True)
    for eps in (0.0, None):
        dp, W, depth, st = device_fill(z, eps)
        W2, depth2 = dp.calc_fill_depressions(eps, return_depth=True)
        assert dp.fill_depressions_stats['n_raised'] == 0 and dp.fill_depressions_stats['max_depth'] == 0.0
        assert W2.tobytes() == W.tobytes() and not (depth2 > 0).any()
        _, W3, depth3, st3 = device_fill(z, eps)
        assert W3.tobytes() == W.tobytes() and depth3.tobytes() == depth.tobytes() and st3['passes'] == st['passes']


def test_no_device_memory_is_kept():
    from pydem_amd import _ffi
    z = F.fractal(300, 260)
    t = _ffi.Tile(*z.shape)
    t.upload(_ffi.ELEV, z)
    b0 = t.device_bytes()
    first = t.fill_depressions(None, None, True)
    assert t.device_bytes() == b0
    _ffi.release_scratch()
    out = np.zeros(z.shape, bool)
    out[100, 100] = True
    t.upload(_ffi.ELEV, z)
    t.fill_depressions(None, out, True)         # the arena grows to what the call needs, once
    b1 = t.device_bytes()
    free1 = _ffi.device_memory(0)[0]
    for k in range(20):
        t.upload(_ffi.ELEV, z)
        got = t.fill_depressions(None, out if k % 2 else None, True)
        if k % 2 == 0:
            assert got[0].tobytes() == first[0].tobytes() and got[1:5] == first[1:5]
    assert t.device_bytes() == b1 and _ffi.device_memory(0)[0] >= free1


def test_the_fill_invalidates_the_flow_graph():
    from pydem_amd import DEMProcessor, _ffi
    z = F.bowl()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)
        dp.calc_uca()
        ring = _ring(z.shape)
        dp._tile.dist_down('h', 'min', ring)
        dp.run_fill_depressions()
        with pytest.raises(_ffi.HipError, match='error -3'):
            dp._tile.dist_down('h', 'min', ring)
        assert 'uca' not in dp._on_device and not dp._has('direction')
        with pytest.raises(_ffi.HipError, match='error -3'):
            dp._tile.download(_ffi.MAG)
        d = dp.calc_dist_down(target=ring, kind='h', stat='min')          # runs the stencil and calc_uca again
        assert np.isfinite(d).all()


def test_outlets_as_mask_and_as_pairs_agree():
    z = F.bowl()
    mask = np.zeros(z.shape, bool)
    mask[F.BOWL_BOTTOM] = True
    for eps in (0.0, None):
        rW, rdepth, _ = ref('bowl_outlet', z, eps, mask)
        _, Wm, dm, stm = device_fill(z, eps, mask)
        _, Wp, dpth, stp = device_fill(z, eps, [F.BOWL_BOTTOM])
        assert Wm.tobytes() == Wp.tobytes() == rW.tobytes() and dm.tobytes() == dpth.tobytes() == rdepth.tobytes()
        assert stm['n_raised'] == stp['n_raised'] == int((rdepth > 0).sum())
        assert Wm[F.BOWL_BOTTOM] == z[F.BOWL_BOTTOM]
    r, c = np.mgrid[0:z.shape[0], 0:z.shape[1]]
    inside = (r - F.BOWL_BOTTOM[0]) ** 2 + (c - F.BOWL_BOTTOM[1]) ** 2 <= F.BOWL_RADIUS ** 2
    assert ref('bowl_outlet', z, 0.0, mask)[0][inside].tobytes() == z[inside].tobytes()     # the bowl stays
