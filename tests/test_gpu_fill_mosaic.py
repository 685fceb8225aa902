"""GPU tier: the seam session of csrc/fill_depressions.hip (pydem_fill_seam_begin / _relax / _get_lines / _end) against its host
twin (pydem_amd/conditioning.py: SeamFill), W compared with tobytes() after every relax; warm restarts; the session's memory; and
ProcessManager.process_fill_depressions on one GPU against conditioning.fill_depressions of the stitched raster, tile by tile.
Shapes sit around the 32-cell block: one block, several, partial ones, a three-row tile."""
import threading

import numpy as np
import pytest

import seam_fill_kit as K

pytestmark = pytest.mark.gpu

SIDES = ('top', 'bottom', 'left', 'right')
SHAPES = [(33, 65), (70, 45), (3, 40), (64, 64)]
RASTER = (203, 261)                                 # tile edges of every cut below are no multiple of 32


def surface(shape, nan=False):
    from pydem_amd import synth
    z = synth.fractal(shape[0], shape[1], seed=11, top_shift=4, n_octaves=4)
    z[1:-1, 1:-1] -= 300.0                          # everything inside the border ring is one depression with relief
    if nan:
        z[0, 5] = z[1, 9] = z[shape[0] // 2, 0] = z[shape[0] - 1, shape[1] - 2] = np.nan        # on and beside the seam lines
    return z


def auto_eps(z):
    from pydem_amd import conditioning
    return conditioning.fill_depressions_epsilon(z, None)


def side_len(shape, side):
    return shape[1] if side in ('top', 'bottom') else shape[0]


def side_of(a, side):
    return {'top': a[0, :], 'bottom': a[-1, :], 'left': a[:, 0], 'right': a[:, -1]}[side]


def make_caps(z, sides, kind, seed=0):
    rng = np.random.RandomState(seed)
    caps = {}
    for k, s in enumerate(sides):
        L = side_len(z.shape, s)
        if kind == 'inf':
            caps[s] = np.full(L, np.inf)
        elif kind == 'z':
            caps[s] = np.nan_to_num(np.array(side_of(z, s)), nan=np.inf)
        else:
            caps[s] = np.nan_to_num(np.array(side_of(z, s)), nan=0.0) + rng.uniform(0.0, 60.0, L) + 7.0 * k     # (the two lines of a corner differ)
    return caps


def device(z):
    from pydem_amd import DEMProcessor
    return DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)


def device_W(dp):
    return np.array(dp.fill_seam_lines([(0, r) for r in range(dp.shape[0])]))


def check_lines(dp, W):
    n, m = W.shape
    got = dp.fill_seam_lines([(0, 0), (1, 0), (0, -1), (1, -1), (1, m // 2), (0, n // 2), (1, 1)])
    want = [W[0], W[:, 0], W[-1], W[:, -1], W[:, m // 2], W[n // 2], W[:, 1]]
    for g, w in zip(got, want):
        assert g.tobytes() == np.ascontiguousarray(w).tobytes()


def session(z, sides, caps_seq, eps, outlets=None):
    """the same session on the device and on the host twin, W and n_lowered compared after every relax; returns (dp, twin)"""
    from pydem_amd import conditioning
    seam = {s: np.ones(side_len(z.shape, s), bool) for s in sides}
    twin = conditioning.SeamFill(z, outlets, seam)
    dp = device(z)
    assert dp.fill_seam_begin(seam, outlets) == twin.amax
    for caps in caps_seq:
        out = dp.fill_seam_relax(eps, caps)
        low = twin.relax(eps, caps)
        assert device_W(dp).tobytes() == twin.W.tobytes()
        assert out['n_lowered'] == low and out['passes'] >= 1 and out['ms'] > 0
    check_lines(dp, twin.W)
    return dp, twin


def finish(dp, twin):
    """commit where W is finite (the elevation is the twin's W), the -5 refusal and an abort where it is not"""
    from pydem_amd import _ffi
    z0 = twin.z
    if np.isinf(twin.W).any():
        with pytest.raises(_ffi.HipError, match='error -5'):
            dp.fill_seam_end(True)
        dp.fill_seam_end(False)
        assert np.asarray(dp.elev).tobytes() == z0.tobytes()
    else:
        st = dp.fill_seam_end(True, return_depth=True)
        W, depth = twin.end(True)
        assert np.asarray(dp.elev).tobytes() == W.tobytes() and dp.fill_depth.tobytes() == depth.tobytes()
        with np.errstate(invalid='ignore'):
            up = depth > 0
        assert st['n_raised'] == int(up.sum()) and st['max_depth'] == (float(depth[up].max()) if up.any() else 0.0)


CONFIGS = {'four_sides': SIDES, 'one_side': ('right',), 'corner': ('top', 'left')}


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('config', sorted(CONFIGS))
@pytest.mark.parametrize('kind', ['inf', 'z', 'random'])
@pytest.mark.parametrize('auto', [False, True])
def test_one_tile_session_against_the_host_twin(shape, config, kind, auto):
    z = surface(shape)
    eps = auto_eps(z) if auto else 0.0
    sides = CONFIGS[config]
    dp, twin = session(z, sides, [make_caps(z, sides, kind)], eps)
    if config == 'corner' and kind == 'random':
        c = twin.cap[0, 0]
        assert c == min(make_caps(z, sides, kind)['top'][0], make_caps(z, sides, kind)['left'][0])      # the smaller line counts
    finish(dp, twin)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('auto', [False, True])
def test_no_data_on_and_beside_the_seam_lines(shape, auto):
    z = surface(shape, nan=True)
    eps = auto_eps(z) if auto else 0.0
    caps = make_caps(z, SIDES, 'random')
    caps['top'][6] = np.nan                         # NaN in a cap counts as +inf
    dp, twin = session(z, SIDES, [caps], eps)
    finish(dp, twin)


@pytest.mark.parametrize('shape', [(70, 45), (64, 64)])
def test_one_step_visits_give_the_same_bytes(monkeypatch, shape):
    z = surface(shape)
    eps = auto_eps(z)
    caps = make_caps(z, SIDES, 'random')
    monkeypatch.setenv('PYDEM_FILL_LOCAL', '0')
    dp, twin = session(z, SIDES, [caps], eps)       # (compared with the twin inside)
    finish(dp, twin)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('auto', [False, True])
def test_warm_restart_equals_a_cold_session(shape, auto):
    z = surface(shape)
    eps = auto_eps(z) if auto else 0.0
    c1 = make_caps(z, SIDES, 'random', seed=1)
    rng = np.random.RandomState(2)
    c2 = {s: c1[s] - rng.uniform(0.0, 30.0, c1[s].size) * (rng.uniform(size=c1[s].size) < 0.5) for s in SIDES}
    warm, twin_warm = session(z, SIDES, [c1, c2], eps)
    cold, twin_cold = session(z, SIDES, [c2], eps)
    assert device_W(warm).tobytes() == device_W(cold).tobytes() == twin_cold.W.tobytes()
    out = warm.fill_seam_relax(eps, c2)             # the caps repeat: the tile does not move
    assert out['n_lowered'] == 0 and device_W(warm).tobytes() == twin_cold.W.tobytes()
    out = warm.fill_seam_relax(eps, None)           # no line given: unchanged
    assert out['n_lowered'] == 0
    warm.fill_seam_end(False)
    finish(cold, twin_cold)


@pytest.mark.parametrize('shape', [(70, 45), (96, 80)])
@pytest.mark.parametrize('auto', [False, True])
def test_a_session_without_seam_lines_is_the_per_tile_fill(shape, auto):
    z = K.fractal(*shape)
    eps = auto_eps(z) if auto else 0.0
    ref = device(z)
    rW, rdepth = ref.calc_fill_depressions(eps, return_depth=True)
    dp = device(z)
    dp.fill_seam_begin(None)
    assert dp.fill_seam_relax(eps)['n_lowered'] > 0
    st = dp.fill_seam_end(True, return_depth=True)
    assert np.asarray(dp.elev).tobytes() == rW.tobytes() and dp.fill_depth.tobytes() == rdepth.tobytes()
    rs = ref.fill_depressions_stats
    assert (st['epsilon'], st['n_raised'], st['max_depth']) == (rs['epsilon'], rs['n_raised'], rs['max_depth'])
    assert st['passes'] == rs['passes']
    assert dp.elev.dtype == np.float64


def test_the_classic_fill_keeps_the_dtype_of_the_upload():
    z = np.rint(K.fractal(40, 50)).astype(np.int16)
    dp = device(z)
    dp.fill_seam_begin(None)
    dp.fill_seam_relax(0.0)
    dp.fill_seam_end(True)
    from pydem_amd import conditioning
    assert dp.elev.dtype == np.int16 and np.array_equal(dp.elev, conditioning.fill_depressions(z, 0.0)[0])


def test_session_memory_and_refusals():
    from pydem_amd import _ffi
    n, m = 70, 45
    z = surface((n, m))
    blocks = n * m * 8 + ((n + 31) // 32) * ((m + 31) // 32) * 4 + (2 * m + 2 * n) * 8
    seam = {s: np.ones(side_len(z.shape, s), bool) for s in SIDES}
    for commit in (False, True):
        dp = device(z)
        dp._ensure_tile()
        dp._push('elev')
        before = dp._tile.device_bytes()
        dp.fill_seam_begin(seam)
        assert dp._tile.device_bytes() == before + blocks
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp._tile.fill_seam_begin(seam)          # a second begin without an end
        assert dp._tile.device_bytes() == before + blocks
        with pytest.raises(_ffi.HipError, match='error -5'):
            dp.fill_seam_end(True)                  # +inf left: all four sides are seam lines and no cap has come
        caps = make_caps(z, SIDES, 'random')
        dp.fill_seam_relax(0.0, caps)
        W = device_W(dp)
        higher = dict(caps, left=caps['left'] + 1.0)
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp.fill_seam_relax(0.0, higher)         # a rising cap
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp.fill_seam_relax(0.5, caps)           # another epsilon
        assert device_W(dp).tobytes() == W.tobytes()
        dp.fill_seam_lines([(1, 3), (1, 7), (0, 2)])
        assert dp._tile.device_bytes() == before + blocks
        dp.fill_seam_end(commit)
        assert dp._tile.device_bytes() == before
        assert (np.asarray(dp.elev).tobytes() == z.tobytes()) == (not commit)
        with pytest.raises(_ffi.HipError, match='error -2'):
            dp._tile.fill_seam_relax(0.0)           # no session
    dp = device(z)
    dp.fill_seam_begin(seam)
    dp._tile.close()                                # destroying the tile with an open session frees it


def test_pass_limit_keeps_the_session_open(monkeypatch):
    from pydem_amd import _ffi
    z = K.fractal(96, 80)
    dp = device(z)
    dp.fill_seam_begin(None)
    monkeypatch.setenv('PYDEM_FILL_MAX_PASSES', '1')
    monkeypatch.setenv('PYDEM_FILL_LOCAL', '0')
    with pytest.raises(_ffi.HipError, match='error -5'):
        dp.fill_seam_relax(0.0)
    monkeypatch.delenv('PYDEM_FILL_MAX_PASSES')
    monkeypatch.delenv('PYDEM_FILL_LOCAL')
    dp.fill_seam_relax(0.0)                         # W was still an upper bound: the session goes on
    dp.fill_seam_end(True)
    from pydem_amd import conditioning
    assert np.asarray(dp.elev).tobytes() == conditioning.fill_depressions(z, 0.0)[0].tobytes()


def test_two_tiles_in_two_threads():
    shapes = [(70, 45), (64, 64)]
    errors = []

    def work(shape):
        try:
            z = surface(shape)
            dp, twin = session(z, SIDES, [make_caps(z, SIDES, 'random', seed=3), make_caps(z, SIDES, 'z')], auto_eps(z))
            finish(dp, twin)
        except BaseException as e:                  # (an assertion in a thread must fail the test)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(s,)) for s in shapes]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---- mosaics on one GPU
_FIELDS = {}


def field(name):
    if name not in _FIELDS:
        _FIELDS[name] = K.designed(*RASTER)[0] if name == 'designed' else K.fractal(*RASTER)
        _FIELDS[name].setflags(write=False)
    return _FIELDS[name]


@pytest.mark.parametrize('name', ['designed', 'fractal'])
@pytest.mark.parametrize('cut', [(2, 2, 1), (3, 3, 2), (2, 3, 3)])
@pytest.mark.parametrize('auto', [False, True])
def test_mosaic_tiles_equal_the_whole_raster_fill(name, cut, auto):
    from pydem_amd import DEMProcessor
    raster = field(name)
    eps = None if auto else 0.0
    pm = K.manager(raster, *cut, processor_cls=DEMProcessor, devices=[0])
    lat = pm.fill_lattice()
    W = K.whole_fill((name, eps), K.stitched(pm, lat), eps)
    pm.process_fill_depressions(eps)
    K.assert_tiles_equal_whole(pm, lat, W)
    if name == 'designed':
        assert pm.fill_rounds > 2
        assert K.per_tile_fill_differs(pm, lat, W, eps) > 0
    # duplicated cells agree: the stitched non-overlap surface is the whole-raster fill
    pm.compute_grid()
    pm.compute_grid_overlaps()
    out = pm.save_non_overlap_data(keys=('elev',))['elev']
    assert out.shape == W.shape and out.tobytes() == W.tobytes()
    st = pm.tiles[0].fill_depressions_stats
    assert st['passes'] >= 1 and st['ms'] > 0 and st['epsilon'] == pm.fill_depressions_epsilon_used


def test_mosaic_abort_leaves_the_tiles_untouched():
    from pydem_amd import DEMProcessor
    raster = field('designed')
    pm = K.manager(raster, 2, 3, 3, processor_cls=DEMProcessor, devices=[0])
    pm.process_elevation()
    before = [np.asarray(t.elev).tobytes() for t in pm.tiles]
    for t in pm.tiles:
        t._ensure_tile()
        t._push('elev')
    bytes_before = [t._tile.device_bytes() for t in pm.tiles]
    with pytest.raises(RuntimeError, match='max_rounds'):
        pm.process_fill_depressions(0.0, max_rounds=1)
    assert [np.asarray(t.elev).tobytes() for t in pm.tiles] == before
    assert [t._tile.device_bytes() for t in pm.tiles] == bytes_before
