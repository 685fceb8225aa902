"""The step without its redundant mask passes, copies and host waits (PYDEM_STEP_LEAN) against the
step with them (PYDEM_STEP_LEAN=0): every plane after every call, the pit lists and the graph words must be the same
bits.  pydem_find_flats only does the work its result needs (pydem_tile.flats_state); the tests below also check that
what the tile claims to know about its mask is true, and that every writer of mag / flats makes it forget.

The search the invariant rests on: 2000 random 24 x 24 tiles of integer heights 0..3 with up to three NaN cells (CPU
oracle, seed 20261018) hold 1456 tiles on which the one-pixel extension of the flats stage clears a cell the stencil
marked flat -- always at or next to a NaN cell.  The first of them is tests/golden/step_lean_cleared_flat.npz (8 cleared
cells, 3 of them NaN themselves); there the device counter must send pydem_find_flats through its full pass."""
import functools
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

SHAPES = [(96, 80), (257, 300)]
KINDS = ['fractal', 'srtm_int16', 'fractal_nan', 'tilted', 'constant', 'no_pit_patch']
NAN_FREE = ('fractal', 'srtm_int16', 'tilted', 'constant', 'no_pit_patch')


@functools.lru_cache(maxsize=None)
def _elev(kind, shape):
    from pydem_amd import synth
    n, m = shape
    if kind == 'fractal':
        return synth.fractal(n, m, seed=5, top_shift=6, n_octaves=6)
    if kind == 'srtm_int16':
        return synth.srtm_int16(n, m, seed=3, top_shift=6, n_octaves=6).astype(np.int16)
    if kind == 'fractal_nan':
        z = synth.fractal(n, m, seed=6, top_shift=6, n_octaves=6)
        z[n // 3:n // 3 + 7, m // 2:m // 2 + 5] = np.nan
        z[0, m // 4] = np.nan
        z[n // 2, m - 1] = np.nan
        return z
    if kind == 'tilted':
        i, j = np.mgrid[0:n, 0:m]
        return 10.0 + 0.5 * i + 0.25 * j
    if kind == 'constant':
        # all flat.  Above sea level every cell is also a pit candidate that grows for all 300 iterations without finding a drain
        # (4 s per run at 257 x 300, the same with and without the lean step): the small tile takes that road, the large one lies
        # below sea level, where the mask kernels see the same all-flat plane and the pit search has nothing to do
        return np.full((n, m), 7.0 if n * m < 10000 else -7.0)
    if kind == 'no_pit_patch':
        # flats, but none above sea level: no pit candidate, so the graph stage patches nothing
        return np.rint(synth.fractal(n, m, seed=7, top_shift=6, n_octaves=6, zrange=40.0)) - 100.0
    raise ValueError(kind)


def _processor(kind, shape):
    from pydem_amd import DEMProcessor
    return DEMProcessor(elev=_elev(kind, shape), dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)


class _Lean(object):
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get('PYDEM_STEP_LEAN')
        os.environ['PYDEM_STEP_LEAN'] = '1' if self.on else '0'

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop('PYDEM_STEP_LEAN', None)
        else:
            os.environ['PYDEM_STEP_LEAN'] = self.old


def _planes(dp, tag, out):
    from pydem_amd import _ffi
    for nm, f in (('mag', _ffi.MAG), ('direction', _ffi.DIRECTION), ('flats', _ffi.FLATS)):
        out['%s/%s' % (tag, nm)] = dp._tile.download(f)


def _results(dp, out):
    from pydem_amd import _ffi
    t = dp._tile
    for nm, f in (('section', _ffi.SECTION), ('proportion', _ffi.PROPORTION), ('uca', _ffi.UCA), ('edge_todo', _ffi.EDGE_TODO),
                  ('edge_done', _ffi.EDGE_DONE), ('twi', _ffi.TWI)):
        out[nm] = t.download(f)
    src, dst, w = t.pit_edges()
    order = np.lexsort((dst, src))
    out['pit_src'], out['pit_dst'], out['pit_w'] = src[order], dst[order], w[order]
    out['graph_words'] = t.graph_words()
    tm = t.timings()
    out['counts'] = np.array([tm['n_flats'], tm['n_pit_edges'], tm['n_pits'], tm['n_pits_undrained']])


def _step(dp, path, out, tag=''):
    """one pass of the hot path; path 'dp': the DEMProcessor calls, 'pm': the order of ProcessManager's workers"""
    if path == 'dp':
        dp.run_slopes_directions(); _planes(dp, tag + 'slopes', out)
        dp.run_uca(); _planes(dp, tag + 'uca', out)
        dp.run_twi(); _planes(dp, tag + 'twi', out)
    else:
        dp.run_slopes_directions(); _planes(dp, tag + 'slopes', out)
        dp.find_flats(); _planes(dp, tag + 'find_flats_1', out)
        dp.run_uca(); _planes(dp, tag + 'uca', out)
        dp.restore_pit_slopes(); _planes(dp, tag + 'restore', out)       # (flats as a caller reads it between the two calls)
        dp.find_flats(); _planes(dp, tag + 'find_flats_2', out)
        dp.run_twi(); _planes(dp, tag + 'twi', out)


@functools.lru_cache(maxsize=None)
def _trace(kind, shape, path, lean):
    out = {}
    with _Lean(lean), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = _processor(kind, shape)
        _step(dp, path, out)
        _results(dp, out)
        out['find_flats'] = np.array(dp._tile.flats_state())
    return out


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8) if a.dtype.kind == 'f' else a, b.view(np.uint8) if b.dtype.kind == 'f' else b), what


@pytest.mark.parametrize('path', ['dp', 'pm'])
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('kind', KINDS)
def test_lean_step_is_bit_identical_to_the_full_step(kind, shape, path):
    on, off = _trace(kind, shape, path, True), _trace(kind, shape, path, False)
    assert sorted(on) == sorted(off)
    for key in sorted(on):
        if key != 'find_flats':
            _same(on[key], off[key], '%s of %s %s (%s order)' % (key, kind, shape, path))
    if path == 'pm':
        # PYDEM_STEP_LEAN=0 runs the full pass on every call; the lean step never does on a tile without NaN
        assert tuple(off['find_flats'][1:]) == (2, 0, 0)
        if kind in NAN_FREE:
            assert on['find_flats'][1] == 0 and on['find_flats'][2] + on['find_flats'][3] == 2, on['find_flats']
        # whichever way it got there, the mask the worker's TWI call sees is slope == -1
        assert np.array_equal(on['find_flats_2/flats'] != 0, on['find_flats_2/mag'] == -1.0)
        assert np.array_equal(on['find_flats_1/flats'] != 0, on['find_flats_1/mag'] == -1.0)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('kind', KINDS)
def test_the_tile_only_claims_what_holds_after_slopes_directions(kind, shape):
    """pydem_find_flats may be skipped behind pydem_slopes_directions only when flats == (mag == -1) on the planes as
    they are; without NaN no flat cell has a flat neighbour of another height, so the claim is also always made."""
    from pydem_amd import _ffi
    with _Lean(True):
        dp = _processor(kind, shape)
        dp.run_slopes_directions()
        state = dp._tile.flats_state()[0]
        holds = np.array_equal(dp._tile.download(_ffi.FLATS) != 0, dp._tile.download(_ffi.MAG) == -1.0)
    assert state in (0, 1)
    assert holds or state == 0
    if kind in NAN_FREE:
        assert holds and state == 1


def test_a_flat_the_extension_clears_sends_find_flats_through_the_full_pass():
    """The golden tile of the search in the module docstring: the extension turns stencil flats off, the reference's
    later find_flats turns them on again -- so must this one, by its full pass."""
    from oracle import oracle as O
    from pydem_amd import DEMProcessor, _ffi
    g = np.load(os.path.join(GOLDEN_DIR, 'step_lean_cleared_flat.npz'))
    o = O.OracleDEM(g['elev'], dX=30.0, dY=30.0)
    o.calc_slopes_directions()
    assert np.array_equal(o.flats, g['flats']) and np.array_equal(o.mag, g['mag'], equal_nan=True)
    assert ((o.mag == -1) & (o.flats == 0)).sum() == 8          # what makes this tile the case
    with _Lean(True):
        dp = DEMProcessor(elev=g['elev'], dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False, drain_pits=True)
        dp.run_slopes_directions()
        t = dp._tile
        assert t.flats_state()[0] == 0
        assert np.array_equal(t.download(_ffi.FLATS), g['flats'])
        assert np.array_equal(t.download(_ffi.MAG), g['mag'], equal_nan=True)
        dp.find_flats()
        assert t.flats_state() == (1, 1, 0, 0)
        assert np.array_equal(t.download(_ffi.FLATS) != 0, o.mag == -1)         # reference :305-306 on the oracle's slopes


def _find_and_check(dp, what):
    from pydem_amd import _ffi
    dp.find_flats()
    flats, mag = dp._tile.download(_ffi.FLATS), dp._tile.download(_ffi.MAG)
    assert np.array_equal(flats != 0, mag == -1.0), what
    return flats, mag


@pytest.mark.parametrize('shape', SHAPES)
def test_every_writer_of_mag_or_flats_makes_the_tile_forget(shape):
    from pydem_amd import _ffi
    n, m = shape
    with _Lean(True), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = _processor('srtm_int16', shape)
        dp.run_slopes_directions()
        assert dp._tile.flats_state()[0] == 1
        # an upload of mag
        mag = np.array(dp.mag)
        flat = np.flatnonzero(mag.ravel() == -1.0)
        assert flat.size > 4
        mag.ravel()[flat[::2]] = 0.25
        mag[1::7, 2::5] = -1.0
        dp.mag = mag
        flats, got = _find_and_check(dp, 'after an upload of mag')
        assert np.array_equal(got, mag)
        # a line of mag, then a line of flats
        row = np.where(np.arange(m) % 3 == 0, -1.0, 0.5)
        dp.set_line('mag', 0, n // 2, row)
        _find_and_check(dp, 'after set_line on mag (row)')
        col = np.where(np.arange(n) % 4 == 1, -1.0, 2.0)
        dp.set_line('mag', 1, m - 2, col)
        _find_and_check(dp, 'after set_line on mag (column)')
        dp.set_line('flats', 0, 3, np.ones(m, np.uint8))
        _find_and_check(dp, 'after set_line on flats (row)')
        dp.set_line('flats', 1, 5, (np.arange(n) % 2).astype(np.uint8))
        _find_and_check(dp, 'after set_line on flats (column)')
        # the weighted accumulation, with a graph of its own (mag / flats patched and put back) and on the tile's graph
        dp = _processor('srtm_int16', shape)
        dp.run_slopes_directions()
        before = dp._tile.download(_ffi.MAG)
        dp.calc_weighted_uca(1.0)
        _, got = _find_and_check(dp, 'after calc_weighted_uca without a graph')
        assert np.array_equal(got, before)
        dp.run_uca()
        dp.calc_weighted_uca(2.0)
        _find_and_check(dp, 'after calc_weighted_uca on the graph of calc_uca')
        # restore_pit_slopes twice, and behind it a call that has nothing left to do
        dp.restore_pit_slopes()
        dp.restore_pit_slopes()
        _find_and_check(dp, 'after restore_pit_slopes twice')
        _find_and_check(dp, 'a second find_flats')
        # restore_pit_slopes without a graph: on a fresh tile, and with the pit list of a graph an elevation write has invalidated
        dq = _processor('srtm_int16', shape)
        dq.run_slopes_directions()
        dq.restore_pit_slopes()
        _find_and_check(dq, 'after restore_pit_slopes on a tile without a graph')
        dp.run_uca()
        dp.set_line('elev', 0, 0, np.asarray(dp.get_line('elev', 0, 0), np.float64))
        dp.restore_pit_slopes()
        _find_and_check(dp, 'after restore_pit_slopes behind an elevation write')
        # the conditioning uses mag and flats as work planes
        dp = _processor('srtm_int16', shape)
        dp.run_slopes_directions()
        dp.find_flats()
        mag = np.array(dp.mag)
        dp.calc_fill_flats()
        dp.mag = mag
        _, got = _find_and_check(dp, 'after calc_fill_flats')
        assert np.array_equal(got, mag)


@pytest.mark.parametrize('kind', ['fractal', 'srtm_int16', 'fractal_nan'])
def test_a_second_step_on_the_same_tile_repeats_the_first(kind):
    """the benchmark's pattern: the same tile, step after step"""
    shape = SHAPES[1]
    first, second = {}, {}
    with _Lean(True), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = _processor(kind, shape)
        _step(dp, 'pm', first); _results(dp, first)
        _step(dp, 'pm', second); _results(dp, second)
        counts = dp._tile.flats_state()
    for key in sorted(first):
        _same(first[key], second[key], '%s of step 2 (%s)' % (key, kind))
    ref = _trace(kind, shape, 'pm', False)
    for key in sorted(first):
        _same(first[key], ref[key], '%s against the full step (%s)' % (key, kind))
    if kind in NAN_FREE:
        assert counts[1] == 0 and counts[2] + counts[3] == 4, counts
