"""CPU tier: the decaying and the transport-limited accumulation (DEMProcessor.calc_decay_accum / calc_trans_lim_accum,
pydem_fwd_accum) are part of the public surface and of the C-ABI, and refuse bad input before any device work."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _dp(**kw):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=np.arange(25, dtype=float).reshape(5, 5) + 1.0, dX=2.0, dY=3.0, fill_flats=False,
                      drain_pits_path=False, **kw)
    dp.mag = np.ones((5, 5)); dp.direction = np.ones((5, 5)); dp.flats = np.zeros((5, 5), bool)   # skip the device stencil
    return dp


def _untouched(dp):
    return (dp._tile is None and dp.decay_accum is None and dp.decay_accum_stats is None and dp.trans_lim_accum is None
            and dp.trans_lim_deposition is None and dp.trans_lim_stats is None)


def test_methods_and_attributes_exist():
    from pydem_amd import DEMProcessor
    sigs = {'calc_decay_accum': [('weights', inspect.Parameter.empty), ('decay', None), ('edge_nan', True)],
            'calc_trans_lim_accum': [('supply', inspect.Parameter.empty), ('capacity', inspect.Parameter.empty), ('edge_nan', True)]}
    for name, want in sigs.items():
        assert callable(getattr(DEMProcessor, name, None)), name
        sig = inspect.signature(getattr(DEMProcessor, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == want
    assert _untouched(_dp())


BAD_SHAPES = [np.ones((5, 4)), np.ones((4, 5)), np.ones(25), np.ones((1, 5, 5))]
NOT_FINITE = [np.nan, np.inf, -np.inf, np.where(np.eye(5) > 0, np.nan, 1.0), np.where(np.eye(5) > 0, np.inf, 1.0)]


@pytest.mark.parametrize('weights', BAD_SHAPES + NOT_FINITE)
def test_decay_accum_refuses_bad_weights(weights):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_decay_accum(weights)
    with pytest.raises(ValueError):
        dp.calc_decay_accum(weights, decay=0.5, edge_nan=False)
    assert _untouched(dp)


@pytest.mark.parametrize('decay', BAD_SHAPES + NOT_FINITE + [-0.01, 1.0 + 1e-12, 2.0, np.where(np.eye(5) > 0, 1.5, 0.5),
                                                             np.where(np.eye(5) > 0, -1e-300, 0.5), 'x'])
def test_decay_accum_refuses_a_decay_outside_0_1(decay):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_decay_accum(1.0, decay=decay)
    assert _untouched(dp)


@pytest.mark.parametrize('supply', BAD_SHAPES + NOT_FINITE + [-1.0, -1e-300, np.where(np.eye(5) > 0, -0.5, 1.0)])
def test_trans_lim_refuses_bad_supply(supply):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_trans_lim_accum(supply, 5.0)
    assert _untouched(dp)


@pytest.mark.parametrize('capacity', BAD_SHAPES + [np.nan, -np.inf, np.where(np.eye(5) > 0, np.nan, 1.0), -1.0, -1e-300,
                                                   np.where(np.eye(5) > 0, -0.5, np.inf), None])
def test_trans_lim_refuses_bad_capacity(capacity):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_trans_lim_accum(1.0, capacity)
    assert _untouched(dp)


def test_normalisation_of_scalars_and_masked_cells():
    dp = _dp()
    mask = np.eye(5) > 0
    for neutral, what in ((0.0, 'supply'), (1.0, 'decay'), (np.inf, 'capacity')):
        a = dp._plane_array(np.ma.masked_array(np.full((5, 5), 0.25), mask), what, neutral)
        assert a.dtype == np.float64 and a.flags['C_CONTIGUOUS'] and (a[mask] == neutral).all() and (a[~mask] == 0.25).all()
        b = dp._plane_array(3, what, neutral)
        assert b.shape == (5, 5) and (b == 3.0).all()
    assert (dp._plane_array(np.inf, 'capacity', np.inf) == np.inf).all()       # +inf is a capacity
    assert _untouched(dp)


@pytest.mark.parametrize('kw', [dict(drain_flats=True), dict(drain_pits_spill=True)])
def test_unimplemented_drainage_alternatives_fail_loudly(kw):
    dp = _dp(drain_pits=False, **kw)
    with pytest.raises(NotImplementedError):
        dp.calc_decay_accum(1.0)
    with pytest.raises(NotImplementedError):
        dp.calc_decay_accum(1.0, decay=0.5, edge_nan=False)
    with pytest.raises(NotImplementedError):
        dp.calc_trans_lim_accum(1.0, np.inf)
    with pytest.raises(ValueError):                                     # the argument checks still come first
        dp.calc_decay_accum(np.nan)
    with pytest.raises(ValueError):
        dp.calc_trans_lim_accum(1.0, -1.0)
    assert _untouched(dp)


def test_implicit_run_uca_and_no_cpu_fallback():
    """HipError where no GPU is visible; where one is, the calls compute the flow graph first and are served by the device."""
    from pydem_amd import _ffi
    try:
        n = _ffi.device_count()
    except _ffi.HipError:
        n = 0
    dp = _dp()
    if n == 0:
        with pytest.raises(_ffi.HipError):
            dp.calc_decay_accum(1.0)
        with pytest.raises(_ffi.HipError):
            dp.calc_trans_lim_accum(1.0, 2.0)
        assert dp.decay_accum is None and dp.decay_accum_stats is None and dp.trans_lim_accum is None and dp.trans_lim_stats is None
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            acc = dp.calc_decay_accum(1.0, decay=0.5, edge_nan=False)
            tr, dep = dp.calc_trans_lim_accum(1.0, 2.0, edge_nan=False)
        assert dp._has('uca')                                              # the implicit run_uca()
        assert acc is dp.decay_accum and acc.shape == (5, 5) and acc.dtype == np.float64 and (acc >= 1.0).all() and (acc < 2.0).all()
        assert set(dp.decay_accum_stats) == set(dp.trans_lim_stats) == {'ms', 'levels', 'n_unresolved', 'edge_nan'}
        assert tr is dp.trans_lim_accum and dep is dp.trans_lim_deposition and tr.shape == dep.shape == (5, 5)
        assert (tr <= 2.0).all() and (dep >= 0).all() and (dep[tr < 2.0] == 0).all()


def test_header_declares_the_export():
    text = open(os.path.join(ROOT, 'include', 'pydem_hip.h')).read()
    assert re.search(r'int\s+pydem_fwd_accum\s*\(\s*pydem_tile\s*\*\s*t\s*,\s*const\s+double\s*\*\s*load[^;]*const\s+double\s*\*\s*mult'
                     r'[^;]*const\s+double\s*\*\s*cap[^;]*int\s+edge_nan[^;]*double\s*\*\s*out[^;]*double\s*\*\s*out_inflow'
                     r'[^;]*double\s*\*\s*ms[^;]*int64_t\s*\*\s*levels[^;]*int64_t\s*\*\s*n_unresolved\s*\)\s*;', text)
    assert re.search(r'^ \*   pydem_fwd_accum\s', text, re.M)               # the list at the top of the header
    from pydem_amd import _ffi
    assert 'pydem_fwd_accum' in _ffi.SYMBOLS
    assert len(_ffi.SYMBOLS['pydem_fwd_accum'][1]) == 10
    sig = inspect.signature(_ffi.Tile.fwd_accum)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ('load', inspect.Parameter.empty), ('mult', None), ('cap', None), ('edge_nan', True), ('inflow', False), ('download', True)]


def test_library_exports_the_symbol():
    from pydem_amd import _ffi
    assert hasattr(_ffi.load(), 'pydem_fwd_accum')


def test_the_unit_is_part_of_the_build():
    from pydem_amd import build
    assert 'flowacc_fwd.hip' in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, 'pydem_amd', 'csrc', 'flowacc_fwd.hip'))
