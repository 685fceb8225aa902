"""CPU tier: upslope dependence, watersheds and reverse accumulation (DEMProcessor.calc_up_dependence / calc_watershed /
calc_rev_accum, pydem_rev_accum) are part of the public surface and of the C-ABI, and refuse bad input before any device work."""
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
    return (dp._tile is None and dp.up_dependence is None and dp.up_dependence_stats is None and dp.watershed is None
            and dp.rev_accum is None and dp.rev_accum_max is None and dp.rev_accum_stats is None)


def test_methods_and_attributes_exist():
    from pydem_amd import DEMProcessor
    sigs = {'calc_up_dependence': [('target', inspect.Parameter.empty)],
            'calc_watershed': [('outlets', inspect.Parameter.empty), ('min_fraction', 0.0)],
            'calc_rev_accum': [('weights', inspect.Parameter.empty)]}
    for name, want in sigs.items():
        assert callable(getattr(DEMProcessor, name, None)), name
        sig = inspect.signature(getattr(DEMProcessor, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == want
    assert _untouched(_dp())


@pytest.mark.parametrize('target', [np.ones((5, 4), bool), np.ones((4, 5), bool), np.ones(25, bool), True])
def test_dependence_refuses_a_wrong_shape(target):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_up_dependence(target)
    assert _untouched(dp)


@pytest.mark.parametrize('outlets', [[(5, 0)], [(0, 5)], [(-1, 2)], [(2, 2), (0, 7)], np.ones((5, 4), bool), [(0.5, 1.0)], [1, 2, 3]])
def test_watershed_refuses_bad_outlets(outlets):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_watershed(outlets)
    assert _untouched(dp)


@pytest.mark.parametrize('frac', [1.0, -0.01, 1.5, np.nan, np.inf, 'x', None])
def test_watershed_refuses_a_fraction_outside_0_1(frac):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_watershed([(2, 2)], min_fraction=frac)
    assert _untouched(dp)


@pytest.mark.parametrize('weights', [np.ones((4, 5)), np.nan, np.inf, np.where(np.eye(5) > 0, np.nan, 1.0), -np.inf * np.ones((5, 5))])
def test_rev_accum_refuses_bad_weights(weights):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_rev_accum(weights)
    assert _untouched(dp)


@pytest.mark.parametrize('kw', [dict(drain_flats=True), dict(drain_pits_spill=True)])
def test_unimplemented_drainage_alternatives_fail_loudly(kw):
    dp = _dp(drain_pits=False, **kw)
    with pytest.raises(NotImplementedError):
        dp.calc_up_dependence(np.ones((5, 5), bool))
    with pytest.raises(NotImplementedError):
        dp.calc_watershed([(1, 1)])
    with pytest.raises(NotImplementedError):
        dp.calc_rev_accum(1.0)
    with pytest.raises(ValueError):                                     # the argument checks still come first
        dp.calc_rev_accum(np.nan)


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
            dp.calc_watershed([(4, 4)])
        with pytest.raises(_ffi.HipError):
            dp.calc_rev_accum(1.0)
        assert dp.up_dependence is None and dp.watershed is None and dp.rev_accum is None and dp.rev_accum_stats is None
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ws = dp.calc_watershed([(4, 4)])
            racc, dmax = dp.calc_rev_accum(1.0)
        assert dp._has('uca')                                              # the implicit run_uca()
        assert ws.dtype == bool and ws.shape == (5, 5) and ws[4, 4] and dp.watershed is ws
        assert dp.up_dependence.dtype == np.float64 and dp.up_dependence[4, 4] == 1.0
        assert set(dp.up_dependence_stats) == {'ms', 'levels', 'n_unresolved'}
        assert racc is dp.rev_accum and dmax is dp.rev_accum_max and racc.shape == dmax.shape == (5, 5)
        assert set(dp.rev_accum_stats) == {'sum', 'max'} and set(dp.rev_accum_stats['sum']) == {'ms', 'levels', 'n_unresolved'}


def test_header_declares_the_export():
    text = open(os.path.join(ROOT, 'include', 'pydem_hip.h')).read()
    assert re.search(r'int\s+pydem_rev_accum\s*\(\s*pydem_tile\s*\*\s*t\s*,\s*int\s+op[^;]*const\s+double\s*\*\s*seed[^;]*const\s+uint8_t\s*\*\s*absorb'
                     r'[^;]*double\s+absorb_value[^;]*double\s*\*\s*out[^;]*double\s*\*\s*ms[^;]*int64_t\s*\*\s*levels[^;]*int64_t\s*\*\s*n_unresolved\s*\)\s*;', text)
    assert re.search(r'^ \*   pydem_rev_accum\s', text, re.M)               # the list at the top of the header
    from pydem_amd import _ffi
    assert 'pydem_rev_accum' in _ffi.SYMBOLS
    assert len(_ffi.SYMBOLS['pydem_rev_accum'][1]) == 9
    assert callable(getattr(_ffi.Tile, 'rev_accum', None))
    sig = inspect.signature(_ffi.Tile.rev_accum)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [('seed', None), ('absorb', None), ('absorb_value', 1.0), ('download', True)]


def test_library_exports_the_symbol():
    from pydem_amd import _ffi
    assert hasattr(_ffi.load(), 'pydem_rev_accum')
