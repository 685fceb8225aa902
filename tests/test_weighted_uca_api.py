"""CPU tier: the weighted flow accumulation (DEMProcessor.calc_weighted_uca / run_weighted_uca, pydem_uca_weighted) is part of
the public surface and of the C-ABI, and refuses bad input before any device work."""
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


def test_method_and_attribute_exist():
    from pydem_amd import DEMProcessor
    from pydem_amd.dem_processing import _FIELD_OF
    assert callable(getattr(DEMProcessor, 'calc_weighted_uca', None))
    assert callable(getattr(DEMProcessor, 'run_weighted_uca', None))
    assert 'uca_weighted' in _FIELD_OF
    assert _dp().uca_weighted is None


@pytest.mark.parametrize('w', [np.ones((5, 4)), np.ones((4, 5)), np.ones(25), np.ones((5, 5, 1))])
def test_wrong_shape_is_refused_before_device_work(w):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_weighted_uca(w)
    assert dp._tile is None


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_weights_are_refused_before_device_work(bad):
    dp = _dp()
    w = np.ones((5, 5)); w[2, 3] = bad
    with pytest.raises(ValueError):
        dp.calc_weighted_uca(w)
    with pytest.raises(ValueError):
        dp.run_weighted_uca(bad)                  # a scalar broadcasts, and is checked the same way
    assert dp._tile is None


def test_weights_are_normalised_on_the_host():
    dp = _dp()
    w = dp._weights_array(2)
    assert w.dtype == np.float64 and w.shape == (5, 5) and (w == 2).all()
    m = np.ma.masked_array(np.full((5, 5), 3, np.int32), mask=np.eye(5, dtype=bool))
    w = dp._weights_array(m)
    assert w.dtype == np.float64 and (np.diag(w) == 0).all() and w[0, 1] == 3.0
    w = dp._weights_array(np.arange(25, dtype=np.float32).reshape(5, 5) - 12)      # negative and zero weights are fine
    assert w.dtype == np.float64 and w.min() == -12 and (w == 0).sum() == 1


@pytest.mark.parametrize('kw', [dict(drain_flats=True), dict(drain_pits_spill=True)])
def test_unimplemented_drainage_alternatives_fail_loudly(kw):
    dp = _dp(drain_pits=False, **kw)
    with pytest.raises(NotImplementedError):
        dp.run_weighted_uca(1.0)


def test_no_cpu_fallback_without_a_device():
    from pydem_amd import _ffi
    try:
        n = _ffi.device_count()
    except _ffi.HipError:
        n = 0
    if n > 0:
        pytest.skip("a GPU is visible")
    dp = _dp()
    with pytest.raises(_ffi.HipError):
        dp.calc_weighted_uca(np.ones((5, 5)))


def test_header_declares_the_export_and_the_fields():
    text = open(os.path.join(ROOT, 'include', 'pydem_hip.h')).read()
    assert re.search(r'int\s+pydem_uca_weighted\s*\(\s*pydem_tile\s*\*\s*t\s*,\s*pydem_options\s*\*\s*opt\s*,\s*int\s+scale_by_cell_area\s*\)\s*;', text)
    assert re.search(r'\bPYDEM_WEIGHT\s*=\s*10\b', text)
    assert re.search(r'\bPYDEM_UCA_WEIGHTED\s*=\s*11\b', text)
    assert re.search(r'\bPYDEM_FIELD_COUNT\s*=\s*12\b', text)
    from pydem_amd import _ffi
    assert (_ffi.WEIGHT, _ffi.UCA_WEIGHTED) == (10, 11)
    assert _ffi.FIELD_DTYPE[_ffi.WEIGHT] == np.float64 and _ffi.FIELD_DTYPE[_ffi.UCA_WEIGHTED] == np.float64
    assert 'pydem_uca_weighted' in _ffi.SYMBOLS
    assert _ffi.Timings._fields_[-1][0] == 'uca_weighted_ms'
