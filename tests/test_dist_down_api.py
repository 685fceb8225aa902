"""CPU tier: the downslope distance (DEMProcessor.calc_dist_down / calc_hand, pydem_dist_down) is part of the public surface
and of the C-ABI, and refuses bad input before any device work."""
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


def test_methods_and_attributes_exist():
    from pydem_amd import DEMProcessor
    assert callable(getattr(DEMProcessor, 'calc_dist_down', None))
    assert callable(getattr(DEMProcessor, 'calc_hand', None))
    dp = _dp()
    assert dp.dist_down is None and dp.hand is None


@pytest.mark.parametrize('kw', [dict(), dict(target=np.ones((5, 5), bool), uca_threshold=3.0)])
def test_exactly_one_target_form(kw):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_dist_down(**kw)
    with pytest.raises(ValueError):
        dp.calc_hand(**kw)
    assert dp._tile is None


@pytest.mark.parametrize('mask', [np.ones((5, 4), bool), np.ones((4, 5), bool), np.ones(25, bool), np.ones((5, 5, 1), bool)])
def test_wrong_mask_shape_is_refused_before_device_work(mask):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_dist_down(target=mask)
    with pytest.raises(ValueError):
        dp.calc_hand(target=mask)
    assert dp._tile is None


@pytest.mark.parametrize('thr', [np.nan, np.inf, -np.inf, -1.0, -1e-300, 'streams'])
def test_bad_threshold_is_refused_before_device_work(thr):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_dist_down(uca_threshold=thr)
    with pytest.raises(ValueError):
        dp.calc_hand(uca_threshold=thr)
    assert dp._tile is None


@pytest.mark.parametrize('kw', [dict(kind='x'), dict(kind='H'), dict(kind=0), dict(stat='mean'), dict(stat='avg'), dict(stat=None)])
def test_unknown_kind_or_statistic_is_refused_before_device_work(kw):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_dist_down(uca_threshold=10.0, **kw)
    assert dp._tile is None


def test_masked_target_counts_masked_cells_as_not_target():
    dp = _dp()
    t = np.ma.masked_array(np.ones((5, 5), bool), mask=np.eye(5, dtype=bool))
    mask, thr = dp._stream_set(t, None)
    assert thr is None and mask.dtype == bool and mask.shape == (5, 5)
    assert not np.diag(mask).any() and mask.sum() == 20
    mask, thr = dp._stream_set(None, 0)                               # a threshold of zero is a threshold
    assert mask is None and thr == 0.0


@pytest.mark.parametrize('kw', [dict(drain_flats=True), dict(drain_pits_spill=True)])
def test_unimplemented_drainage_alternatives_fail_loudly(kw):
    dp = _dp(drain_pits=False, **kw)
    with pytest.raises(NotImplementedError):
        dp.calc_dist_down(uca_threshold=10.0)
    with pytest.raises(NotImplementedError):
        dp.calc_hand(uca_threshold=10.0)


def test_no_cpu_fallback_without_a_device():
    """HipError where no GPU is visible; where one is, the same call is served by it."""
    from pydem_amd import _ffi
    try:
        n = _ffi.device_count()
    except _ffi.HipError:
        n = 0
    dp = _dp()
    if n == 0:
        with pytest.raises(_ffi.HipError):
            dp.calc_dist_down(target=np.ones((5, 5), bool))
        with pytest.raises(_ffi.HipError):
            dp.calc_hand(uca_threshold=1.0)
        assert dp.dist_down is None and dp.hand is None
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            d = dp.calc_dist_down(target=np.ones((5, 5), bool))
        assert d.shape == (5, 5) and (d == 0).all() and dp.dist_down is d


def test_header_declares_the_export():
    text = open(os.path.join(ROOT, 'include', 'pydem_hip.h')).read()
    assert re.search(r'int\s+pydem_dist_down\s*\(\s*pydem_tile\s*\*\s*t\s*,\s*int\s+kind[^;]*const\s+uint8_t\s*\*\s*target[^;]*double\s+uca_threshold'
                     r'[^;]*double\s*\*\s*out[^;]*double\s*\*\s*ms[^;]*int64_t\s*\*\s*levels[^;]*int64_t\s*\*\s*n_unresolved\s*\)\s*;', text)
    assert re.search(r'\bPYDEM_FIELD_COUNT\s*=\s*12\b', text)
    from pydem_amd import _ffi
    assert 'pydem_dist_down' in _ffi.SYMBOLS
    assert len(_ffi.SYMBOLS['pydem_dist_down'][1]) == 9
    assert len(_ffi.FIELD_DTYPE) == 12
    assert _ffi.Timings._fields_[-1][0] == 'uca_weighted_ms'
    assert set(_ffi.Tile.DIST_KINDS) == {'h', 'v', 's'} and set(_ffi.Tile.DIST_STATS) == {'ave', 'min', 'max'}


def test_library_exports_the_symbol():
    from pydem_amd import _ffi
    assert hasattr(_ffi.load(), 'pydem_dist_down')
