"""CPU tier: the upslope flow-path distance (DEMProcessor.calc_dist_up, pydem_dist_up) is part of the public surface and of
the C-ABI, and refuses bad input before any device work."""
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


def test_method_and_attributes_exist():
    import inspect
    from pydem_amd import DEMProcessor
    assert callable(getattr(DEMProcessor, 'calc_dist_up', None))
    sig = inspect.signature(DEMProcessor.calc_dist_up)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [('kind', 'h'), ('stat', 'max'), ('edge_nan', True)]
    dp = _dp()
    assert dp.dist_up is None and dp.dist_up_stats is None


@pytest.mark.parametrize('kw', [dict(kind='x'), dict(kind='H'), dict(kind=0), dict(stat='mean'), dict(stat='avg'), dict(stat=None)])
def test_unknown_kind_or_statistic_is_refused_before_device_work(kw):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_dist_up(**kw)
    assert dp._tile is None and dp.dist_up is None and dp.dist_up_stats is None


@pytest.mark.parametrize('kw', [dict(drain_flats=True), dict(drain_pits_spill=True)])
def test_unimplemented_drainage_alternatives_fail_loudly(kw):
    dp = _dp(drain_pits=False, **kw)
    with pytest.raises(NotImplementedError):
        dp.calc_dist_up()
    with pytest.raises(NotImplementedError):
        dp.calc_dist_up(kind='v', stat='ave', edge_nan=False)


def test_implicit_run_uca_and_no_cpu_fallback():
    """HipError where no GPU is visible; where one is, the call computes the flow graph first and is served by the device."""
    from pydem_amd import _ffi
    try:
        n = _ffi.device_count()
    except _ffi.HipError:
        n = 0
    dp = _dp()
    if n == 0:
        with pytest.raises(_ffi.HipError):
            dp.calc_dist_up()
        assert dp.dist_up is None and dp.dist_up_stats is None
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            d = dp.calc_dist_up(kind='s', stat='min', edge_nan=False)
        assert dp._has('uca')                                              # the implicit run_uca()
        assert d.shape == (5, 5) and d.dtype == np.float64 and dp.dist_up is d and not np.isnan(d).any() and (d >= 0).all()
        st = dp.dist_up_stats
        assert set(st) == {'ms', 'levels', 'n_unresolved', 'kind', 'stat', 'edge_nan'}
        assert (st['kind'], st['stat'], st['edge_nan'], st['n_unresolved']) == ('s', 'min', False, 0) and st['levels'] >= 1


def test_header_declares_the_export():
    text = open(os.path.join(ROOT, 'include', 'pydem_hip.h')).read()
    assert re.search(r'int\s+pydem_dist_up\s*\(\s*pydem_tile\s*\*\s*t\s*,\s*int\s+kind[^;]*int\s+stat[^;]*int\s+edge_nan[^;]*double\s*\*\s*out'
                     r'[^;]*double\s*\*\s*ms[^;]*int64_t\s*\*\s*levels[^;]*int64_t\s*\*\s*n_unresolved\s*\)\s*;', text)
    from pydem_amd import _ffi
    assert 'pydem_dist_up' in _ffi.SYMBOLS
    assert len(_ffi.SYMBOLS['pydem_dist_up'][1]) == 8
    assert callable(getattr(_ffi.Tile, 'dist_up', None))


def test_library_exports_the_symbol():
    from pydem_amd import _ffi
    assert hasattr(_ffi.load(), 'pydem_dist_up')
