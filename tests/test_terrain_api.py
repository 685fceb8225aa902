"""CPU tier: the terrain attributes (DEMProcessor.calc_terrain_attributes / calc_curvature / calc_hillshade,
pydem_terrain_attributes) are part of the public surface and of the C-ABI, refuse bad input before any device work, and have no
CPU fallback."""
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT
from pydem_amd import terrain as T


def _dp(**kw):
    from pydem_amd import DEMProcessor
    return DEMProcessor(elev=np.arange(49, dtype=float).reshape(7, 7) ** 1.5, dX=2.0, dY=3.0, fill_flats=False, drain_pits_path=False, **kw)


def _untouched(dp):
    return dp._tile is None and dp.terrain_attributes is None and dp.terrain_attributes_stats is None and not dp._on_device


def test_methods_and_attributes_exist():
    from pydem_amd import DEMProcessor, _ffi, build
    sigs = {'calc_terrain_attributes': [('which', ('gradient', 'aspect', 'profile', 'plan', 'tangential', 'mean')), ('window', 3),
                                        ('azimuth', 315.0), ('altitude', 45.0), ('z_factor', 1.0)],
            'calc_curvature': [('kind', 'profile'), ('window', 3)],
            'calc_hillshade': [('azimuth', 315.0), ('altitude', 45.0), ('z_factor', 1.0), ('window', 3)]}
    for name, want in sigs.items():
        assert callable(getattr(DEMProcessor, name, None)), name
        sig = inspect.signature(getattr(DEMProcessor, name))
        assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == want
    sig = inspect.signature(T.terrain_attributes_ref)
    assert list(sig.parameters) == ['elev', 'dX2', 'dY2', 'window', 'which', 'light', 'z_factor']
    assert 'pydem_terrain_attributes' in _ffi.SYMBOLS and callable(_ffi.Tile.terrain_attributes)
    assert 'terrain.hip' in build.SOURCES and os.path.exists(os.path.join(ROOT, 'pydem_amd', 'csrc', 'terrain.hip'))
    assert _untouched(_dp())


def test_the_plane_names_follow_the_enum():
    import re
    text = open(os.path.join(ROOT, 'include', 'pydem_hip.h')).read()
    body = re.search(r'enum pydem_terrain_attr \{(.*?)\};', text, re.S).group(1)
    ids = {k.lower(): int(v) for k, v in re.findall(r'PYDEM_TA_([A-Z]+) = (\d+)', body)}
    assert ids.pop('count') == len(T.ATTRIBUTES)
    assert [ids[nm] for nm in T.ATTRIBUTES] == list(range(len(T.ATTRIBUTES)))


@pytest.mark.parametrize('kw', [
    dict(window=1), dict(window=2), dict(window=4), dict(window=17), dict(window=-3), dict(window=3.0), dict(window='3'), dict(window=None),
    dict(window=True), dict(which=()), dict(which=[]), dict(which=('slope',)), dict(which=('gradient', 'curl')), dict(which=(3,)),
    dict(which=None), dict(altitude=0.0), dict(altitude=-10.0), dict(altitude=90.5), dict(altitude=np.nan), dict(altitude='high'),
    dict(azimuth=np.nan), dict(azimuth=np.inf), dict(azimuth=None), dict(z_factor=0.0), dict(z_factor=-1.0), dict(z_factor=np.nan),
    dict(z_factor=np.inf), dict(z_factor='x')])
def test_bad_arguments_are_refused_before_device_work(kw):
    dp = _dp()
    with pytest.raises(ValueError):
        dp.calc_terrain_attributes(**kw)
    assert _untouched(dp)


def test_the_wrappers_refuse_too():
    dp = _dp()
    for call in (lambda: dp.calc_curvature('gaussian'), lambda: dp.calc_curvature('gradient'), lambda: dp.calc_curvature(window=6),
                 lambda: dp.calc_hillshade(altitude=0), lambda: dp.calc_hillshade(z_factor=0), lambda: dp.calc_hillshade(window=16),
                 lambda: dp.calc_hillshade(azimuth=float('nan'))):
        with pytest.raises(ValueError):
            call()
    assert _untouched(dp)


def test_arguments_at_the_limits_are_accepted():
    assert [T.check_window(w) for w in (3, 5, 15, np.int64(7))] == [1, 2, 7, 3]
    assert T.check_which('mean') == ('mean',) and T.check_which(['plan', 'mean', 'plan']) == ('plan', 'mean')
    assert T.check_which(T.ATTRIBUTES) == T.ATTRIBUTES
    Le, Ln, Lu = T.light_vector(0.0, 90.0)
    assert Lu == 1.0 and abs(Le) < 1e-16 and abs(Ln) < 1e-16
    assert T.light_vector(-45.0, 45.0) == pytest.approx(T.light_vector(315.0, 45.0), abs=1e-15)


def test_no_cpu_fallback_without_a_device():
    from pydem_amd import _ffi
    try:
        n = _ffi.device_count()
    except _ffi.HipError:
        n = 0
    if n > 0:
        pytest.skip("a GPU is visible")
    for dp in (_dp(), __import__('pydem_amd').DEMProcessor(elev=np.ones((2, 9)), fill_flats=False, drain_pits_path=False)):
        for call in (dp.calc_terrain_attributes, dp.calc_curvature, dp.calc_hillshade):
            with pytest.raises(_ffi.HipError):
                call()
        assert dp.terrain_attributes is None and dp.terrain_attributes_stats is None
