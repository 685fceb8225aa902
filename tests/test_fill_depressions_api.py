"""CPU tier: DEMProcessor.calc_fill_depressions / run_fill_depressions check their arguments before the library is touched, the
two options are constructor keywords, and they are off by default."""
import numpy as np
import pytest

import fill_fields as F


@pytest.fixture
def dp(monkeypatch):
    from pydem_amd import DEMProcessor, _ffi

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_ffi, 'load', no_library)
    monkeypatch.setattr(_ffi, 'Tile', no_library)
    return DEMProcessor(elev=F.bowl(), dX=30.0, dY=30.0)


@pytest.mark.parametrize('eps', [-1.0, -1e-300, float('nan'), float('inf'), -float('inf'), 'x', 2.0 ** -45])
def test_bad_epsilon(dp, eps):
    with pytest.raises(ValueError):
        dp.calc_fill_depressions(eps)
    with pytest.raises(ValueError):
        dp.run_fill_depressions(epsilon=eps)
    assert dp._tile is None


def test_bad_outlets(dp):
    n, m = F.BOWL_SHAPE
    for bad in (np.zeros((n, m + 1), bool), np.zeros((3, 3), bool), [(n, 0)], [(0, m)], [(-1, 5)], [(1, 2), (3, -4)],
                np.zeros((n, m, 2), bool), [(1.5, 2.0)]):
        with pytest.raises(ValueError):
            dp.calc_fill_depressions(0.0, outlets=bad)
    assert dp._tile is None


def test_outlet_pairs_and_mask_are_the_same_mask(dp):
    n, m = F.BOWL_SHAPE
    mask = np.zeros((n, m), bool)
    mask[F.BOWL_BOTTOM] = mask[3, 7] = True
    assert np.array_equal(dp._outlets_mask([F.BOWL_BOTTOM, (3, 7)]), mask)
    assert np.array_equal(dp._outlets_mask(mask), mask)
    assert np.array_equal(dp._outlets_mask(mask.astype(np.uint8)), mask)


def test_options_are_constructor_keywords_and_off_by_default():
    from pydem_amd import DEMProcessor
    assert DEMProcessor.fill_depressions is False and DEMProcessor.fill_depressions_epsilon is None
    assert 'fill_depressions' in DEMProcessor._OPTION_NAMES and 'fill_depressions_epsilon' in DEMProcessor._OPTION_NAMES
    z = F.bowl()
    dp = DEMProcessor(elev=z)
    assert dp.fill_depressions is False and dp.fill_depressions_epsilon is None
    dp = DEMProcessor(elev=z, fill_depressions=True, fill_depressions_epsilon=0.0)
    assert dp.fill_depressions is True and dp.fill_depressions_epsilon == 0.0
    assert dp.fill_depressions_stats is None and dp.fill_depth is None


def test_tiles_too_small_for_the_device_go_through_the_host(dp):
    """fewer than three rows: no library, same contract"""
    from pydem_amd import DEMProcessor
    thin = np.array([[5, 1, 7, 0, 3, 9, 2]], np.int16)
    p = DEMProcessor(elev=thin)
    out, depth = p.calc_fill_depressions(0.0, return_depth=True)
    assert out.dtype == np.int16 and np.array_equal(out, thin) and not depth.any()
    assert p.fill_depressions_stats == dict(epsilon=0.0, n_raised=0, max_depth=0.0, passes=0, ms=0.0)
    out = p.calc_fill_depressions()
    assert out.dtype == np.float64 and np.array_equal(out, thin) and p.fill_depressions_stats['epsilon'] == 2.0 ** -32 * 16
    assert p._tile is None and p.fill_depth is None
