"""CPU tier: the two comparators of tests/flowgraph_kit.py, which every GPU test of the flow-graph analyses relies on, pinned on
4 x 4 arrays; and the one coercion behind DEMProcessor._weights_array / _plane_array / _mask_array, where the test_*_api.py files
(which cover the refused inputs one by one) leave off: the fill of masked cells, the broadcast of scalars, layout and dtype, and
that a refused input has not touched the device."""
import numpy as np
import pytest

from flowgraph_kit import assert_bound, assert_same_bits


def _plane():
    a = np.linspace(-2.0, 5.0, 16).reshape(4, 4)
    a[1, 2] = np.nan
    a[3, 0] = 0.0
    return a


# ---- assert_same_bits
def test_same_bits_accepts_identical_arrays_with_nan():
    assert_same_bits(_plane(), _plane(), 'identical')


def test_same_bits_refuses_another_nan_pattern():
    b = _plane()
    b[0, 0] = np.nan
    with pytest.raises(AssertionError, match='NaN patterns differ'):
        assert_same_bits(_plane(), b, 'one more NaN')
    b = _plane()
    b[1, 2] = 1.0
    with pytest.raises(AssertionError, match='NaN patterns differ'):
        assert_same_bits(_plane(), b, 'one NaN less')


def test_same_bits_refuses_one_ulp():
    b = _plane()
    b[2, 2] = np.nextafter(b[2, 2], np.inf)
    with pytest.raises(AssertionError, match='1 cells differ in their bits'):
        assert_same_bits(_plane(), b, 'one ulp')


def test_same_bits_tells_the_zeros_apart():
    b = _plane()
    b[3, 0] = -0.0
    assert np.array_equal(_plane(), b, equal_nan=True)               # (== does not see it)
    with pytest.raises(AssertionError, match='1 cells differ in their bits'):
        assert_same_bits(_plane(), b, 'minus zero')


# ---- assert_bound
BOUND, FLOOR = 2.0 ** -30, 2.0 ** -40         # powers of two: bound * |refabs| + floor is exact for the values below


def _bound_case():
    """(ref, refabs, the limit per cell): small integers, refabs of both signs, so that ref + limit is exact; one NaN in ref"""
    ref = np.array([[1.0, -2.0, 0.0, 4.0], [-3.0, 2.0, np.nan, 1.0], [0.0, 5.0, -1.0, 2.0], [3.0, -4.0, 1.0, 0.0]])
    refabs = np.array([[3.0, -5.0, 1.0, 2.0], [8.0, 1.0, -7.0, 4.0], [2.0, 6.0, -1.0, 3.0], [5.0, 2.0, 4.0, -9.0]])
    return ref, refabs, BOUND * np.abs(refabs) + FLOOR


def test_bound_accepts_an_error_exactly_at_the_limit():
    ref, refabs, lim = _bound_case()
    ok = ~np.isnan(ref)
    for dev in (ref + lim, ref - lim):
        assert (np.abs(dev - ref)[ok] == lim[ok]).all()              # (the case is what it says: no rounding anywhere)
        assert_bound(dev, ref, refabs, 'at the limit', BOUND, FLOOR)
    assert_bound(ref + BOUND * np.abs(refabs), ref, refabs, 'at the limit, no floor', BOUND)


def test_bound_refuses_the_next_value_above_the_limit():
    ref, refabs, lim = _bound_case()
    ref[:] = np.where(np.isnan(ref), np.nan, 0.0)                   # around 0 the error is the device's value, exactly
    for cell in ((0, 0), (1, 1), (3, 3)):
        dev = ref.copy()
        dev[cell] = lim[cell]
        assert_bound(dev, ref, refabs, 'the limit itself', BOUND, FLOOR)
        dev[cell] = np.nextafter(lim[cell], np.inf)
        with pytest.raises(AssertionError, match='1 cells off'):
            assert_bound(dev, ref, refabs, 'one step above the limit', BOUND, FLOOR)
        dev[cell] = -np.nextafter(lim[cell], np.inf)
        with pytest.raises(AssertionError, match='1 cells off'):
            assert_bound(dev, ref, refabs, 'one step below the limit', BOUND, FLOOR)


def test_bound_refuses_another_nan_pattern():
    ref, refabs, _ = _bound_case()
    dev = ref.copy()
    dev[0, 3] = np.nan
    with pytest.raises(AssertionError, match='NaN patterns differ'):
        assert_bound(dev, ref, refabs, 'one more NaN', BOUND, FLOOR)
    dev = ref.copy()
    dev[1, 2] = 0.0
    with pytest.raises(AssertionError, match='NaN patterns differ'):
        assert_bound(dev, ref, refabs, 'one NaN less', BOUND, FLOOR)


def test_bound_without_a_floor_allows_nothing_where_refabs_is_zero():
    ref, refabs, _ = _bound_case()
    refabs[2, 1] = 0.0
    dev = ref.copy()
    assert_bound(dev, ref, refabs, 'no error', BOUND)                # the floor defaults to 0
    dev[2, 1] = np.nextafter(ref[2, 1], np.inf)
    with pytest.raises(AssertionError, match='1 cells off'):
        assert_bound(dev, ref, refabs, 'one ulp on a zero scale', BOUND, 0.0)
    assert_bound(dev, ref, refabs, 'one ulp on a zero scale, with a floor', BOUND, FLOOR)


# ---- the coercion, through its three named forms
def _dp(**kw):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=np.arange(25, dtype=float).reshape(5, 5) + 1.0, dX=2.0, dY=3.0, fill_flats=False,
                      drain_pits_path=False, **kw)
    dp.mag = np.ones((5, 5)); dp.direction = np.ones((5, 5)); dp.flats = np.zeros((5, 5), bool)   # skip the device stencil
    return dp


FORMS = [('weights', lambda dp, v: dp._weights_array(v), np.float64, 0.0),
         ('decay', lambda dp, v: dp._plane_array(v, 'decay', 1.0), np.float64, 1.0),
         ('capacity', lambda dp, v: dp._plane_array(v, 'capacity', np.inf), np.float64, np.inf),
         ('target', lambda dp, v: dp._mask_array(v, 'target'), bool, False)]


@pytest.mark.parametrize('what,form,dtype,neutral', FORMS)
def test_coercion_fills_masked_cells_and_gives_a_contiguous_plane(what, form, dtype, neutral):
    dp = _dp()
    base = np.arange(25).reshape(5, 5) % 2 if dtype is bool else np.arange(25, dtype=np.float32).reshape(5, 5) / 32
    for values in (base, base.T.copy().T, np.asfortranarray(base), base.astype(np.int16 if dtype is bool else np.float64)):
        a = form(dp, np.ma.masked_array(values, mask=np.eye(5, dtype=bool)))
        assert a.dtype == dtype and a.shape == (5, 5) and a.flags.c_contiguous and not np.ma.isMaskedArray(a)
        assert (np.diag(a) == neutral).all()
        off = ~np.eye(5, dtype=bool)
        assert np.array_equal(a[off], np.asarray(values)[off].astype(dtype))
        b = form(dp, values)                                          # unmasked: the values themselves
        assert b.dtype == dtype and b.flags.c_contiguous and np.array_equal(b, np.asarray(values).astype(dtype))
    assert dp._tile is None


@pytest.mark.parametrize('what,form,dtype,neutral', FORMS[:3])
def test_coercion_broadcasts_a_scalar(what, form, dtype, neutral):
    dp = _dp()
    for v in (0.25, 1, np.float32(0.5), np.array(0.75)):
        a = form(dp, v)
        assert a.dtype == np.float64 and a.shape == (5, 5) and a.flags.c_contiguous and (a == float(v)).all()
    assert dp._tile is None


def test_a_mask_does_not_broadcast_and_is_a_copy():
    dp = _dp()
    with pytest.raises(ValueError, match=r"target of shape \(\) for a tile of shape \(5, 5\)"):
        dp._mask_array(True, 'target')
    m = np.ones((5, 5), bool)
    out = dp._mask_array(m, 'target')
    assert out is not m and not np.shares_memory(out, m)
    assert dp._tile is None


@pytest.mark.parametrize('call,message', [
    (lambda dp: dp._weights_array(np.ones((5, 4))), r"weights of shape \(5, 4\) for a tile of shape \(5, 5\)"),
    (lambda dp: dp._weights_array(np.where(np.eye(5) > 0, np.nan, 1.0)), r"weights must be finite \(5 NaN / inf values\)"),
    (lambda dp: dp._weights_array(-np.inf), r"weights must be finite \(25 NaN / inf values\)"),
    (lambda dp: dp._plane_array(np.ones(25), 'supply', 0.0), r"supply of shape \(25,\) for a tile of shape \(5, 5\)"),
    (lambda dp: dp._plane_array(np.where(np.eye(5) > 0, np.nan, 1.0), 'decay', 1.0), r"decay must not be NaN \(5 NaN values\)"),
    (lambda dp: dp._plane_array('a lot', 'capacity', np.inf), r"capacity must be a number or an array of numbers"),
    (lambda dp: dp._mask_array(np.ones((5, 5, 1), bool), 'outlets'), r"outlets of shape \(5, 5, 1\) for a tile of shape \(5, 5\)"),
    (lambda dp: dp._stream_set(np.ones((4, 5), bool), None), r"target of shape \(4, 5\) for a tile of shape \(5, 5\)"),
    (lambda dp: dp.calc_reach_attributes(uca_threshold=1.0, values=np.ones((5, 6))), r"values of shape \(5, 6\) for a tile of shape \(5, 5\)"),
    (lambda dp: dp.calc_reach_attributes(uca_threshold=1.0, values=[['a'] * 5] * 5), r"values must be an array of numbers"),
])
def test_refused_input_names_itself_and_leaves_the_device_alone(call, message):
    dp = _dp()
    with pytest.raises(ValueError, match=message):
        call(dp)
    assert dp._tile is None
