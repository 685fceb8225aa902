"""CPU tier: the Python surface of the depression inventory (DEMProcessor.calc_depressions, calc_fill_depressions_limited):
argument checks before any device work, the host twin behind masked arrays and small tiles, the table's dtype, and that the
elevation is left alone."""
import numpy as np
import pytest

import depression_fields as D


def processor(z, **kw):
    from pydem_amd import DEMProcessor
    return DEMProcessor(elev=z, dX=30.0, dY=30.0, **kw)


@pytest.mark.parametrize('kw', [dict(min_depth=-1.0), dict(min_depth=float('nan')), dict(min_cells=-1), dict(min_volume=-0.5),
                                dict(min_volume=float('nan')), dict(min_depth='deep'), dict(min_depth=None),
                                dict(outlets=np.zeros((3, 3), bool)), dict(outlets=[(500, 2)])])
def test_calc_depressions_refuses_bad_arguments(kw):
    dp = processor(D.two_levels())
    with pytest.raises(ValueError):
        dp.calc_depressions(**kw)
    assert dp.depressions is None and dp._tile is None          # before any device work


@pytest.mark.parametrize('kw', [dict(max_depth=-1.0), dict(max_depth=float('nan')), dict(max_cells=-3), dict(max_volume=float('nan')),
                                dict(max_volume=-1.0), dict(max_depth=1.0, outlets=np.zeros((2, 2), bool))])
def test_limited_fill_refuses_bad_arguments(kw):
    z = D.limits()
    dp = processor(z)
    with pytest.raises(ValueError):
        dp.calc_fill_depressions_limited(**kw)
    assert dp._tile is None and dp.elev.tobytes() == z.tobytes()


def test_masked_array_is_served_by_the_host_twin():
    from pydem_amd import conditioning
    z = D.lake_nan_hole()
    masked = np.ma.masked_invalid(z)
    masked.data[masked.mask] = -9999.0                          # what lies under the mask does not count
    label, table, quanta = conditioning.label_depressions(masked)
    ref = conditioning.label_depressions(z)
    assert np.array_equal(label, ref[0]) and np.array_equal(table, ref[1]) and quanta == ref[2]
    assert table['open_sill'][0] == 1 and (label == -1).sum() == 9 and len(table) == 1
    W = conditioning.fill_depressions_limited(masked, max_depth=5.0)
    assert W[3].tolist() == [[table['bottom_row'][0], table['bottom_col'][0]]]


def as_objects(z):
    """the surface in a dtype the device cannot hold: DEMProcessor serves it on the host"""
    return np.asarray(z).astype(object)


def test_a_dtype_the_device_cannot_hold_is_served_by_the_host_twin():
    from pydem_amd import conditioning
    z = D.lake_nan_hole()
    dp = processor(as_objects(z))
    res = dp.calc_depressions()
    assert dp._tile is None
    label, table, quanta = conditioning.label_depressions(z, dX2dY2=np.full(z.shape[0], 900.0))
    assert np.array_equal(res['label'], label) and np.array_equal(res['table'], table)
    assert dp.depressions is res and dp.depressions_stats['quanta'] == quanta
    assert dp.calc_depressions(return_labels=False)['label'] is None


def test_table_dtype():
    from pydem_amd import conditioning
    dp = processor(np.array([[5.0, 1.0, 5.0, 0.0, 5.0, 2.0, 5.0]]))          # too small for the device: the host twin
    res = dp.calc_depressions()
    t = res['table']
    assert t.dtype == conditioning.DEPRESSION_DTYPE and t.shape == (0,)
    assert t.dtype.names == ('cells', 'r0', 'r1', 'c0', 'c1', 'spill_elev', 'bottom_row', 'bottom_col', 'bottom_elev', 'max_depth',
                             'pour_row', 'pour_col', 'n_sills', 'open_sill', 'area', 'volume', 'mean_depth')
    for nm in t.dtype.names:
        want = np.float64 if nm in ('spill_elev', 'bottom_elev', 'max_depth', 'area', 'volume', 'mean_depth') else np.int64
        assert t.dtype[nm] == want, nm
    assert res['label'].dtype == np.int32 and res['label'].shape == (1, 7) and not res['label'].any()


@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int16])
def test_calc_depressions_leaves_the_elevation_alone(dtype):
    z = (100 + 50 * np.cos(np.arange(60.0).reshape(2, 30))).astype(dtype)      # two rows: every cell is a border cell, the host serves it
    keep = z.copy()
    dp = processor(z)
    res = dp.calc_depressions()
    assert dp._tile is None and len(res['table']) == 0 and not res['label'].any()
    assert dp.elev.dtype == dtype and dp.elev.tobytes() == keep.tobytes()


def test_units_of_area_and_volume():
    z = as_objects(D.two_levels())
    dp = processor(z)
    res = dp.calc_depressions(min_cells=2)
    assert dp._tile is None and len(res['table']) == 2
    assert dp.elev.dtype == object and (dp.elev == D.two_levels()).all()
    # area and volume in the units of dX * dY and z * dX * dY: 400 cells of 900 m2, a flat bed 30 and 40 below the sills
    assert list(res['table']['area']) == [400 * 900.0, 400 * 900.0]
    assert list(res['table']['volume']) == [400 * 900.0 * 30.0, 400 * 900.0 * 40.0]
    assert list(res['table']['mean_depth']) == [30.0, 40.0]


def test_limited_fill_on_the_host_path():
    from pydem_amd import conditioning
    z = D.limits()
    dp = processor(as_objects(z))
    W = dp.calc_fill_depressions_limited(max_depth=20.0)
    ref = conditioning.fill_depressions_limited(z, max_depth=20.0, dX2dY2=np.full(z.shape[0], 900.0))
    assert dp._tile is None and np.asarray(W, dtype=np.float64).tobytes() == ref[0].tobytes() and np.array_equal(dp.kept_sinks, ref[3])
    assert dp.kept_sinks.tolist() == [list(D.LIMITS_DEEP_BOTTOM)] and dp.depressions is None
    dp = processor(as_objects(z))
    with pytest.raises(RuntimeError, match='max_rounds'):
        dp.calc_fill_depressions_limited(max_depth=2.0, max_rounds=1)
    assert (dp.elev == z).all() and dp.kept_sinks is None
