"""GPU tier: pydem_depressions (csrc/depressions.hip) against the host twin (pydem_amd/conditioning.py: label_depressions, itself held
against a plain flood by tests/test_depressions_ref.py): the label raster and every column with array_equal, the fixed-point sums
as bits; block shapes; the schedules; that nothing else on the tile moves; the pass bound; the limited fill; outlets."""
import warnings

import numpy as np
import pytest

import depression_fields as D
import fill_fields as F
from depression_checks import same

pytestmark = pytest.mark.gpu


def cases():
    d = dict(D.builders())
    d.update(F.designed())
    d['fractal96'] = lambda: F.fractal(96, 80)
    d['fractal300'] = lambda: F.fractal(300, 260)
    d['fractal300_nan'] = lambda: F.fractal(300, 260, True)
    d['terraces_int16'] = F.terraces
    return d


_REF = {}


def ref(name, z, outlets=None, **kw):
    """(label, table, quanta) of the host twin, computed once per case"""
    key = (name, outlets is not None, tuple(sorted(kw.items())))
    if key not in _REF:
        from pydem_amd import conditioning
        _REF[key] = conditioning.label_depressions(z, outlets, dX2dY2=D.row_area(name, z.shape[0]), **kw)
    return _REF[key]


def device(name, z, outlets=None, **kw):
    from pydem_amd import DEMProcessor
    dp = DEMProcessor(elev=z, **D.spacing_kwargs(name))
    res = dp.calc_depressions(outlets, **kw)
    return dp, res


# 1. device against host twin
@pytest.mark.parametrize('name', sorted(cases()))
def test_device_against_host_twin(name):
    z = cases()[name]()
    dp, res = device(name, z)
    want = ref(name, z)
    same(res, want, dp.depressions_stats)
    assert dp.depressions_stats['n_found'] == len(want[1]) and dp.depressions_stats['passes'] >= 1
    assert dp.depressions_stats['ms']['total'] > 0
    if name == 'fractal96':
        assert len(res['table']) >= 50            # the input has not silently become trivial
    if name == 'checkerboard':
        assert len(res['table']) == 31 * 31
    if name == 'terraces_int16':
        assert dp.elev.dtype == np.int16 and len(res['table']) == 36


def test_filters_on_the_device():
    z = F.fractal(96, 80)
    full = ref('fractal96', z)[1]
    kw = dict(min_depth=float(np.median(full['max_depth'])), min_cells=3, min_volume=float(np.percentile(full['volume'], 30)))
    dp, res = device('fractal96', z, **kw)
    want = ref('fractal96', z, **kw)
    assert 0 < len(want[1]) < len(full) and dp.depressions_stats['n_found'] == len(full)
    same(res, want)
    assert device('fractal96', z, return_labels=False)[1]['label'] is None


# 2. block shapes
@pytest.mark.parametrize('shape', [(33, 65), (64, 64), (3, 3), (1, 7), (65, 33), (32, 97)])
@pytest.mark.parametrize('drop', [300.0, 1000.0])
def test_block_shapes(shape, drop):
    """The shapes of the fill's block-shape test with the interior lowered.  Lowered by 300 the relief of the surface (up to 658)
    still reaches above the lowest border cell, so the raised cells fall into several depressions (12, 12, 1, 7 and 17 on the five
    shapes the device takes): the cells of the table add up to the count of raised cells.  Lowered by 1000 every interior cell
    lies below every border cell: one depression, and its cells are the interior."""
    from pydem_amd import synth
    z = synth.fractal(shape[0], shape[1], seed=11, top_shift=4, n_octaves=4)
    if min(shape) >= 3:
        z[1:-1, 1:-1] -= drop                 # the interior of the border ring: depressions with relief
    name = 'shape%r%r' % (shape, drop)
    dp, res = device(name, z)
    want = ref(name, z)
    same(res, want, dp.depressions_stats)
    if min(shape) >= 3:
        raised = int((want[0] > 0).sum())
        assert raised >= 1 and res['table']['cells'].sum() == raised == (res['label'] > 0).sum()
        if drop == 1000.0 or shape == (3, 3):
            assert len(res['table']) == 1 and res['table']['cells'][0] == raised == (shape[0] - 2) * (shape[1] - 2)
    else:
        assert len(res['table']) == 0 and dp._tile is None        # the host path


# 3. schedule independence
@pytest.mark.parametrize('name', ['serpentine', 'comb', 'diagonal_chain', 'fractal96'])
def test_schedules_give_the_same_labels_and_table(monkeypatch, name):
    z = cases()[name]()
    want = ref(name, z)
    monkeypatch.setenv('PYDEM_DEPR_LOCAL', '0')
    dp, res = device(name, z)
    same(res, want, dp.depressions_stats)
    monkeypatch.setenv('PYDEM_DEPR_LOCAL', '1')
    monkeypatch.setenv('PYDEM_FILL_LOCAL', '0')
    dp, res = device(name, z)
    same(res, want, dp.depressions_stats)


# 4. nothing disturbed
def test_nothing_else_on_the_tile_moves():
    from pydem_amd import DEMProcessor, _ffi
    z = F.fractal(96, 80)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0)
        uca0 = dp.calc_uca().copy()
        elev0 = dp._tile.download(_ffi.ELEV)
        bytes0 = dp._tile.device_bytes()
        res = dp.calc_depressions()
        assert len(res['table']) >= 1
        assert dp._tile.device_bytes() == bytes0
        assert dp._tile.download(_ffi.ELEV).tobytes() == elev0.tobytes()
        assert dp._tile.download(_ffi.UCA).tobytes() == uca0.tobytes() and dp.uca.tobytes() == uca0.tobytes()
        # a following calc_uca (it conditions the resident surface once more) gives what it gives without the inventory
        control = DEMProcessor(elev=z, dX=30.0, dY=30.0)
        assert control.calc_uca().tobytes() == uca0.tobytes()
        again = control.calc_uca().copy()
        assert dp.calc_uca().tobytes() == again.tobytes()
        assert dp._tile.download(_ffi.ELEV).tobytes() == control._tile.download(_ffi.ELEV).tobytes()
        bytes0 = dp._tile.device_bytes()
        dp.calc_depressions()
        assert dp._tile.device_bytes() == bytes0
        # the raw surface of a float32 upload stays float32
        dp = DEMProcessor(elev=z.astype(np.float32), dX=30.0, dY=30.0)
        dp.calc_depressions()
        assert dp.elev.dtype == np.float32 and dp.elev.tobytes() == z.astype(np.float32).tobytes()


# 5. pass bound
def test_pass_bound_is_an_error_and_leaves_no_table(monkeypatch):
    from pydem_amd import DEMProcessor, _ffi
    z = F.serpentine()
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0)
    monkeypatch.setenv('PYDEM_FILL_MAX_PASSES', '1')
    with pytest.raises(_ffi.HipError, match='error -5'):
        dp.calc_depressions()
    assert dp.depressions is None
    rows = np.zeros(1, _ffi.Tile.DEPRESSION_ROW)
    assert dp._tile.lib.pydem_depressions_table(dp._tile._h, 1, rows.ctypes.data_as(_ffi.C.c_void_p)) == -2      # no table to read
    assert dp._tile.lib.pydem_depressions_table(dp._tile._h, 0, None) == 0
    monkeypatch.delenv('PYDEM_FILL_MAX_PASSES')
    assert dp._tile.download(_ffi.ELEV).tobytes() == z.tobytes()
    same(dp.calc_depressions(), ref('serpentine', z))


def test_bad_arguments_at_the_c_abi():
    from pydem_amd import _ffi
    z = D.two_levels()
    t = _ffi.Tile(*z.shape)
    t.upload(_ffi.ELEV, z)
    with pytest.raises(_ffi.HipError, match='error -3'):         # no spacing yet
        t.depressions()
    n = z.shape[0]
    t.set_spacing(np.full(n - 1, 30.0), np.full(n - 1, 30.0), np.full(n, 30.0), np.full(n, 30.0))
    for kw in (dict(min_depth=-1.0), dict(min_depth=float('nan')), dict(min_volume=-1.0), dict(min_cells=-1)):
        with pytest.raises(_ffi.HipError, match='error -2'):
            t.depressions(**kw)
    bad = z.copy()
    bad[5, 5] = np.inf
    t.upload(_ffi.ELEV, bad)
    with pytest.raises(_ffi.HipError, match='error -2'):
        t.depressions()
    t.upload(_ffi.ELEV, z)
    label, rows, info = t.depressions()
    assert len(rows) == 2 and info['n_found'] == 2 and list(rows['spill_elev']) == [80.0, 90.0]


# 6. limited fill
@pytest.mark.parametrize('name', ['limits', 'fractal96'])
def test_limited_fill_on_the_device(name):
    from pydem_amd import DEMProcessor, conditioning
    z = cases()[name]()
    limit = 20.0 if name == 'limits' else float(np.median(ref(name, z)[1]['max_depth']))
    want = conditioning.fill_depressions_limited(z, max_depth=limit, dX2dY2=D.row_area(name, z.shape[0]))
    dp = DEMProcessor(elev=z, dX=30.0, dY=30.0)
    W = dp.calc_fill_depressions_limited(max_depth=limit)
    assert W.tobytes() == want[0].tobytes() and np.array_equal(dp.kept_sinks, want[3]) and len(dp.kept_sinks) >= 1
    assert dp.fill_depressions_stats['epsilon'] == want[2]
    if name == 'limits':
        assert dp.kept_sinks.tolist() == [list(D.LIMITS_DEEP_BOTTOM)]
        dp = DEMProcessor(elev=z, dX=30.0, dY=30.0)
        with pytest.raises(RuntimeError, match='max_rounds'):
            dp.calc_fill_depressions_limited(max_depth=2.0, max_rounds=1)
        assert dp.elev.tobytes() == z.tobytes()


# 7. outlets
def test_an_outlet_at_the_bottom_removes_the_lake():
    z = D.limits()
    dp, res = device('limits', z, [D.LIMITS_DEEP_BOTTOM])
    out = np.zeros(z.shape, bool)
    out[D.LIMITS_DEEP_BOTTOM] = True
    same(res, ref('limits', z, out), dp.depressions_stats)
    t = res['table']
    assert len(t) == 2 and sorted(t['max_depth']) == [3.0, 10.0]       # the shallow cone and the pit inside the drained one
    assert res['label'][D.LIMITS_DEEP_BOTTOM] == 0
    # an outlet that is a sill makes the sill open
    z = D.two_levels()
    dp, res = device('two_levels', z, [(20, 9)])
    out = np.zeros(z.shape, bool)
    out[20, 9] = True
    same(res, ref('two_levels', z, out))
    assert list(res['table']['open_sill']) == [1, 0]
