"""GPU tier: the inventory part of the seam session (csrc/depressions.hip: pydem_fill_seam_label / _label_roots / _get_id_lines /
_inventory / _labels) against its host twin (pydem_amd/conditioning.py: SeamFill) on one tile, word for word, with owner planes,
lookups and halo rings that no mosaic would produce; the session's memory; and ProcessManager.process_depressions on one GPU
against conditioning.label_depressions of the stitched raster.  Shapes sit around the 32-cell block: one block, several, partial
ones, a three-row tile."""
import numpy as np
import pytest

import seam_fill_kit as K
import depression_mosaic_kit as D

pytestmark = pytest.mark.gpu

SIDES = ('top', 'bottom', 'left', 'right')
SHAPES = [(33, 65), (70, 45), (3, 40), (64, 64)]


def surface(shape):
    """a fractal with relief, NaN cells on and off the border, and caps low enough that lakes reach the seam lines"""
    z = K.fractal(shape[0], shape[1])
    z[shape[0] // 2, shape[1] // 3] = np.nan
    z[0, 5] = z[shape[0] - 1, shape[1] - 2] = np.nan
    return z


def device(z):
    from pydem_amd import DEMProcessor
    return DEMProcessor(elev=z, dX=30.0, dY=30.0, fill_flats=False, drain_pits_path=False)


def open_pair(z, outlets=None):
    """the same session on the device and on the twin, every side a seam line, relaxed once at epsilon 0 under caps a little above z"""
    from pydem_amd import conditioning
    n, m = z.shape
    seam = {s: np.ones(m if s in ('top', 'bottom') else n, bool) for s in SIDES}
    line = {'top': z[0], 'bottom': z[-1], 'left': z[:, 0], 'right': z[:, -1]}
    rng = np.random.RandomState(4)
    caps = {s: np.nan_to_num(np.array(line[s]), nan=np.inf) + rng.uniform(0.0, 3.0, line[s].size) for s in SIDES}
    mask = D.outlets_mask(z.shape, outlets)
    twin = conditioning.SeamFill(z, mask, seam)
    dp = device(z)
    dp.fill_seam_begin(seam, outlets)
    dp.fill_seam_relax(0.0, caps)
    twin.relax(0.0, caps)
    return dp, twin


def inventory_inputs(shape, K_local, seed):
    """a lookup that sends several local ids to one row, rows that occur in the halo only, a random owner plane, a halo ring with
    every kind of entry and levels taken from the surface, row areas that differ per row"""
    n, m = shape
    rng = np.random.RandomState(seed)
    rows_own = max(1, (K_local + 1) // 2)
    T = rows_own + 3                                # the last three rows occur in the halo only
    lut = np.zeros(K_local + 1, np.int32)
    lut[1:] = rng.randint(1, rows_own + 1, K_local)
    owner = rng.uniform(size=shape) < 0.7
    ring = 2 * m + 2 * n + 4
    halo_ids = rng.randint(-1, T + 1, ring).astype(np.int32)
    row_area = 900.0 + rng.uniform(0.0, 5.0, n)
    return lut, T, owner, halo_ids, row_area


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('local', ['1', '0'])
def test_label_and_inventory_against_the_host_twin(monkeypatch, shape, local):
    from pydem_amd import conditioning
    monkeypatch.setenv('PYDEM_DEPR_LOCAL', local)
    n, m = shape
    z = surface(shape)
    outlets = [(n // 2, m // 2), (1, 1)]
    dp, twin = open_pair(z, outlets)
    got = dp.fill_seam_label()
    roots, levels, dmax = twin.label()
    assert got['roots'].dtype == np.int32 and np.array_equal(got['roots'], roots) and np.array_equal(got['levels'], levels)
    assert got['max_depth'] == dmax and got['ms'] > 0
    assert roots.size >= 1
    req = [(0, r) for r in range(n)] + [(1, 0), (1, -1), (1, m // 2), (0, -1)]
    ids = dp.fill_seam_id_lines(req)
    for a, b in zip(ids, twin.id_lines(req)):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert np.array_equal(np.array(ids[:n]), twin.ids)
    if shape != (3, 40):
        assert (twin.ids[0] > 0).any() or (twin.ids[-1] > 0).any() or (twin.ids[:, 0] > 0).any() or (twin.ids[:, -1] > 0).any()    # a lake on a seam line
    for seed in (0, 1):
        lut, T, owner, halo_ids, row_area = inventory_inputs(shape, roots.size, seed)
        # halo levels: values of the surface, so that cells beside the ring do find their own elevation there
        rng = np.random.RandomState(seed + 10)
        halo_W = np.concatenate([z[0, [0] + list(range(m)) + [m - 1]], z[-1, [0] + list(range(m)) + [m - 1]], z[:, 0], z[:, -1]])
        halo_W = np.where(rng.uniform(size=halo_W.size) < 0.7, np.nan_to_num(halo_W, nan=0.0), rng.uniform(0.0, 100.0, halo_W.size))
        sh_a, _ = conditioning.fixed_point(n * m, row_area.max())
        sh_v, _ = conditioning.fixed_point(n * m, dmax * row_area.max())
        want = twin.inventory(lut, T, owner, halo_ids, halo_W, row_area, sh_a, sh_v)
        out = dp.fill_seam_inventory(lut, T, owner, halo_ids, halo_W, row_area, sh_a, sh_v)
        assert out['table'].dtype == np.uint64 and out['table'].shape == (len(conditioning.SEAM_TABLE_COLS), T)
        assert np.array_equal(out['table'], want) and out['ms'] > 0
        col = {nm: k for k, nm in enumerate(conditioning.SEAM_TABLE_COLS)}
        assert (want[col['cells']] > 0).any() and (want[col['n_sills']] > 0).any()
        if shape != (3, 40):
            assert (want[col['n_sills']][-3:] > 0).any()           # a row that occurs in the halo only has a sill inside the tile
        kept = np.concatenate(([0], rng.randint(0, 5, roots.size))).astype(np.int32)
        lab = dp.fill_seam_labels(kept)
        assert lab['label'].dtype == np.int32 and np.array_equal(lab['label'], twin.labels(kept))
    dp.fill_seam_end(False)
    assert np.asarray(dp.elev).tobytes() == z.tobytes()


def test_bad_lookups_and_halos_are_refused():
    from pydem_amd import _ffi
    shape = (33, 65)
    z = surface(shape)
    dp, twin = open_pair(z)
    with pytest.raises(_ffi.HipError, match='error -2'):
        dp._tile.fill_seam_id_lines([(0, 0)])       # no labels yet
    k = dp.fill_seam_label()['roots'].size
    lut, T, owner, halo_ids, row_area = inventory_inputs(shape, k, 0)
    halo_W = np.zeros(halo_ids.size)
    bad = lut.copy()
    bad[-1] = T + 1
    with pytest.raises(_ffi.HipError, match='error -2'):
        dp.fill_seam_inventory(bad, T, owner, halo_ids, halo_W, row_area, 0, 0)
    bad = halo_ids.copy()
    bad[3] = -2
    with pytest.raises(_ffi.HipError, match='error -2'):
        dp.fill_seam_inventory(lut, T, owner, bad, halo_W, row_area, 0, 0)
    with pytest.raises(ValueError, match='lookup'):
        dp.fill_seam_inventory(lut[:-1], T, owner, halo_ids, halo_W, row_area, 0, 0)
    with pytest.raises(ValueError, match='lookup'):
        dp.fill_seam_labels(lut[:-1])
    dp.fill_seam_end(False)
    fresh = device(z)
    fresh.fill_seam_begin({s: np.ones(65 if s in ('top', 'bottom') else 33, bool) for s in SIDES})
    with pytest.raises(_ffi.HipError, match='error -5'):
        fresh.fill_seam_label()                     # W still holds +inf
    fresh.fill_seam_end(False)


def test_session_memory_with_the_id_plane():
    from pydem_amd import _ffi
    n, m = 70, 45
    z = surface((n, m))
    blocks = n * m * 8 + ((n + 31) // 32) * ((m + 31) // 32) * 4 + (2 * m + 2 * n) * 8
    for commit in (False, True):
        dp = device(z)
        dp._ensure_tile()
        dp._push('elev')
        before = dp._tile.device_bytes()
        seam = {s: np.ones(m if s in ('top', 'bottom') else n, bool) for s in SIDES}
        caps = {s: np.full(m if s in ('top', 'bottom') else n, 1e6) for s in SIDES}
        dp.fill_seam_begin(seam)
        dp.fill_seam_relax(0.0, caps)
        assert dp._tile.device_bytes() == before + blocks
        k = dp.fill_seam_label()['roots'].size
        assert dp._tile.device_bytes() == before + blocks + 4 * n * m
        dp.fill_seam_label()                        # again: the same plane
        lut, T, owner, halo_ids, row_area = inventory_inputs((n, m), k, 0)
        dp.fill_seam_inventory(lut, T, owner, halo_ids, np.zeros(halo_ids.size), row_area, 0, 0)
        dp.fill_seam_labels(lut)
        dp.fill_seam_id_lines([(1, 3), (0, 2)])
        assert dp._tile.device_bytes() == before + blocks + 4 * n * m
        assert np.asarray(dp._tile.download(_ffi.ELEV)).tobytes() == z.tobytes()        # the resident elevation after the inventory
        dp.fill_seam_end(commit)
        assert dp._tile.device_bytes() == before
        assert (np.asarray(dp.elev).tobytes() == z.tobytes()) == (not commit)


# ---- mosaics on one GPU
def _mosaic(name, cut, drop=(), **kw):
    from pydem_amd import DEMProcessor
    pm = D.manager(D.field(name), *cut, drop=drop, spacing=True, processor_cls=DEMProcessor, devices=[0])
    lat = pm.fill_lattice()
    ref = D.whole(('gpu', name, cut, drop, repr(sorted(kw.items()))), pm, lat, **kw)
    pm.process_elevation()
    before = D.elevation_bytes(pm)
    for t in pm.tiles:
        t._ensure_tile()
        t._push('elev')
    bytes_before = [t._tile.device_bytes() for t in pm.tiles]
    res = pm.process_depressions(**kw)
    D.assert_equals_whole(pm, lat, res, ref)
    assert D.elevation_bytes(pm) == before
    assert [t._tile.device_bytes() for t in pm.tiles] == bytes_before
    return pm, ref


@pytest.mark.parametrize('case', [(cut, ()) for cut in D.CUTS] + [D.DROP])
@pytest.mark.parametrize('name', ['fractal', 'fractal_nan', 'designed', 'designed_nan'])
def test_mosaic_equals_the_whole_raster_inventory(name, case):
    cut, drop = case
    pm, ref = _mosaic(name, cut, drop)
    st = pm.depressions_stats
    assert st['n_found'] == len(ref[1]) and st['fill_rounds'] >= 1
    assert all(st['ms'][part] > 0 for part in ('fill', 'label', 'inventory', 'labels'))


def test_mosaic_filters_and_outlets():
    _mosaic('fractal_nan', (3, 3, 2), min_depth=1.5, min_cells=4, min_volume=1000.0)
    _mosaic('designed', (2, 2, 1), outlets=[(66, 86), (50, 131), (150, 87), (102, 131)])


def test_mosaic_abort_leaves_the_tiles_untouched():
    from pydem_amd import DEMProcessor
    pm = D.manager(D.field('designed'), 2, 3, 3, processor_cls=DEMProcessor, devices=[0])
    pm.process_elevation()
    before = D.elevation_bytes(pm)
    for t in pm.tiles:
        t._ensure_tile()
        t._push('elev')
    bytes_before = [t._tile.device_bytes() for t in pm.tiles]
    with pytest.raises(RuntimeError, match='max_rounds'):
        pm.process_depressions(max_rounds=1)
    assert D.elevation_bytes(pm) == before
    assert [t._tile.device_bytes() for t in pm.tiles] == bytes_before
