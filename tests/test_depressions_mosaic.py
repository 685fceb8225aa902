"""CPU tier: ProcessManager.process_depressions -- the join of the tiles' components, the owner and halo bookkeeping, the combined
table and its refusals -- with the host twin of the device session (conditioning.SeamFill behind tests/depression_mosaic_kit.py:
InventoryProcessor).  The table, the quanta and every tile's labels are compared with array_equal against
conditioning.label_depressions of the stitched raster, with one cell area per lattice row from the lowest-index tile that holds it."""
import numpy as np
import pytest

import seam_fill_kit as K
import depression_mosaic_kit as D

CASES = [(cut, ()) for cut in D.CUTS] + [D.DROP]


def _run(name, cut, drop=(), outlets=None, spacing=True, **filters):
    pm = D.manager(D.field(name), *cut, drop=drop, spacing=spacing)
    lat = pm.fill_lattice()
    ref = D.whole((name, cut, drop, spacing, repr(outlets), repr(sorted(filters.items()))), pm, lat, outlets, **filters)
    pm.process_elevation()
    before = D.elevation_bytes(pm)
    res = pm.process_depressions(outlets=outlets, **filters)
    assert res is pm.depressions
    D.assert_equals_whole(pm, lat, res, ref)
    assert D.elevation_bytes(pm) == before and all(t._seam is None for t in pm.tiles)      # nothing committed, every session closed
    return pm, lat, res, ref


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('name', ['fractal', 'fractal_nan', 'designed', 'designed_nan'])
def test_table_quanta_and_labels_equal_the_whole_mosaic_inventory(name, case):
    cut, drop = case
    pm, lat, res, ref = _run(name, cut, drop)
    st = pm.depressions_stats
    assert st['n_found'] == len(ref[1]) > 0 and st['fill_rounds'] >= 1
    assert sorted(st['ms']) == ['fill', 'inventory', 'label', 'labels']
    if name == 'fractal':
        assert len(ref[1]) > 100 and (ref[1]['open_sill'] == 1).any() and (ref[1]['open_sill'] == 0).any()


@pytest.mark.parametrize('cut', D.CUTS)
def test_spacing_from_the_bounds(cut):
    pm, lat, res, ref = _run('fractal', cut, spacing=False)
    ra = D.row_area(pm, lat)
    assert (ra > 0).all() and np.allclose(ra, ra[0], rtol=1e-9)     # the pixel size of the bounds, up to the rounding of each tile's own


def test_row_area_comes_from_the_lowest_index_tile():
    pm = D.manager(D.field('designed'), 2, 2, 1, spacing=True)
    lat = pm.fill_lattice()
    ra = D.row_area(pm, lat)
    s0, s1, s2 = pm._spacing(0), pm._spacing(1), pm._spacing(2)
    assert ra[5] == s0['dX2'][5] * s0['dY2'][5] != s1['dX2'][5] * s1['dY2'][5]          # tiles 0 and 1 hold row 5 with different spacing
    assert ra[102] == s0['dX2'][102] * s0['dY2'][102] != s2['dX2'][0] * s2['dY2'][0]    # the shared row is tile 0's
    assert np.unique(ra).size == ra.size


def test_the_designed_cases_are_in_the_field():
    """what the designed field is for, read from the reference table of the (2, 2, 1) and (2, 3, 3) cuts"""
    pm, lat, res, ref = _run('designed', (2, 2, 1))
    label, table, _ = ref
    assert len(table) == 7
    by_first = {(int(t['r0']), int(t['c0'])): t for t in table}
    corner = table[label[D.CORNER_LAKE][0, 0] - 1]
    assert (corner['pour_row'], corner['pour_col'], corner['n_sills'], corner['cells']) == D.CORNER_SILL + (1, 25)
    assert tuple(lat[:, :2][3]) == D.CORNER_SILL and all(lat[i, 0] + lat[i, 2] > 102 and lat[i, 1] + lat[i, 3] > 131 for i in range(4))
    twin = table[label[50, 125] - 1]
    assert twin['n_sills'] == 2 and (twin['pour_row'], twin['pour_col']) == D.TWIN_SILLS[0] and twin['spill_elev'] == 940.0
    assert (twin['bottom_row'], twin['bottom_col']) == (50, 125) and D.TWIN_SILLS[0][1] < 131 < D.TWIN_SILLS[1][1]
    # the U-shaped lake is two components in tile 0 and one in tile 1
    from pydem_amd import conditioning
    from scipy import ndimage
    u = label == label[D.U_LAKE_FIRST]
    parts = [ndimage.label(u[r0:r0 + n, c0:c0 + m], structure=np.ones((3, 3)))[1] for r0, c0, n, m in lat[:2].tolist()]
    assert parts == [2, 1] and by_first[D.U_LAKE_FIRST]['cells'] == 37
    # the pit inside the overlap of width 3 is labelled by both tiles and counted once
    pm3 = D.manager(D.field('designed'), 2, 3, 3)
    lat3 = pm3.fill_lattice()
    r, c = D.OVERLAP_PIT
    holders = [i for i in range(6) if lat3[i, 0] < r < lat3[i, 0] + lat3[i, 2] - 1 and lat3[i, 1] < c < lat3[i, 1] + lat3[i, 3] - 1]
    assert holders == [3, 4]
    pit = table[label[D.OVERLAP_PIT] - 1]
    assert pit['cells'] == 1 and pit['n_sills'] == 8


def test_per_tile_inventories_are_wrong_on_the_designed_field():
    from pydem_amd import conditioning
    pm, lat, res, ref = _run('designed', (2, 3, 3))
    label, table, _ = ref
    basin = table[label[67, 87] - 1]                # the basin: a seam of three columns runs through it
    pieces, found = [], 0
    for i, meta in enumerate(pm._tile_meta):
        r0, c0, n, m = [int(v) for v in lat[i]]
        lab_i, tab_i, _ = conditioning.label_depressions(meta['elev'])
        found += len(tab_i)
        here = np.unique(lab_i[(label[r0:r0 + n, c0:c0 + m] == label[67, 87]) & (lab_i > 0)])
        pieces += [tab_i[k - 1] for k in here]
    assert found != pm.depressions_stats['n_found']
    # cut open, the basin's floor drains off each tile: only the pit below the floor is left of a lake 200 deep
    assert len(pieces) >= 1 and basin['max_depth'] == 200.0 and basin['cells'] == 144
    assert all(p['max_depth'] < basin['max_depth'] and p['cells'] < basin['cells'] for p in pieces)


def test_open_sill_beside_no_data_and_beside_a_missing_tile():
    pm, lat, res, ref = _run('designed_nan', (2, 2, 1))
    label, table, _ = ref
    lake = table[label[D.NAN_LAKE][0, 0] - 1]
    assert lake['open_sill'] == 1 and (lake['pour_row'], lake['pour_col']) == D.NAN_SILL
    pm, lat, res, ref = _run('designed', *D.DROP)
    label, table, _ = ref
    assert np.isnan(K.stitched(pm, lat)).any()
    lake = table[label[D.DROP_LAKE][0, 0] - 1]      # spills into the cells no tile holds
    assert lake['open_sill'] == 1 and lake['spill_elev'] == 950.0 and (lake['pour_row'], lake['pour_col']) == D.DROP_SILL
    pm9 = D.manager(D.field('designed'), 3, 3, 2)
    whole = D.whole(('designed', (3, 3, 2), 'whole'), pm9, pm9.fill_lattice())
    lake = whole[1][whole[0][D.DROP_LAKE][0, 0] - 1]
    assert lake['open_sill'] == 0 and lake['spill_elev'] == 1000.0


@pytest.mark.parametrize('case', [((3, 3, 2), ()), ((2, 3, 3), ()), D.DROP])
def test_filters_renumber_in_the_same_order(case):
    cut, drop = case
    pm, lat, res, ref = _run('fractal_nan', cut, drop, min_depth=1.5, min_cells=4, min_volume=1000.0)
    full = D.whole(('fractal_nan', cut, drop, 'all'), pm, lat)
    assert 0 < len(ref[1]) < len(full[1]) == pm.depressions_stats['n_found']
    assert (res['table']['max_depth'] >= 1.5).all() and (res['table']['cells'] >= 4).all() and (res['table']['volume'] >= 1000.0).all()


def test_without_labels():
    pm = D.manager(D.field('fractal'), 2, 3, 3, spacing=True)
    lat = pm.fill_lattice()
    res = pm.process_depressions(return_labels=False)
    assert res['labels'] is None and np.array_equal(res['table'], D.whole(('fractal', (2, 3, 3), 'nolabels'), pm, lat)[1])


@pytest.mark.parametrize('cut', [(2, 2, 1), (3, 3, 2)])
def test_outlets_in_lattice_coordinates(cut):
    outlets = [(66, 86), (50, 131), (150, 87), (102, 131)]      # the basin floor, the twin lake on the shared column, the pit, a sill
    pm, lat, res, ref = _run('designed', cut, outlets=outlets)
    label, table, _ = ref
    assert label[50, 131] == 0 and label[150, 87] == 0          # an outlet is not raised
    plain = D.whole(('designed', cut, 'plain'), pm, lat)
    assert len(table) != len(plain[1])
    corner = table[label[D.CORNER_LAKE][0, 0] - 1]
    assert corner['open_sill'] == 1                             # its sill is an outlet now


def test_refusals_come_before_any_tile_is_touched():
    from pydem_amd import process_manager
    raster = D.field('fractal')
    pm = D.manager(raster, 2, 2, 0)
    with pytest.raises(NotImplementedError, match='overlap'):
        pm.process_depressions()
    assert all(t is None for t in pm.tiles)
    sp = D.specs(raster, 2, 2, 1)
    l, b, r, t = sp[3]['bounds']
    sp[3]['bounds'] = (l, b, l + 2 * (r - l), t)
    pm = process_manager.ProcessManager(elev_source_files=sp, processor_cls=D.InventoryProcessor, elev_conditioned=True, out_path='.')
    with pytest.raises(NotImplementedError, match='pixel size'):
        pm.process_depressions()
    assert all(t is None for t in pm.tiles)
    sp = D.specs(raster, 2, 2, 1)
    l, b, r, t = sp[1]['bounds']
    w = (r - l) / sp[1]['elev'].shape[1]
    sp[1]['bounds'] = (l + 0.3 * w, b, r + 0.3 * w, t)
    pm = process_manager.ProcessManager(elev_source_files=sp, processor_cls=D.InventoryProcessor, elev_conditioned=True, out_path='.')
    with pytest.raises(NotImplementedError, match='lattice'):
        pm.process_depressions()
    assert all(t is None for t in pm.tiles)
    pm = D.manager(raster, 2, 2, 1)
    with pytest.raises(ValueError, match='min_depth'):
        pm.process_depressions(min_depth=-1.0)
    assert all(t is None for t in pm.tiles)


def test_max_rounds_aborts_with_every_tile_untouched():
    pm = D.manager(D.field('designed'), 3, 3, 2)
    pm.process_elevation()
    before = D.elevation_bytes(pm)
    with pytest.raises(RuntimeError, match='max_rounds'):
        pm.process_depressions(max_rounds=1)
    assert D.elevation_bytes(pm) == before and all(t._seam is None for t in pm.tiles)
    assert pm.depressions is None
    lat = pm.fill_lattice()
    D.assert_equals_whole(pm, lat, pm.process_depressions(), D.whole(('designed', (3, 3, 2), 'after abort'), pm, lat))     # a later run is not disturbed


def test_an_error_in_the_inventory_closes_every_session(monkeypatch):
    pm = D.manager(D.field('fractal'), 2, 2, 1)
    pm.process_elevation()
    before = D.elevation_bytes(pm)

    def broken(self, *a):
        raise RuntimeError("no table today")
    monkeypatch.setattr(D.InventoryProcessor, 'fill_seam_inventory', broken)
    with pytest.raises(RuntimeError, match='no table today'):
        pm.process_depressions()
    assert D.elevation_bytes(pm) == before and all(t._seam is None for t in pm.tiles)


def test_the_fill_still_commits_after_the_inventory():
    """the loop that both callers share: an inventory, then the fill of the same manager"""
    raster = D.field('designed')
    pm = D.manager(raster, 2, 3, 3)
    lat = pm.fill_lattice()
    pm.process_depressions()
    pm.process_fill_depressions(0.0)
    K.assert_tiles_equal_whole(pm, lat, K.whole_fill(('dm_designed', 0.0), K.stitched(pm, lat), 0.0))
    res = pm.process_depressions()                  # the filled mosaic has no depression left
    assert len(res['table']) == 0 and pm.depressions_stats['n_found'] == 0
    assert all((lab == 0).all() for lab in res['labels'])


def test_host_twin_calls_need_their_order():
    from pydem_amd import conditioning
    z = K.fractal(20, 30)
    s = conditioning.SeamFill(z, None, dict(left=np.ones(20, bool)))
    with pytest.raises(RuntimeError, match='inf'):
        s.label()                                   # nothing has relaxed yet
    s.relax(0.0, dict(left=np.full(20, 500.0)))
    with pytest.raises(RuntimeError, match='label first'):
        s.id_lines([(0, 0)])
    roots, levels, dmax = s.label()
    assert roots.dtype == np.int32 and (np.diff(roots) > 0).all() and np.array_equal(levels, s.W.ravel()[roots])
    with pytest.raises(ValueError, match='lookup'):
        s.inventory(np.zeros(roots.size), 1, np.ones(z.shape, bool), np.zeros(104), np.zeros(104), np.ones(20), 0, 0)
