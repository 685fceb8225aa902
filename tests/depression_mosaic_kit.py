"""Test kit of the depression inventory across tiles (tests/test_depressions_mosaic.py, tests/test_gpu_depressions_mosaic.py): a CPU
processor whose inventory calls are the host twin (pydem_amd/conditioning.py: SeamFill.label / id_lines / inventory / labels), the
designed field, mosaics with explicit per-tile spacing, and the whole-raster reference.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import seam_fill_kit as K

RASTER = (203, 261)                                 # tile edges of every cut are no multiple of 32
CUTS = K.CUTS
DROP = ((3, 3, 2), (4,))                            # the cut with a dropped tile: the centre of the 3 x 3
NAN_PATCH = (slice(160, 170), slice(40, 50))

# cells of the designed field that the tests name (lattice row, col)
CORNER_SILL = (102, 131)                            # the cell the four tiles of the (2, 2, 1) cut share
CORNER_LAKE = (slice(97, 102), slice(126, 131))
TWIN_SILLS = ((49, 124), (49, 139))
TWIN_LAKE = (50, slice(125, 139))
OVERLAP_PIT = (150, 87)
U_LAKE_FIRST = (80, 120)
NAN_LAKE = (slice(160, 166), slice(30, 39))
NAN_SILL = (162, 39)
DROP_LAKE = (slice(136, 140), slice(100, 105))
DROP_SILL = (135, 102)                              # the first row below the cells that only the centre tile of the (3, 3, 2) cut holds


class InventoryProcessor(K.SeamProcessor):
    """SeamProcessor with the inventory calls of DEMProcessor's seam session, served by conditioning.SeamFill"""

    def fill_seam_label(self):
        roots, levels, dmax = self._seam.label()
        return dict(roots=roots, levels=levels, max_depth=dmax, ms=0.0)

    def fill_seam_id_lines(self, requests):
        return self._seam.id_lines(requests)

    def fill_seam_inventory(self, lut, n_rows, owner, halo_ids, halo_W, row_area, shift_area, shift_volume):
        return dict(table=self._seam.inventory(lut, n_rows, owner, halo_ids, halo_W, row_area, shift_area, shift_volume), ms=0.0)

    def fill_seam_labels(self, lut):
        return dict(label=self._seam.labels(lut), ms=0.0)


def designed(n=RASTER[0], m=RASTER[1], nan_patch=False):
    """seam_fill_kit.designed -- (a) the basin over the point where the four tiles of the (3, 3, 2) cut meet, its diagonal spill
    channel and the serpentine through rows 2, 4, 6 -- and on the same plateau at 1000:
      (b) a one-cell pit at OVERLAP_PIT: in the (2, 3, 3) cut the middle column of an overlap of width 3, interior to both tiles;
      (c) a U-shaped lake at 950, arms along rows 80 and 84 from column 120, joined by a bar in column 136 only: in the (2, 2, 1) cut
          the left tile (columns .. 131) sees two components, the right tile joins them;
      (d) a 5 x 5 lake at 900 whose only sill (950) is CORNER_SILL, the cell all four tiles of the (2, 2, 1) cut share; the lake lies
          in the top-left tile alone, and the spill runs down column 132 into the diagonal channel;
      (e, f) a lake along row 50 across column 131, all of it at 900 (its lowest z occurs in two tiles), with two sill cells at 940,
          TWIN_SILLS, diagonally off its two ends, left of column 131 and right of it; each spills up its column into the serpentine;
      (g) with nan_patch: NAN_PATCH is no data, and a lake at 900 west of it spills through NAN_SILL (950) into it; a lake at 900 in
          rows 136 .. 139 with DROP_SILL (950) above it: the (3, 3, 2) cut without its centre tile leaves that cell beside cells that
          no tile holds and the lake spills there, while in a whole mosaic the lake rises to the plateau."""
    assert (n, m) == RASTER
    z = K.designed(n, m)[0]
    z[OVERLAP_PIT] = 990.0
    z[80, 120:137] = z[84, 120:137] = z[80:85, 136] = 950.0
    z[CORNER_LAKE] = 900.0
    z[CORNER_SILL] = 950.0
    for k, r in enumerate(range(103, 112)):
        z[r, 132] = 940.0 - 0.1 * k
    z[TWIN_LAKE] = 900.0
    for r, c in TWIN_SILLS:
        for k, rr in enumerate(range(r, 6, -1)):
            z[rr, c] = 940.0 - 0.1 * k
    z[DROP_LAKE] = 900.0
    z[DROP_SILL] = 950.0
    if nan_patch:
        z[NAN_LAKE] = 900.0
        z[NAN_SILL] = 950.0
        z[NAN_PATCH] = np.nan
    return z


_FIELDS = {}


def field(name):
    """'fractal', 'fractal_nan', 'designed', 'designed_nan': computed once, read-only"""
    if name not in _FIELDS:
        nan = name.endswith('_nan')
        _FIELDS[name] = designed(nan_patch=nan) if name.startswith('designed') else K.fractal(RASTER[0], RASTER[1], NAN_PATCH if nan else None)
        _FIELDS[name].setflags(write=False)
    return _FIELDS[name]


def specs(raster, ny, nx, overlap, drop=(), spacing=False):
    """seam_fill_kit.specs; with `spacing` every tile carries its own dX2 / dY2, different per row and per tile, so that the
    lowest-index tile of a lattice row decides its cell area"""
    out = []
    for k, sp in enumerate(K.specs(raster, ny, nx, overlap)):
        if spacing:
            n = sp['elev'].shape[0]
            sp.update(dX=np.full(n - 1, 30.0), dY=np.full(n - 1, 28.0), dX2=30.0 + 0.01 * np.arange(n) + 0.5 * k,
                      dY2=28.0 - 0.003 * np.arange(n) + 0.25 * k)
        if k not in drop:
            out.append(sp)
    return out


def manager(raster, ny, nx, overlap, drop=(), spacing=False, processor_cls=InventoryProcessor, **kw):
    from pydem_amd import process_manager
    kw.setdefault('dem_proc_kwargs', dict(fill_flats=False, drain_pits_path=False))
    return process_manager.ProcessManager(elev_source_files=specs(raster, ny, nx, overlap, drop, spacing), processor_cls=processor_cls,
                                          elev_conditioned=True, out_path=kw.pop('out_path', '.'), **kw)


def row_area(pm, lat):
    """one cell area per lattice row: dX2 * dY2 of the lowest-index tile that holds the row, from the tile specs"""
    out = np.zeros(int((lat[:, 0] + lat[:, 2]).max()))
    for i in reversed(range(pm.n_inputs)):
        sp = pm._spacing(i)
        out[lat[i, 0]:lat[i, 0] + lat[i, 2]] = sp['dX2'] * sp['dY2']
    return out


def outlets_mask(shape, outlets):
    if outlets is None:
        return None
    mask = np.zeros(shape, bool)
    o = np.asarray(outlets).reshape(-1, 2)
    mask[o[:, 0], o[:, 1]] = True
    return mask


_WHOLE = {}


def whole(key, pm, lat, outlets=None, **filters):
    """(label, table, quanta) of conditioning.label_depressions of the stitched raster, computed once per key and left unchanged"""
    if key not in _WHOLE:
        from pydem_amd import conditioning
        full = K.stitched(pm, lat)
        label, table, quanta = conditioning.label_depressions(full, outlets_mask(full.shape, outlets), dX2dY2=row_area(pm, lat), **filters)
        label.setflags(write=False)
        table.setflags(write=False)
        _WHOLE[key] = (label, table, quanta)
    return _WHOLE[key]


def assert_equals_whole(pm, lat, res, ref):
    label, table, quanta = ref
    assert res['table'].dtype == table.dtype and np.array_equal(res['table'], table)
    assert pm.depressions_stats['quanta'] == quanta
    for i in range(pm.n_inputs):
        r0, c0, n, m = [int(v) for v in lat[i]]
        got = res['labels'][i]
        assert got.dtype == np.int32 and np.array_equal(got, label[r0:r0 + n, c0:c0 + m]), "labels of tile %d" % i


def elevation_bytes(pm):
    return [np.asarray(t.elev).tobytes() for t in pm.tiles]
