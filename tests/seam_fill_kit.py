"""Test kit of the fill across tiles (tests/test_fill_mosaic.py, tests/test_gpu_fill_mosaic.py): a CPU processor whose seam
session is the host twin (pydem_amd/conditioning.py: SeamFill), mosaics cut from one raster, the whole-raster reference and the
designed field.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle_processor import OracleProcessor

CUTS = [(2, 2, 1), (3, 3, 2), (2, 3, 3), (1, 4, 1)]        # (grid rows, grid columns, overlap)


class SeamProcessor(OracleProcessor):
    """OracleProcessor with the seam session of DEMProcessor, served by conditioning.SeamFill"""

    def __init__(self, **kw):
        OracleProcessor.__init__(self, **kw)
        self._seam = None
        self.fill_depressions_stats = None

    @property
    def shape(self):
        return self.elev.shape

    def fill_seam_begin(self, seam, outlets=None):
        from pydem_amd import conditioning
        assert self._seam is None
        mask = None
        if outlets is not None:
            mask = np.zeros(self.elev.shape, bool)
            o = np.asarray(outlets).reshape(-1, 2)
            mask[o[:, 0], o[:, 1]] = True
        self._seam = conditioning.SeamFill(self.elev, mask, seam)
        return self._seam.amax

    def fill_seam_relax(self, eps, caps=None):
        return dict(n_lowered=self._seam.relax(eps, caps), passes=0, ms=0.0)

    def fill_seam_lines(self, requests):
        return self._seam.lines(requests)

    def fill_seam_end(self, commit=True, return_depth=False):
        s = self._seam
        if commit:
            W, depth = s.end(True)
            self.elev = np.ascontiguousarray(W)
            self.fill_depressions_stats = dict(epsilon=s.eps)
        self._seam = None


def specs(raster, ny, nx, overlap, drop=()):
    """in-memory tile specs of ProcessManager for a cut of `raster` (synth.split_mosaic), without the tiles `drop`"""
    from pydem_amd import synth
    return [dict(elev=e, bounds=b) for k, (e, b) in enumerate(synth.split_mosaic(raster, ny, nx, overlap)) if k not in drop]


def manager(raster, ny, nx, overlap, drop=(), processor_cls=SeamProcessor, **kw):
    from pydem_amd import process_manager
    kw.setdefault('dem_proc_kwargs', dict(fill_flats=False, drain_pits_path=False))
    return process_manager.ProcessManager(elev_source_files=specs(raster, ny, nx, overlap, drop), processor_cls=processor_cls,
                                          elev_conditioned=True, out_path=kw.pop('out_path', '.'), **kw)


def stitched(pm, lat):
    """the raster the tiles of `pm` cover, NaN where no tile does"""
    full = np.full((int((lat[:, 0] + lat[:, 2]).max()), int((lat[:, 1] + lat[:, 3]).max())), np.nan)
    for i, meta in enumerate(pm._tile_meta):
        r0, c0, n, m = [int(v) for v in lat[i]]
        full[r0:r0 + n, c0:c0 + m] = meta['elev']
    return full


_WHOLE = {}


def whole_fill(key, full, eps, outlets=None):
    """conditioning.fill_depressions of the stitched raster, computed once per key; outlets: lattice (row, col) pairs"""
    if key not in _WHOLE:
        from pydem_amd import conditioning
        mask = None
        if outlets is not None:
            mask = np.zeros(full.shape, bool)
            o = np.asarray(outlets).reshape(-1, 2)
            mask[o[:, 0], o[:, 1]] = True
        _WHOLE[key] = conditioning.fill_depressions(full, eps, mask)[0]
        _WHOLE[key].setflags(write=False)
    return _WHOLE[key]


def assert_tiles_equal_whole(pm, lat, W):
    for i in range(pm.n_inputs):
        r0, c0, n, m = [int(v) for v in lat[i]]
        got = np.asarray(pm.tiles[i].elev, np.float64)
        assert got.tobytes() == np.ascontiguousarray(W[r0:r0 + n, c0:c0 + m]).tobytes(), "tile %d differs from the whole-raster fill" % i


def per_tile_fill_differs(pm, lat, W, eps):
    """cells in which the per-tile fill of today (every tile's border open) differs from the whole-raster fill"""
    from pydem_amd import conditioning
    bad = 0
    for i, meta in enumerate(pm._tile_meta):
        r0, c0, n, m = [int(v) for v in lat[i]]
        Wt = conditioning.fill_depressions(meta['elev'], eps)[0]
        ref = W[r0:r0 + n, c0:c0 + m]
        bad += int(np.count_nonzero(~((Wt == ref) | (np.isnan(Wt) & np.isnan(ref)))))
    return bad


def fractal(n, m, nan_patch=None):
    from pydem_amd import synth
    z = synth.fractal(n, m, seed=5)
    if nan_patch is not None:
        z[nan_patch] = np.nan
    return z


def designed(n, m):
    """A plateau at 1000 with (a) a basin (floor 500, pit 400) around (n/3, m/3), the point where four tiles of a 3 x 3 cut meet,
    whose only spill is a one-cell channel (sill 600) that runs diagonally down to the raster's last row in the bottom-right tile,
    and (b) a one-cell serpentine channel through rows 2, 4, 6 that descends AWAY from its single outlet at (2, 0) and crosses
    every vertical seam once per row: what the outlet's level means for its far end travels one seam per round.  Returns
    (z, basin mask)."""
    z = np.full((n, m), 1000.0)
    br, bc = n // 3, m // 3
    basin = np.zeros((n, m), bool)
    basin[br - 6:br + 6, bc - 6:bc + 6] = True
    z[basin] = 500.0
    z[br - 2, bc - 2] = 400.0
    r, c, k = br + 6, bc + 6, 0
    while r < n:                                    # the spill: diagonal while there is room, then straight down
        z[r, c] = 600.0 - 0.1 * k
        r, c, k = r + 1, (c + 1 if c < m - 3 else c), k + 1
    path = [(2, 0), (2, 1)]
    right = True
    for row in (2, 4, 6):
        cols = range(2, m - 2) if right else range(m - 3, 1, -1)
        path += [(row, cc) for cc in cols]
        if row < 6:
            path.append((row + 1, m - 3 if right else 2))
        right = not right
    for k, (r, c) in enumerate(path):
        z[r, c] = 900.0 - 0.01 * k
    return z, basin
