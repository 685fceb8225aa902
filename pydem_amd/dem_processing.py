"""Drop-in `DEMProcessor` for the per-tile hot path, backed by the HIP library.

Mirrors the public surface of the reference class (creare-com/pydem v1.2.1,
pydem/dem_processing.py:98-258): same option names and defaults (:105-154), same constructor
normalisation of scalar `dX`/`dY` (:229-242), same methods and result attributes
(`mag, direction, flats, uca, twi, edge_todo, edge_done, section, proportion, twi_min_area`)
and the same quirks (`calc_twi()` returns the un-scaled value while `self.twi` is x10, :1674-1677).
The reference declares its options with traitlets; that package is not a dependency here, the
options are plain attributes.

All arithmetic runs on the GPU through the C-ABI (include/pydem_hip.h); arrays are uploaded once,
stay resident, and are downloaded lazily the first time the corresponding attribute is read.
"""
import logging
import warnings

import numpy as np

from . import _ffi

logger = logging.getLogger(__name__)

FLAT_ID = np.nan
FLAT_ID_INT = -1

_FIELD_OF = {'elev': _ffi.ELEV, 'mag': _ffi.MAG, 'direction': _ffi.DIRECTION, 'flats': _ffi.FLATS,
             'section': _ffi.SECTION, 'proportion': _ffi.PROPORTION, 'uca': _ffi.UCA,
             'edge_todo': _ffi.EDGE_TODO, 'edge_done': _ffi.EDGE_DONE, 'uca_weighted': _ffi.UCA_WEIGHTED}
_BOOL_FIELDS = ('flats', 'edge_todo', 'edge_done')


class _Resident(object):
    """Attribute whose value lives on the device until somebody reads it."""

    def __init__(self, name):
        self.name = name

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        if self.name not in obj._host and self.name in obj._on_device:
            arr = obj._tile.download(_FIELD_OF[self.name])
            if self.name in _BOOL_FIELDS:
                arr = arr.astype(bool)
            obj._host[self.name] = arr
        return obj._host.get(self.name)

    def __set__(self, obj, value):
        obj._on_device.discard(self.name)
        if value is None:
            obj._host.pop(self.name, None)
        else:
            if np.ma.isMaskedArray(value):
                # masked cells are no-data: NaN, like the reference's np.ma.filled(elev.astype(float64), nan) (:213-214)
                value = np.ma.filled(value.astype(np.float64), np.nan)
            obj._host[self.name] = np.asarray(value)


class DEMProcessor(object):
    """Slope magnitude, D-infinity direction, upstream contributing area and TWI of one DEM tile."""

    # ---- options: names and defaults of the reference (dem_processing.py:105-154) ----
    fill_flats = True
    fill_flats_below_sea = False
    fill_flats_source_tol = 1
    fill_flats_peaks = True
    fill_flats_pits = True
    fill_flats_max_iter = 10

    drain_pits = True
    drain_pits_path = True
    drain_pits_min_border = False
    drain_pits_spill = False
    drain_flats = False
    drain_pits_max_iter = 300
    drain_pits_max_dist = 32
    drain_pits_max_dist_XY = None

    fill_depressions = False             # run_slopes_directions fills the depressions too (calc_fill_depressions; no counterpart in the reference)
    fill_depressions_epsilon = None      # ... with this epsilon (None: automatic)

    apply_uca_limit_edges = False
    apply_twi_limits = False
    apply_twi_limits_on_uca = False

    plotflag = False
    _elev_dtype_after = None
    uca_saturation_limit = 32.0
    twi_min_slope = 1e-3
    twi_min_area = np.inf
    circular_ref_maxcount = 50
    maximum_pit_area = 32.0

    # facet geometry, identical to the reference tables (:173-193)
    facets = [
        [(0, 0), (0, 1), (-1, 1)],
        [(0, 0), (-1, 0), (-1, 1)],
        [(0, 0), (-1, 0), (-1, -1)],
        [(0, 0), (0, -1), (-1, -1)],
        [(0, 0), (0, -1), (1, -1)],
        [(0, 0), (1, 0), (1, -1)],
        [(0, 0), (1, 0), (1, 1)],
        [(0, 0), (0, 1), (1, 1)],
    ]
    ang_adj = np.array([[0, 1], [1, -1], [1, 1], [2, -1], [2, 1], [3, -1], [3, 1], [4, -1]])

    _OPTION_NAMES = ('fill_flats', 'fill_flats_below_sea', 'fill_flats_source_tol', 'fill_flats_peaks',
                     'fill_flats_pits', 'fill_flats_max_iter', 'drain_pits', 'drain_pits_path',
                     'drain_pits_min_border', 'drain_pits_spill', 'drain_flats', 'drain_pits_max_iter',
                     'drain_pits_max_dist', 'drain_pits_max_dist_XY', 'apply_uca_limit_edges',
                     'apply_twi_limits', 'apply_twi_limits_on_uca', 'plotflag', 'uca_saturation_limit',
                     'twi_min_slope', 'twi_min_area', 'circular_ref_maxcount', 'maximum_pit_area',
                     'bounds', 'transform', 'done', 'fill_depressions', 'fill_depressions_epsilon')

    elev = _Resident('elev')
    mag = _Resident('mag')
    direction = _Resident('direction')
    flats = _Resident('flats')
    section = _Resident('section')
    proportion = _Resident('proportion')
    uca = _Resident('uca')
    edge_todo = _Resident('edge_todo')
    edge_done = _Resident('edge_done')
    uca_weighted = _Resident('uca_weighted')      # last calc_weighted_uca / run_weighted_uca (no counterpart in the reference)

    @property
    def twi(self):
        """10 x ln(uca / (mag + min_slope)) (the reference stores the scaled value, :1674); downloaded lazily."""
        if self._twi10 is None and self._twi_on_device:
            self._twi10 = self._tile.download(_ffi.TWI) * 10
        return self._twi10

    @twi.setter
    def twi(self, value):
        self._twi10 = None if value is None else np.asarray(value)
        self._twi_on_device = False

    def __init__(self, elev_fn=None, device=0, **kwargs):
        if elev_fn:
            # reference :229-232: the raster's array, spacing, bounds and transform, overridden by explicit keywords
            from .raster import dem_processor_from_raster_kwargs
            kwds = dem_processor_from_raster_kwargs(elev_fn)
            kwds.update(kwargs)
            kwargs = kwds
        self._shape = None
        if kwargs.get('elev') is None:
            if kwargs.get('shape') is None:
                raise ValueError("DEMProcessor needs an elevation array (elev=...)")
            self._shape = tuple(int(v) for v in kwargs.pop('shape'))     # elevation will be produced on the device
            kwargs.pop('elev', None)
            n_rows = self._shape[0]
        else:
            n_rows = np.shape(kwargs['elev'])[0]
        # scalar / missing spacing -> per-row arrays (reference :233-240, defaults :244-258)
        if not isinstance(kwargs.get('dX'), np.ndarray):
            if 'dX2' not in kwargs:
                kwargs['dX2'] = np.ones(n_rows) * kwargs.get('dX', 1)
            kwargs['dX'] = np.ones(n_rows - 1) * kwargs.get('dX', 1)
        if not isinstance(kwargs.get('dY'), np.ndarray):
            if 'dY2' not in kwargs:
                kwargs['dY2'] = np.ones(n_rows) * kwargs.get('dY', 1)
            kwargs['dY'] = np.ones(n_rows - 1) * kwargs.get('dY', 1)
        self._host = {}
        self._on_device = set()
        self._uploaded = set()
        self._tile = None
        self._device = device
        self._twi10 = None
        self._twi_on_device = False
        self.A = None
        self.bounds = []
        self.transform = []
        self.done = None
        self.dX = np.array(kwargs.pop('dX'), dtype='float64')
        self.dY = np.array(kwargs.pop('dY'), dtype='float64')
        self.dX2 = np.array(kwargs.pop('dX2', np.ones(n_rows)), dtype='float64')
        self.dY2 = np.array(kwargs.pop('dY2', np.ones(n_rows)), dtype='float64')
        for nm in ('dX', 'dY'):
            d = getattr(self, nm)
            if not (np.isfinite(d).all() and (d > 0).all()):
                # (the reference runs on with negative / zero cell sizes and returns mirrored / infinite slopes; the device
                # kernels compare slopes by cross-multiplication with the spacings and refuse such input instead)
                raise ValueError("%s must be finite and > 0 (pass cell sizes, not signed geotransform steps)" % nm)
        area = self.dX2 * self.dY2
        if not (np.isfinite(area).all() and (area > 0).all()):
            raise ValueError("dX2 * dY2 (the cell areas) must be finite and > 0")   # the sweep keeps a flag in the sign of a share
        for k, v in kwargs.items():
            if k in _FIELD_OF:
                setattr(self, k, v)
            elif k == 'twi':
                self.twi = v
            elif k in self._OPTION_NAMES:
                setattr(self, k, v)
            elif k in ('bounds', 'transform'):
                setattr(self, k, list(v))              # tl.List() traits of the reference (:201-202)
            # unknown keywords are dropped, as traitlets' HasTraits.__init__ does

    # ------------------------------------------------------------------ device plumbing
    def _ensure_tile(self):
        if self._tile is None:
            n, m = self._shape if self._shape is not None else self.elev.shape
            self._tile = _ffi.Tile(n, m, self._device)
        # the reference lets callers overwrite dX/dY after construction (process_manager.py:59-63): re-send them
        # whenever one of the four attributes was rebound (an edge round calls this ~100 times per tile)
        cur = (self.dX, self.dY, self.dX2, self.dY2)
        last = getattr(self, '_spacing_sent', None)
        if last is None or any(a is not b for a, b in zip(cur, last)):
            self._tile.set_spacing(*cur)
            self._spacing_sent = cur
        return self._tile

    def _push(self, *names):
        """Upload host-side fields that the device does not hold yet."""
        tile = self._tile
        for nm in names:
            if nm in self._on_device:
                continue
            arr = self._host.get(nm)
            if arr is None:
                raise RuntimeError("field %r is required but has not been set or computed" % nm)
            tile.upload(_FIELD_OF[nm], arr)
            self._on_device.add(nm)

    def _produced(self, *names):
        for nm in names:
            self._host.pop(nm, None)
            self._on_device.add(nm)

    def _options(self):
        o = _ffi.Options()
        o.drain_pits = int(bool(self.drain_pits))
        o.drain_pits_min_border = int(bool(self.drain_pits_min_border))
        o.drain_pits_max_iter = int(self.drain_pits_max_iter)
        o.drain_pits_max_dist = int(self.drain_pits_max_dist or 0)
        o.drain_pits_max_dist_XY = float(self.drain_pits_max_dist_XY) if self.drain_pits_max_dist_XY else float('nan')
        o.apply_uca_limit_edges = int(bool(self.apply_uca_limit_edges))
        o.apply_twi_limits = int(bool(self.apply_twi_limits))
        o.apply_twi_limits_on_uca = int(bool(self.apply_twi_limits_on_uca))
        o.circular_ref_maxcount = int(self.circular_ref_maxcount)
        o.uca_saturation_limit = float(self.uca_saturation_limit)
        o.twi_min_slope = float(self.twi_min_slope)
        o.twi_min_area = float(self.twi_min_area)
        return o

    def _has(self, name):
        return name in self._on_device or self._host.get(name) is not None

    # one row (axis 0) / column (axis 1) of a field without moving the whole array off the device
    def get_line(self, name, axis, index):
        if name in self._on_device and name not in self._host:
            arr = self._tile.get_line(_FIELD_OF[name], axis, index)
            return arr.astype(bool) if name in _BOOL_FIELDS else arr
        a = self._host[name]
        return np.array(a[index, :] if axis == 0 else a[:, index])

    def get_lines(self, requests):
        """[(name, axis, index)] -> list of 1-D arrays; device-resident fields are fetched with one synchronisation."""
        dev = [k for k, (name, _, _) in enumerate(requests) if name in self._on_device and name not in self._host]
        out = [None] * len(requests)
        if len(dev) > 1:
            got = self._tile.get_lines([(_FIELD_OF[requests[k][0]], requests[k][1], requests[k][2]) for k in dev])
            for k, arr in zip(dev, got):
                out[k] = arr.astype(bool) if requests[k][0] in _BOOL_FIELDS else arr
        for k, (name, axis, index) in enumerate(requests):
            if out[k] is None:
                out[k] = self.get_line(name, axis, index)
        return out

    def set_line(self, name, axis, index, values):
        if name in self._on_device:
            self._tile.set_line(_FIELD_OF[name], axis, index, values)
            self._host.pop(name, None)
        else:
            a = self._host[name]
            if axis == 0:
                a[index, :] = values
            else:
                a[:, index] = values

    @property
    def timings(self):
        return self._tile.timings() if self._tile is not None else {}

    @classmethod
    def from_synthetic(cls, shape, synth, device=0, **kwargs):
        """Tile whose elevation is generated on the device by the deterministic fractal generator
        (pydem_amd/synth.py:fractal parameters) -- bench / test input, never leaves HBM."""
        dp = cls(shape=shape, device=device, **kwargs)
        dp._ensure_tile()
        dp._tile.synth_fractal(**synth)
        dp._on_device.add('elev')
        return dp

    @property
    def shape(self):
        # never a reason to bring the elevation back from the device (a 8192^2 float64 surface is 512 MB over PCIe)
        if self._shape is not None:
            return self._shape
        h = self._host.get('elev')
        if h is not None:
            return tuple(np.shape(h))
        if self._tile is not None:
            return tuple(self._tile.shape)
        return self.elev.shape

    # ------------------------------------------------------------------ reference API
    def find_flats(self):
        """flats = (mag == -1)  (reference :305-306)"""
        self._ensure_tile()
        self._push('mag')
        self._tile.find_flats()
        self._produced('flats')

    # ---- elevation conditioning: artefacts, flats and pit drain paths on the device (csrc/cond_device.hip, csrc/cond_paths.hip),
    # tiles with no-data cells included; masked arrays / exotic dtypes go through the host implementation (pydem_amd/conditioning.py)
    def _condition_on_device(self, artefacts_only):
        """True when the resident elevation was conditioned by the library (False: the caller falls back to the host)."""
        elev = self._host.get('elev')
        if elev is not None and (np.ma.isMaskedArray(elev) or np.asarray(elev).dtype.kind not in 'iuf' or np.asarray(elev).ndim != 2):
            return False
        if min(self.shape) < 3:
            return False
        self._ensure_tile()
        self._push('elev')
        ok = self._tile.fill_flats(self.maximum_pit_area if (self.maximum_pit_area or artefacts_only) else 0.0, self.fill_flats_below_sea,
                                   self.fill_flats_source_tol, self.fill_flats_peaks, self.fill_flats_pits, artefacts_only)
        if not ok:
            return False
        dtype = None if elev is None else np.asarray(elev).dtype
        self._produced('elev')
        for nm in ('mag', 'direction', 'flats', 'uca', 'section', 'proportion', 'edge_todo', 'edge_done'):
            self._on_device.discard(nm)             # the conditioning used those planes as scratch
        self._elev_dtype_after = dtype if artefacts_only else None
        return True

    def calc_fill_pit_artifacts(self):
        """Fill quantisation pits (reference :396-426)."""
        if self._condition_on_device(artefacts_only=True):
            if self._elev_dtype_after is not None and self._elev_dtype_after != np.float64:
                self.elev = self.elev.astype(self._elev_dtype_after)          # the step keeps the array's dtype
            return
        from . import conditioning
        self.elev = conditioning.fill_pit_artifacts(self.elev, self.maximum_pit_area, self.fill_flats_below_sea)

    def calc_fill_flats(self):
        """Fill / interpolate flats before the slope stencil (reference :551-579)."""
        if self._condition_on_device(artefacts_only=False):
            return
        from . import conditioning
        self.elev = conditioning.fill_flats(self.elev, self.maximum_pit_area, self.fill_flats_below_sea,
                                            self.fill_flats_source_tol, self.fill_flats_peaks, self.fill_flats_pits)

    def calc_pit_drain_paths(self):
        """Carve monotone paths from pits to their outlets (reference :428-548).  Works on a copy of the
        array (the reference edits the caller's array in place).  Returns the drained surface like the reference;
        `run_pit_drain_paths` is the same step without bringing it back to the host."""
        self.run_pit_drain_paths()
        return self.elev

    def run_pit_drain_paths(self):
        res = self._pit_paths_on_device()
        if res is None and self._tile is not None and 'elev' in self._on_device:
            warnings.warn("calc_pit_drain_paths: the device schedule handed this tile to the sequential host loop "
                          "(a conflict of the speculative rounds): same result, much slower")
        if res is not None:
            n_failed, used, self._pit_path_rounds = res
            if n_failed:
                warnings.warn("Warning %d pits had no place to drain to in this chunk" % n_failed)
            logger.info("... done draining pits with maxiter = %d", used)
            return
        from . import conditioning
        elev = np.array(self.elev)
        elev, n_failed, used = conditioning.pit_drain_paths(elev, self.dX, self.dY, self.drain_pits_max_iter,
                                                            self.drain_pits_max_dist, self.drain_pits_max_dist_XY,
                                                            self.fill_flats_below_sea)
        logger.info("... done draining pits with maxiter = %d", used)
        self.elev = elev

    def _pit_paths_on_device(self):
        """(n_failed, iterations, rounds) when the library carved the paths on the resident surface, else None (tiles with
        no-data cells, dtypes the device cannot hold, or the parallel schedule gave up: the caller runs the host loop).
        Integer / float32 surfaces keep numpy's in-dtype arithmetic (:537-539): the library truncates / rounds the path
        values like the array's dtype would, the pits are sorted on keys of that dtype, and the surface comes back in it."""
        elev = self._host.get('elev')
        dtype = None
        if elev is not None:
            if np.ma.isMaskedArray(elev) or np.asarray(elev).ndim != 2:
                return None
            dtype = np.asarray(elev).dtype
            if dtype not in (np.dtype('float64'), np.dtype('float32'), np.dtype('int16'), np.dtype('int32'), np.dtype('uint8'), np.dtype('int8')):
                return None
        if min(self.shape) < 3:
            return None
        self._ensure_tile()
        self._push('elev')
        res = self._tile.pit_drain_paths(self.fill_flats_below_sea, self.drain_pits_max_iter, self.drain_pits_max_dist,
                                         self.drain_pits_max_dist_XY, sort_dtype=dtype)
        if res is None:
            return None
        self._produced('elev')
        for nm in ('mag', 'direction', 'flats', 'uca', 'section', 'proportion', 'edge_todo', 'edge_done'):
            self._on_device.discard(nm)
        if dtype is not None and dtype != np.float64:
            self.elev = self.elev.astype(dtype)                # the reference edits the array in place: it keeps its dtype
        return res

    fill_depth = None             # W - z of the last calc_fill_depressions(return_depth=True) (no counterpart in the reference)
    fill_depressions_stats = None # {'epsilon', 'n_raised', 'max_depth', 'passes', 'ms'} of the last calc_fill_depressions

    def calc_fill_depressions(self, epsilon=None, outlets=None, return_depth=False):
        """Fill the depressions of the elevation (TauDEM's PitRemove, priority-flood + epsilon; no reference method), so that
        every cell drains to the tile's border, to a no-data cell or to one of `outlets`: the filled surface W keeps the open
        cells -- border, neighbours of no-data cells, `outlets` -- and is max(z, min over the 8 neighbours of (W + epsilon))
        elsewhere (include/pydem_hip.h: pydem_fill_depressions).  epsilon=0 is the classic fill: lakes become flats.
        epsilon > 0 leaves no interior pit or flat; flat areas that are not depressions get the same gradient of epsilon
        per step toward the open cells.  epsilon=None: automatic, 2**-32 of the smallest power of two >= max |z|.
        `outlets`: a boolean mask of the tile's shape or a sequence of (row, col) pairs: known sinks that must stay.  With
        epsilon == 0 the array keeps its dtype (as calc_pit_drain_paths does), otherwise it becomes float64 (as after
        calc_fill_flats).  Per tile: a depression cut by the tile's border drains off the tile.  Returns the filled
        elevation, or (elevation, depth) with return_depth (depth = W - z, float64, kept as `fill_depth`);
        `run_fill_depressions` is the same step without bringing the surface back to the host."""
        self.run_fill_depressions(epsilon, outlets, return_depth)
        return (self.elev, self.fill_depth) if return_depth else self.elev

    def run_fill_depressions(self, epsilon=None, outlets=None, return_depth=False):
        """calc_fill_depressions without the download: {'epsilon', 'n_raised', 'max_depth', 'passes', 'ms'} (epsilon as used;
        passes and ms are 0 where the host implementation served the call), kept as `fill_depressions_stats`."""
        if epsilon is not None:
            try:
                epsilon = float(epsilon)
            except (TypeError, ValueError):
                raise ValueError("epsilon must be a number >= 0 or None (got %r)" % (epsilon,))
            if not (np.isfinite(epsilon) and epsilon >= 0):
                raise ValueError("epsilon must be finite and >= 0, or None for the automatic value (got %r)" % (epsilon,))
        mask = None if outlets is None else self._outlets_mask(outlets)
        from . import conditioning
        elev = self._host.get('elev')
        dtype = None
        on_host = False
        if elev is not None:
            on_host = np.ma.isMaskedArray(elev) or np.asarray(elev).dtype.kind not in 'iuf' or np.asarray(elev).ndim != 2
            if not on_host:
                dtype = np.asarray(elev).dtype
                if epsilon:     # a value that vanishes at the surface's magnitude (the library would refuse it with -2)
                    conditioning.fill_depressions_epsilon(np.asarray(elev, dtype=np.float64), epsilon)
        if min(self.shape) < 3:
            on_host = True
        if on_host:
            W, depth, eps = conditioning.fill_depressions(self.elev, epsilon, mask)
            with np.errstate(invalid='ignore'):
                raised = depth > 0
            stats = dict(epsilon=eps, n_raised=int(raised.sum()), max_depth=float(depth[raised].max()) if raised.any() else 0.0,
                         passes=0, ms=0.0)
            if eps == 0 and dtype is not None:
                W = W.astype(dtype)                 # (a tile too small for the device: every value is one of z)
            self.elev = W
        else:
            self._ensure_tile()
            self._push('elev')
            logger.info("Starting depression filling")
            depth, eps, n_raised, max_depth, passes, ms = self._tile.fill_depressions(epsilon, mask, return_depth)
            stats = dict(epsilon=eps, n_raised=n_raised, max_depth=max_depth, passes=passes, ms=ms)
            self._produced('elev')
            if eps == 0 and dtype is not None and dtype != np.float64:
                self.elev = self.elev.astype(dtype)             # every value of the classic fill is a value of the input
        for nm in ('mag', 'direction', 'flats', 'uca', 'section', 'proportion', 'edge_todo', 'edge_done'):
            self._on_device.discard(nm)             # the fields of the surface as it was
            self._host.pop(nm, None)
        self.fill_depth = depth if return_depth else None
        self.fill_depressions_stats = stats
        return stats

    depressions = None            # {'label', 'table'} of the last calc_depressions (no counterpart in the reference)
    depressions_stats = None      # {'n_found', 'quanta', 'passes', 'ms'} of the last calc_depressions
    kept_sinks = None             # (N, 2) int array: the outlets calc_fill_depressions_limited added

    def _surface_on_host(self):
        """True when the host twin must serve a call on the elevation: a dtype the device cannot hold, or a tile with fewer than
        three rows or columns"""
        elev = self._host.get('elev')
        if elev is not None and (np.asarray(elev).dtype.kind not in 'iuf' or np.asarray(elev).ndim != 2):
            return True
        return min(self.shape) < 3

    def calc_depressions(self, outlets=None, min_depth=0.0, min_cells=1, min_volume=0.0, return_labels=True):
        """The depression inventory (closed-depression mapping; no reference method): W is the classic fill (epsilon 0) of the
        elevation with the open cells of calc_fill_depressions -- border, neighbours of no-data cells, `outlets` (a boolean mask
        of the tile's shape or a sequence of (row, col) pairs) -- and a depression is an 8-connected component of W > z, numbered
        in ascending order of its first cell in raster order (include/pydem_hip.h: pydem_depressions).  Returns {'label', 'table'},
        kept as `depressions`: the int32 label raster (0: in no kept depression, -1: no data; None without return_labels) and a
        structured array with one row per depression: cells, bounding box r0 r1 c0 c1, spill_elev, bottom_row bottom_col
        bottom_elev (the first of its lowest cells), max_depth, pour_row pour_col (the first of its sill cells: cells that are not
        raised, touch the depression and lie at its spill elevation), n_sills, open_sill (1: a sill is an open cell, the lake may
        be cut by the tile), area and volume (fixed-point sums with one result, in the units of dX * dY and z * dX * dY; their
        quanta are in `depressions_stats`) and mean_depth = volume / area.  Depressions below min_depth, min_cells or min_volume
        are dropped and the rest renumbered in the same order.  The elevation, its dtype and everything computed from it stay
        as they are.  Per tile: a depression cut by the tile's border is open there; the nested hierarchy is not computed."""
        from . import conditioning
        lim = conditioning.depression_limits("calc_depressions", min_depth=min_depth, min_cells=min_cells, min_volume=min_volume)
        if any(v is None for v in lim.values()):
            raise ValueError("calc_depressions: min_depth, min_cells and min_volume must be numbers >= 0")
        mask = None if outlets is None else self._outlets_mask(outlets)
        if self._surface_on_host():
            label, table, quanta = conditioning.label_depressions(self.elev, mask, lim['min_depth'], lim['min_cells'], lim['min_volume'],
                                                                  self.dX2 * self.dY2)
            stats = dict(n_found=None, quanta=quanta, passes=0, ms={})
        else:
            self._ensure_tile()
            self._push('elev')
            logger.info("Starting depression inventory")
            label, rows, stats = self._tile.depressions(mask, lim['min_depth'], lim['min_cells'], lim['min_volume'], return_labels)
            table = conditioning.depression_table(rows['cells'], rows['r0'], rows['r1'], rows['c0'], rows['c1'], rows['spill_elev'],
                                                  rows['bottom'], rows['bottom_elev'], rows['pour'], rows['n_sills'], rows['open_sill'],
                                                  rows['area'], rows['volume'], self.shape[1])
        self.depressions = dict(label=label if return_labels else None, table=table)
        self.depressions_stats = stats
        return self.depressions

    def calc_fill_depressions_limited(self, max_depth=None, max_cells=None, max_volume=None, epsilon=None, outlets=None, max_rounds=64):
        """The z-limit fill (ArcGIS Fill's z-limit, WhiteboxTools' max_depth): a depression deeper than max_depth, with more than
        max_cells cells or more than max_volume of volume is kept as a sink; everything else is filled, the shallow depressions
        nested inside a kept one included.  A loop over calc_depressions and calc_fill_depressions: the inventory is taken with
        the outlets collected so far, the bottoms of the depressions over a limit join the outlets (each round adds at least
        one), and when none is over a limit calc_fill_depressions(epsilon, outlets=collected) runs once.  The outlets the loop
        added are kept as `kept_sinks`, an (N, 2) int array.  RuntimeError after max_rounds rounds: the elevation is then
        untouched.  With no limit it is calc_fill_depressions.  Returns the filled elevation."""
        from . import conditioning
        lim = conditioning.depression_limits("calc_fill_depressions_limited", max_depth=max_depth, max_cells=max_cells, max_volume=max_volume)
        mask = None if outlets is None else self._outlets_mask(outlets)
        if all(v is None for v in lim.values()):
            self.kept_sinks = np.zeros((0, 2), np.int64)
            return self.calc_fill_depressions(epsilon, mask)
        before = self.depressions, self.depressions_stats
        try:
            mask, kept = conditioning.limited_outlets(lambda o: self.calc_depressions(o, return_labels=False)['table'], tuple(self.shape),
                                                      mask, lim['max_depth'], lim['max_cells'], lim['max_volume'], max_rounds)
        finally:
            self.depressions, self.depressions_stats = before
        self.kept_sinks = kept
        return self.calc_fill_depressions(epsilon, mask)

    def calc_slopes_directions(self, plotflag=False):
        """Slope magnitude and D-infinity direction (reference :587-619)."""
        self.run_slopes_directions()
        return self.mag, self.direction

    def run_slopes_directions(self):
        """calc_slopes_directions without bringing the results back to the host."""
        if self.fill_flats:
            self.calc_fill_flats()
        if self.drain_pits_path:
            self.run_pit_drain_paths()
        if self.fill_depressions:
            self.run_fill_depressions(self.fill_depressions_epsilon)
        self._ensure_tile()
        self._push('elev')
        logger.info("Starting slope/direction calculation")
        self._tile.slopes_directions()
        self._produced('mag', 'direction', 'flats')

    def calc_uca(self, plotflag=False, edge_init_data=None, uca_init=None):
        """Upstream contributing area (reference :682-776)."""
        self.run_uca(edge_init_data=edge_init_data, uca_init=uca_init)
        return self.uca

    def run_uca(self, edge_init_data=None, uca_init=None, uca_resident=False, incremental=False):
        """calc_uca without bringing the result back to the host.  `uca_resident=True` (edge rounds only)
        says uca_init is the tile's own device-resident UCA, so nothing is uploaded; `incremental=True` (with
        uca_resident) runs the round on the persistent fix-up state (pydem_uca_edge_round_inc): finished cells and
        masks are those of the plain round, cells below an unresolved inlet are settled by `flush_edge_rounds()`."""
        if not self._has('direction'):
            self.run_slopes_directions()
        if uca_init is not None or uca_resident:
            return self._calc_uca_edge_round(uca_init, edge_init_data, uca_resident,
                                             incremental and uca_resident and not self.apply_uca_limit_edges)
        if not self.drain_pits and (self.drain_flats or self.drain_pits_spill):
            # (_mk_connectivity_flats / _mk_connectivity_pits_spill, dem_processing.py:1108-1123: alternatives the
            # reference itself labels "not a great option"; only reachable with drain_pits=False)
            raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                      "device path; use drain_pits=True (the reference default) or leave both off")
        self._ensure_tile()
        self._push('elev', 'mag', 'direction', 'flats')
        opt = self._options()
        logger.info("Starting uca calculation")
        self._tile.uca(opt)
        tm = self._tile.timings()
        if tm['n_unresolved']:
            # circular drainage that the re-seed loop (dem_processing.py:951-964, replayed on the device) did not resolve
            # within circular_ref_maxcount rounds: like the reference, those cells keep the area they have received
            warnings.warn("%d cells lie on or below a circular drainage pattern that the re-seed loop did not resolve"
                          % tm['n_unresolved'])
        if tm['n_pits_undrained']:
            warnings.warn("Warning %d pits had no place to drain to in this chunk" % tm['n_pits_undrained'])
        self.twi_min_area = min(self.twi_min_area, opt.twi_min_area)
        # pits that found a drain are patched into mag/flats by the graph stage (reference :1369-1371)
        self._produced('section', 'proportion', 'uca', 'edge_todo', 'edge_done', 'mag', 'flats')

    def calc_weighted_uca(self, weights, scale_by_cell_area=True):
        """Weighted flow accumulation along the D-infinity flow graph of calc_uca: the reference's sweep (_calc_uca_chunk
        :864-987, cyutils.pyx:119-187) started from w * dX2 * dY2 (scale_by_cell_area) or w per cell instead of the cell area,
        like TauDEM's AreaDinf with a weight grid -- pit drains, the on-edge skip and the circular-drainage re-seed loop
        included, NaN on flats.  `weights`: a scalar or an array of the tile's shape, any finite values (zero and negative
        ones too); masked cells count as 0.  With weights = 1 the result is `uca` bit for bit.  Returns the float64 array."""
        self.run_weighted_uca(weights, scale_by_cell_area)
        return self.uca_weighted

    def run_weighted_uca(self, weights, scale_by_cell_area=True):
        """calc_weighted_uca without bringing the result back to the host (the `uca_weighted` attribute).  Leaves uca,
        mag, flats, the edge masks and twi_min_area alone.  The flow graph is the one calc_uca would build with the current
        options: the tile's own after calc_uca, built for the call (and not kept) otherwise."""
        w = self._weights_array(weights)
        if not self.drain_pits and (self.drain_flats or self.drain_pits_spill):
            raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                      "device path; use drain_pits=True (the reference default) or leave both off")
        if not self._has('direction'):
            self.run_slopes_directions()
        self._ensure_tile()
        self._push('elev', 'mag', 'direction', 'flats')
        self._tile.upload(_ffi.WEIGHT, w)
        logger.info("Starting weighted uca calculation")
        self._tile.uca_weighted(self._options(), scale_by_cell_area)
        # (a graph the call had to build itself is not kept: section, proportion, mag, flats, edge_todo are as they were)
        self._produced('uca_weighted')

    def _weights_array(self, weights):
        """float64 weights of the tile's shape (scalars broadcast, masked cells 0); ValueError before any device work."""
        shape = tuple(self.shape)
        if np.ma.isMaskedArray(weights):
            weights = np.ma.filled(weights.astype(np.float64), 0.0)
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim == 0:
            w = np.full(shape, float(w))
        if w.shape != shape:
            raise ValueError("weights of shape %r for a tile of shape %r" % (w.shape, shape))
        if not np.isfinite(w).all():
            raise ValueError("weights must be finite (%d NaN / inf values)" % int((~np.isfinite(w)).sum()))
        return np.ascontiguousarray(w)

    dist_down = None      # last calc_dist_down (no counterpart in the reference)
    hand = None           # last calc_hand
    dist_down_stats = None    # {'ms', 'levels', 'n_unresolved', 'kind', 'stat'} of the last calc_dist_down / calc_hand

    def calc_dist_down(self, target=None, uca_threshold=None, kind='h', stat='ave'):
        """Distance along the D-infinity flow paths of calc_uca down to the nearest target cells (TauDEM's DinfDistDown; no
        reference method).  Targets: `target`, a boolean mask of the tile's shape (masked cells are no targets), or
        `uca_threshold`: the cells with uca >= uca_threshold (the streams) -- exactly one of the two.  kind: 'h' horizontal
        distance, 'v' drop in elevation (signed), 's' distance along the surface; stat: 'ave' (flow-weighted mean over the
        out-edges), 'min' or 'max'.  NaN where some flow path from the cell does not end in a target inside the tile (it
        leaves the tile, or ends in an undrained pit or flat) and on or upstream of a drainage cycle.  Runs on the flow
        graph of calc_uca (computed first if the tile has none).  Returns the float64 array, kept as `dist_down`."""
        res = self._dist_down(target, uca_threshold, kind, stat)
        self.dist_down = res
        return res

    def calc_hand(self, uca_threshold=None, target=None):
        """Height above the nearest drainage: calc_dist_down with kind='v', stat='ave'.  Kept as `hand`."""
        res = self._dist_down(target, uca_threshold, 'v', 'ave')
        self.hand = res
        return res

    def _dist_down_target(self, target, uca_threshold, kind, stat):
        """(mask or None, threshold or None) after the checks that need no device; ValueError otherwise."""
        if kind not in _ffi.Tile.DIST_KINDS:
            raise ValueError("kind must be one of 'h', 'v', 's' (got %r)" % (kind,))
        if stat not in _ffi.Tile.DIST_STATS:
            raise ValueError("stat must be one of 'ave', 'min', 'max' (got %r)" % (stat,))
        if (target is None) == (uca_threshold is None):
            raise ValueError("give exactly one of target (a mask) and uca_threshold")
        if target is not None:
            if np.ma.isMaskedArray(target):
                target = np.ma.filled(target.astype(bool), False)
            mask = np.asarray(target)
            if mask.shape != tuple(self.shape):
                raise ValueError("target of shape %r for a tile of shape %r" % (mask.shape, tuple(self.shape)))
            return np.ascontiguousarray(mask.astype(bool)), None
        try:
            thr = float(uca_threshold)
        except (TypeError, ValueError):
            raise ValueError("uca_threshold must be a number (got %r)" % (uca_threshold,))
        if not np.isfinite(thr) or thr < 0:
            raise ValueError("uca_threshold must be finite and >= 0 (got %r)" % (uca_threshold,))
        return None, thr

    def _dist_down(self, target, uca_threshold, kind, stat):
        mask, thr = self._dist_down_target(target, uca_threshold, kind, stat)
        if not self.drain_pits and (self.drain_flats or self.drain_pits_spill):
            raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                      "device path; use drain_pits=True (the reference default) or leave both off")
        if self._tile is None or 'uca' not in self._on_device:
            self.run_uca()                     # the flow graph the distances run on (kept, with uca: nothing is thrown away)
        self._ensure_tile()
        logger.info("Starting downslope distance calculation")
        out, ms, levels, left = self._tile.dist_down(kind, stat, mask, thr)
        self.dist_down_stats = dict(ms=ms, levels=levels, n_unresolved=left, kind=kind, stat=stat)
        if left:
            warnings.warn("%d cells lie on or upstream of a circular drainage pattern: their downslope distance is NaN" % left)
        return out

    dist_up = None        # last calc_dist_up (no counterpart in the reference)
    dist_up_stats = None      # {'ms', 'levels', 'n_unresolved', 'kind', 'stat', 'edge_nan'} of the last calc_dist_up

    def calc_dist_up(self, kind='h', stat='max', edge_nan=True):
        """Distance along the D-infinity flow paths of calc_uca from the divides down to each cell (TauDEM's DinfDistUp; no
        reference method); with stat='max' the longest flow path into the cell.  kind: 'h' horizontal distance, 'v' drop in
        elevation (signed), 's' distance along the surface; stat: 'ave' (flow-weighted mean over the in-edges), 'min' or
        'max'.  0 where nothing flows into the cell, NaN where the elevation is NaN and on or downstream of a drainage cycle.
        edge_nan (TauDEM's edge contamination): the tile's border cells and the neighbours of no-data cells are NaN, and so
        is everything downstream of them -- a value is finite only where no flow path into the cell can start outside the
        tile's data; edge_nan=False gives the values of the paths inside the tile (a lower bound for 'max').  Runs on the flow
        graph of calc_uca (computed first if the tile has none).  Returns the float64 array, kept as `dist_up`."""
        if kind not in _ffi.Tile.DIST_KINDS:
            raise ValueError("kind must be one of 'h', 'v', 's' (got %r)" % (kind,))
        if stat not in _ffi.Tile.DIST_STATS:
            raise ValueError("stat must be one of 'ave', 'min', 'max' (got %r)" % (stat,))
        if not self.drain_pits and (self.drain_flats or self.drain_pits_spill):
            raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                      "device path; use drain_pits=True (the reference default) or leave both off")
        if self._tile is None or 'uca' not in self._on_device:
            self.run_uca()                     # the flow graph the distances run on (kept, with uca: nothing is thrown away)
        self._ensure_tile()
        logger.info("Starting upslope distance calculation")
        edge_nan = bool(edge_nan)
        out, ms, levels, left = self._tile.dist_up(kind, stat, edge_nan)
        self.dist_up_stats = dict(ms=ms, levels=levels, n_unresolved=left, kind=kind, stat=stat, edge_nan=edge_nan)
        if left:
            warnings.warn("%d cells lie on or downstream of a circular drainage pattern: their upslope distance is NaN" % left)
        self.dist_up = out
        return out

    up_dependence = None          # last calc_up_dependence / calc_watershed (no counterpart in the reference)
    up_dependence_stats = None    # {'ms', 'levels', 'n_unresolved'} of that call
    watershed = None              # last calc_watershed
    rev_accum = None              # last calc_rev_accum: the weighted sum downslope ...
    rev_accum_max = None          # ... and the maximum downslope
    rev_accum_stats = None        # {'sum': {'ms', 'levels', 'n_unresolved'}, 'max': {...}} of the two calls behind it

    def _mask_array(self, mask, what):
        """boolean mask of the tile's shape (masked cells False); ValueError before any device work."""
        if np.ma.isMaskedArray(mask):
            mask = np.ma.filled(mask.astype(bool), False)
        mask = np.asarray(mask)
        if mask.shape != tuple(self.shape):
            raise ValueError("%s of shape %r for a tile of shape %r" % (what, mask.shape, tuple(self.shape)))
        return np.ascontiguousarray(mask.astype(bool))

    def _rev_accum(self, what, op, seed=None, absorb=None):
        """One pydem_rev_accum call on the flow graph of calc_uca (computed first if the tile has none): (array, stats)."""
        if not self.drain_pits and (self.drain_flats or self.drain_pits_spill):
            raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                      "device path; use drain_pits=True (the reference default) or leave both off")
        if self._tile is None or 'uca' not in self._on_device:
            self.run_uca()                     # the flow graph the recursion runs on (kept, with uca: nothing is thrown away)
        self._ensure_tile()
        logger.info("Starting %s calculation" % what)
        out, ms, levels, left = self._tile.rev_accum(op, seed, absorb, 1.0)
        if left:
            warnings.warn("%d cells lie on or upstream of a circular drainage pattern: their %s is NaN" % (left, what))
        return out, dict(ms=ms, levels=levels, n_unresolved=left)

    def calc_up_dependence(self, target):
        """Upslope dependence on a target set (TauDEM's DinfUpDependence; no reference method): per cell, the fraction of its
        flow that reaches the targets along the D-infinity flow paths of calc_uca; 1 on the targets, and > 0 exactly on their
        D-infinity watershed.  `target`: a boolean mask of the tile's shape (masked cells are no targets).  Not normalised:
        the share of a cell's flow that leaves the tile, or ends in an undrained pit or flat, reaches nothing.  NaN where the
        elevation is NaN and on or upstream of a drainage cycle.  Runs on the flow graph of calc_uca (computed first if the tile
        has none).  Returns the float64 array, kept as `up_dependence`; `up_dependence_stats` holds the call's device time, levels
        and unresolved cells."""
        mask = self._mask_array(target, 'target')
        out, st = self._rev_accum('upslope dependence', 'sum', None, mask)
        self.up_dependence, self.up_dependence_stats = out, st
        return out

    def _outlets_mask(self, outlets):
        """`outlets` -- a boolean mask of the tile's shape, or a sequence of (row, col) pairs -- as a boolean mask; ValueError
        before any device work."""
        shape = tuple(self.shape)
        arr = outlets if np.ma.isMaskedArray(outlets) else np.asarray(outlets)
        pairs = arr.ndim == 2 and arr.shape[1] == 2 and arr.dtype.kind in 'iu'
        if arr.shape == shape and (arr.dtype.kind == 'b' or not pairs):
            return self._mask_array(arr, 'outlets')
        if pairs or arr.size == 0:
            arr = arr.reshape(-1, 2).astype(np.int64)
            rows, cols = arr[:, 0], arr[:, 1]
            bad = (rows < 0) | (rows >= shape[0]) | (cols < 0) | (cols >= shape[1])
            if bad.any():
                raise ValueError("outlet %r is outside the tile of shape %r" % (tuple(int(v) for v in arr[np.argmax(bad)]), shape))
            mask = np.zeros(shape, bool)
            mask[rows, cols] = True
            return mask
        raise ValueError("outlets must be a mask of shape %r or a sequence of (row, col) pairs of integers (got shape %r, dtype %s)"
                         % (shape, arr.shape, arr.dtype))

    def calc_watershed(self, outlets, min_fraction=0.0):
        """The D-infinity watershed of `outlets`: the cells of which more than `min_fraction` (in [0, 1)) of the flow reaches
        an outlet -- calc_up_dependence and a comparison (NaN is outside, the outlets themselves inside).  `outlets`: a
        boolean mask of the tile's shape, or a sequence of (row, col) pairs.  Returns the boolean mask, kept as `watershed`;
        `up_dependence` is set too."""
        try:
            frac = float(min_fraction)
        except (TypeError, ValueError):
            raise ValueError("min_fraction must be a number in [0, 1) (got %r)" % (min_fraction,))
        if not (0.0 <= frac < 1.0):
            raise ValueError("min_fraction must be in [0, 1) (got %r)" % (min_fraction,))
        mask = self._outlets_mask(outlets)
        dep = self.calc_up_dependence(mask)
        with np.errstate(invalid='ignore'):
            self.watershed = dep > frac
        return self.watershed

    def calc_rev_accum(self, weights):
        """Reverse accumulation of a per-cell load (TauDEM's DinfRevAccum; no reference method): (racc, dmax), the
        flow-weighted sum and the maximum of `weights` over the cell itself and everything downslope of it along the
        D-infinity flow paths of calc_uca.  `weights`: a scalar or an array of the tile's shape, any finite values; masked
        cells count as 0.  The sum is not normalised: flow that leaves the tile carries nothing back.  NaN where the
        elevation is NaN and on or upstream of a drainage cycle.  Runs on the flow graph of calc_uca (computed first if the tile
        has none).  Kept as `rev_accum` and `rev_accum_max`; `rev_accum_stats` holds the stats of both calls."""
        w = self._weights_array(weights)
        racc, st_sum = self._rev_accum('reverse accumulation', 'sum', w, None)
        dmax, st_max = self._rev_accum('maximum downslope load', 'max', w, None)
        self.rev_accum, self.rev_accum_max = racc, dmax
        self.rev_accum_stats = dict(sum=st_sum, max=st_max)
        return racc, dmax

    decay_accum = None            # last calc_decay_accum (no counterpart in the reference)
    decay_accum_stats = None      # {'ms', 'levels', 'n_unresolved', 'edge_nan'} of that call
    trans_lim_accum = None        # last calc_trans_lim_accum: the transport ...
    trans_lim_deposition = None   # ... and the deposition
    trans_lim_stats = None        # {'ms', 'levels', 'n_unresolved', 'edge_nan'} of that call

    def _plane_array(self, values, what, neutral):
        """float64 plane of the tile's shape (scalars broadcast, masked cells `neutral`); ValueError before any device work.
        NaN is refused here; what else the values must satisfy is the caller's to check."""
        shape = tuple(self.shape)
        if np.ma.isMaskedArray(values):
            values = np.ma.filled(values.astype(np.float64), neutral)
        try:
            a = np.asarray(values, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number or an array of numbers" % what)
        if a.ndim == 0:
            a = np.full(shape, float(a))
        if a.shape != shape:
            raise ValueError("%s of shape %r for a tile of shape %r" % (what, a.shape, shape))
        if np.isnan(a).any():
            raise ValueError("%s must not be NaN (%d NaN values)" % (what, int(np.isnan(a).sum())))
        return np.ascontiguousarray(a)

    def _fwd_accum(self, what, load, mult, cap, edge_nan, inflow):
        """One pydem_fwd_accum call on the flow graph of calc_uca (computed first if the tile has none): (array, inflow or
        None, stats)."""
        if not self.drain_pits and (self.drain_flats or self.drain_pits_spill):
            raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                      "device path; use drain_pits=True (the reference default) or leave both off")
        if self._tile is None or 'uca' not in self._on_device:
            self.run_uca()                     # the flow graph the recursion runs on (kept, with uca: nothing is thrown away)
        self._ensure_tile()
        logger.info("Starting %s calculation" % what)
        edge_nan = bool(edge_nan)
        out, flow, ms, levels, left = self._tile.fwd_accum(load, mult, cap, edge_nan, inflow)
        if left:
            warnings.warn("%d cells lie on or downstream of a circular drainage pattern: their %s is NaN" % (left, what))
        return out, flow, dict(ms=ms, levels=levels, n_unresolved=left, edge_nan=edge_nan)

    def calc_decay_accum(self, weights, decay=None, edge_nan=True):
        """Accumulation of a per-cell load that decays on its way down (TauDEM's DinfDecayAccum; no reference method): every
        cell holds its own `weights` plus, over the D-infinity in-edges of calc_uca, the flow-weighted share of decay x the
        value of the cells that flow into it.  `weights`: a scalar or an array of the tile's shape, any finite values; masked
        cells count as 0.  `decay`: the share of a cell's value that leaves it, a scalar or an array in [0, 1] (masked cells
        1), or None: the plain weighted accumulation over the graph's in-edges.  The values are the tile's own: nothing enters
        through the border.  NaN where the elevation is NaN and on or downstream of a drainage cycle.  edge_nan (TauDEM's edge
        contamination, as in calc_dist_up): the tile's border cells and the neighbours of no-data cells are NaN, and so is
        everything downstream of them -- a value is finite only where it is complete, because no flow path into the cell can
        start outside the tile's data.  Runs on the flow graph of calc_uca (computed first if the tile has none).  Returns the
        float64 array, kept as `decay_accum`; `decay_accum_stats` holds the call's device time, levels and unresolved cells."""
        w = self._weights_array(weights)
        k = None
        if decay is not None:
            k = self._plane_array(decay, 'decay', 1.0)
            if not ((k >= 0.0) & (k <= 1.0)).all():
                raise ValueError("decay must be in [0, 1] (%d values outside)" % int((~((k >= 0.0) & (k <= 1.0))).sum()))
        out, _, st = self._fwd_accum('decaying accumulation', w, k, None, edge_nan, False)
        self.decay_accum, self.decay_accum_stats = out, st
        return out

    def calc_trans_lim_accum(self, supply, capacity, edge_nan=True):
        """Transport-limited accumulation (TauDEM's DinfTransLimAccum; no reference method): (transport, deposition).  Every cell
        receives its own `supply` plus the flow-weighted transport of the cells that flow into it along the D-infinity in-edges
        of calc_uca, passes on min(that, `capacity`) -- the transport -- and keeps the rest -- the deposition, (supply + inflow)
        - transport: exactly 0 wherever the capacity does not bind, never negative.  `supply`: a scalar or an array of the
        tile's shape, finite and >= 0 (masked cells 0); `capacity`: the same, >= 0, +inf allowed (masked cells +inf).  The
        values are the tile's own; NaN, edge_nan and the flow graph as for calc_decay_accum.  Kept as `trans_lim_accum` and
        `trans_lim_deposition`; `trans_lim_stats` holds the call's device time (sweep and inflow pass), levels and unresolved cells."""
        s = self._plane_array(supply, 'supply', 0.0)
        if not (np.isfinite(s).all() and (s >= 0.0).all()):
            raise ValueError("supply must be finite and >= 0 (%d values are not)" % int((~(np.isfinite(s) & (s >= 0.0))).sum()))
        cap = self._plane_array(capacity, 'capacity', np.inf)
        if not (cap >= 0.0).all():
            raise ValueError("capacity must be >= 0 (%d negative values)" % int((cap < 0.0).sum()))
        transport, inflow, st = self._fwd_accum('transport-limited accumulation', s, None, cap, edge_nan, True)
        with np.errstate(invalid='ignore'):
            deposition = (s + inflow) - transport
        self.trans_lim_accum, self.trans_lim_deposition, self.trans_lim_stats = transport, deposition, st
        return transport, deposition

    flow_receiver = None          # last calc_flow_receiver (no counterpart in the reference)
    stream_network = None         # last calc_stream_network: a streamnet.StreamNetwork
    stream_network_stats = None   # {'ms', 'levels', 'n_unresolved', 'n_links', 'max_order'} of that call

    def _stream_network(self, mask, thr, **planes):
        """One pydem_stream_network call on the flow graph of calc_uca (computed first if the tile has none)."""
        if not self.drain_pits and (self.drain_flats or self.drain_pits_spill):
            raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                      "device path; use drain_pits=True (the reference default) or leave both off")
        if self._tile is None or 'uca' not in self._on_device:
            self.run_uca()                     # the flow graph the network lies on (kept, with uca: nothing is thrown away)
        self._ensure_tile()
        logger.info("Starting stream network calculation")
        return self._tile.stream_network(mask, thr, **planes)

    def calc_flow_receiver(self):
        """The receiver of every cell: the flat index (row * n_cols + col) of the cell its heaviest D-infinity out-edge leads to
        -- the first of greatest weight in ascending destination order, a regular edge before a pit edge to the same cell --,
        -1 where the cell has no out-edge or no data.  The receivers pick the one tree the flow graph of calc_uca (computed
        first if the tile has none) contains.  Returns the int32 array, kept as `flow_receiver`."""
        planes, _, _, _ = self._stream_network(None, None, receiver=True, order=False, link=False, basin=False)
        self.flow_receiver = planes['receiver']
        return self.flow_receiver

    def calc_stream_network(self, uca_threshold=None, streams=None, basins=True):
        """The stream network on the flow graph of calc_uca (TauDEM's StreamNet / GridNet, there on D8; no reference method).
        The streams: the cells with uca >= `uca_threshold`, or `streams`, a boolean mask of the tile's shape (masked cells are
        no streams) -- exactly one of the two.  Stream cells are joined along the receivers of calc_flow_receiver: `order` is
        the Strahler order (0 off the streams), `link` the id of the reach between two junctions (a cell with other than one
        stream inflow starts a link), `basin` the id of the link that a cell's receivers lead to (0: none; None with
        basins=False), `links` a structured array with one row per link: id (1..K in ascending head-cell order), head, tail
        (flat cells), order, n_cells and down, the id of the link below (0: none).  -1 in order, link and basin marks cells
        that circular drainage left unresolved.  Returns the streamnet.StreamNetwork, kept as `stream_network`;
        `stream_network_stats` holds the device times (receiver pass, forward sweep, reverse sweep), the levels and the
        unresolved cells of the two sweeps, the number of links and the greatest order."""
        from . import streamnet
        mask, thr = self._dist_down_target(streams, uca_threshold, 'h', 'ave')
        planes, ms, levels, left = self._stream_network(mask, thr, receiver=True, order=True, link=True, basin=bool(basins))
        net = streamnet.compact_network(planes['receiver'], planes['order'], planes['link'], planes['basin'])
        self.flow_receiver, self.stream_network = net.receiver, net
        self.stream_network_stats = dict(ms=ms, levels=levels, n_unresolved=left, n_links=int(net.links.size),
                                         max_order=int(net.order.max()) if net.order.size else 0)
        if any(left):
            warnings.warn("%d stream cells lie on or downstream of a circular drainage pattern (order and link are -1) and %d "
                          "cells lead into it (basin is -1)" % left)
        return net

    tree_accum = None             # last calc_tree_accum (no counterpart in the reference)
    tree_accum_stats = None       # {'ms', 'levels', 'n_unresolved', 'edge_nan', 'cut'} of that call
    reach_attributes = None       # last calc_reach_attributes: one row per link of `stream_network`
    reach_attributes_stats = None     # {'ms', 'sweeps': {column: {'ms', 'levels', 'n_unresolved'}}, 'edge_nan', 'n_links'}

    def _tree_accum(self, load, op, mask, thr, edge_nan, at=None, download=True):
        """One pydem_tree_accum call on the flow graph of calc_uca (computed first if the tile has none): (array or None, values
        at `at` or None, stats)."""
        if not self.drain_pits and (self.drain_flats or self.drain_pits_spill):
            raise NotImplementedError("drain_flats / drain_pits_spill (without drain_pits) are not implemented on the "
                                      "device path; use drain_pits=True (the reference default) or leave both off")
        if self._tile is None or 'uca' not in self._on_device:
            self.run_uca()                     # the flow graph the tree lies in (kept, with uca: nothing is thrown away)
        self._ensure_tile()
        logger.info("Starting receiver-tree accumulation")
        edge_nan = bool(edge_nan)
        out, vals, ms, levels, left = self._tile.tree_accum(load, op, mask, thr, edge_nan, at, download)
        return out, vals, dict(ms=ms, levels=levels, n_unresolved=left, edge_nan=edge_nan, cut=mask is not None or thr is not None)

    def _cell_area_plane(self):
        return np.ascontiguousarray(np.broadcast_to((self.dX2 * self.dY2)[:, None], tuple(self.shape)))

    def calc_tree_accum(self, weights=None, op='sum', streams=None, uca_threshold=None, edge_nan=True):
        """Accumulation along the receiver tree (the single-flow-direction, D8-style accumulation on the steepest D-infinity
        receiver of calc_flow_receiver; no reference method): every cell holds the `op` ('sum', 'max' or 'min') of its own
        `weights` and the values of the cells whose receiver it is.  `weights`: a scalar or an array of the tile's shape, any
        finite values (masked cells 0), or None: the cell area dX2 * dY2, which makes the sum the D8-style contributing area.
        With a stream set -- `streams`, a boolean mask of the tile's shape, or `uca_threshold`, not both -- the accumulation is
        cut at the link boundaries of calc_stream_network: a stream cell passes its value on only to the cell that continues its
        link, so the value at a link's tail is the reduction over that link's own sub-basin.  NaN where the elevation is NaN
        and on or downstream of a drainage cycle.  edge_nan (as in calc_dist_up): the tile's border cells and the neighbours of
        no-data cells are NaN, and so is what their values reach along the tree -- a cut stops that too, so a finite value
        under a cut says the link's own catchment lies inside the tile's data.  Runs on the flow graph of calc_uca (computed
        first if the tile has none).  Returns the float64 array, kept as `tree_accum`; `tree_accum_stats` holds the call's
        device time, levels, unresolved cells, edge_nan and cut."""
        if op not in _ffi.Tile.TREE_OPS:
            raise ValueError("op must be one of 'sum', 'max', 'min' (got %r)" % (op,))
        if streams is not None and uca_threshold is not None:
            raise ValueError("give at most one of streams (a mask) and uca_threshold")
        mask = thr = None
        if streams is not None or uca_threshold is not None:
            mask, thr = self._dist_down_target(streams, uca_threshold, 'h', 'ave')
        w = self._cell_area_plane() if weights is None else self._weights_array(weights)
        out, _, st = self._tree_accum(w, op, mask, thr, edge_nan)
        if st['n_unresolved']:
            warnings.warn("%d cells lie on or downstream of a circular drainage pattern: their tree accumulation is NaN" % st['n_unresolved'])
        self.tree_accum, self.tree_accum_stats = out, st
        return out

    def calc_reach_attributes(self, uca_threshold=None, streams=None, values=None, edge_nan=True):
        """The attribute table of the stream network's reaches (TauDEM's StreamNet table; no reference method).  Runs
        calc_stream_network(basins=False) for the stream set -- `uca_threshold` or `streams`, exactly one -- and then one
        receiver-tree accumulation (calc_tree_accum's) per catchment column, each read at the link tails only.  Returns a
        structured array with one row per link, in the order of `stream_network.links`:
            id; length, the channel length along the receivers (streamnet.channel_attributes states the formulas); drop =
            elev[head] - elev[tail]; slope = drop / length (NaN for a one-cell link); straight, the head-to-tail distance;
            local_cells / local_area, the cells / area of the link's own sub-basin (cut at the link boundaries); total_area, the
            area of everything whose receivers lead to the link's tail; magnitude, the Shreve magnitude (the sources above the
            tail); complete = local_area is finite; with `values` (an array of the tile's shape, masked cells NaN, NaN allowed)
            also v_sum, v_mean = v_sum / local_cells, v_min and v_max of it over the link's own sub-basin.
        The catchment columns are the tile's own: with edge_nan a column is NaN where the cells it covers may continue beyond
        the tile's data (for the cut columns: only this link's sub-basin), and on or downstream of circular drainage.  Kept as
        `reach_attributes`; `reach_attributes_stats` holds the device time of all sweeps and the stats of each."""
        from . import streamnet
        mask, thr = self._dist_down_target(streams, uca_threshold, 'h', 'ave')
        vals = None
        if values is not None:
            if np.ma.isMaskedArray(values):
                values = np.ma.filled(values.astype(np.float64), np.nan)
            try:
                vals = np.ascontiguousarray(values, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("values must be an array of numbers")
            if vals.shape != tuple(self.shape):
                raise ValueError("values of shape %r for a tile of shape %r" % (vals.shape, tuple(self.shape)))
        net = self.calc_stream_network(uca_threshold=thr, streams=mask, basins=False)
        tails = net.links['tail']
        area = self._cell_area_plane()
        ones = np.ones(tuple(self.shape), np.float64)
        sweeps = [('local_cells', ones, 'sum', True), ('local_area', area, 'sum', True), ('total_area', area, 'sum', False),
                  ('magnitude', streamnet.magnitude_load(net), 'sum', False)]
        if vals is not None:
            sweeps += [('v_sum', vals, 'sum', True), ('v_min', vals, 'min', True), ('v_max', vals, 'max', True)]
        at_tails, stats = {}, {}
        for name, load, op, cut in sweeps:
            _, at_tails[name], st = self._tree_accum(load, op, mask if cut else None, thr if cut else None, edge_nan, tails, False)
            stats[name] = dict(ms=st['ms'], levels=st['levels'], n_unresolved=st['n_unresolved'])
        table = streamnet.reach_table(net, self.elev, self.dX2, self.dY2, at_tails)
        self.reach_attributes = table
        self.reach_attributes_stats = dict(ms=sum(st['ms'] for st in stats.values()), sweeps=stats, edge_nan=bool(edge_nan),
                                           n_links=int(table.size))
        return table

    def build_graph(self):
        """The flow graph for a tile whose slope / aspect were set instead of computed (a resumed directory job): built now,
        before stored edge masks are uploaded (the graph stage resets them)."""
        self._ensure_tile()
        if not self._has('flats'):
            self.find_flats()
        self._push('elev', 'mag', 'direction', 'flats')
        self._tile.build_graph(self._options())
        self._produced('mag', 'flats', 'section', 'proportion')

    def restore_pit_slopes(self):
        """mag = -1 again at the pits drained by calc_uca (what the reference's slope *store* holds in
        the directory flow, process_manager.py:192-194)."""
        if self._tile is not None and 'mag' in self._on_device:
            self._tile.restore_pit_slopes()
            self._host.pop('mag', None)

    def run_edge_round_dev(self):
        """One incremental edge round whose strips the edge board (pydem_board_eval) has put into the tile's buffers."""
        self._ensure_tile()
        self._tile.uca_edge_round_dev(self._options())
        self._produced('uca', 'edge_todo', 'edge_done')

    def flush_edge_rounds(self):
        """End of a series of incremental edge rounds (no-op otherwise)."""
        if self._tile is not None:
            self._tile.uca_edge_flush()
            self._host.pop('uca', None)

    def _calc_uca_edge_round(self, uca_init, edge_init_data, uca_resident=False, incremental=False):
        """calc_uca(uca_init=..., edge_init_data=[data, done, todo]) of the reference (:724-771):
        only the contributions entering through finished neighbour edges are propagated."""
        keys = ('left', 'right', 'top', 'bottom')
        n, m = self.shape
        lens = dict(left=n, right=n, top=m, bottom=m)
        if edge_init_data is None:
            data = {k: np.zeros(lens[k]) for k in keys}
            done = {k: np.zeros(lens[k], bool) for k in keys}
            todo = {k: np.zeros(lens[k], bool) for k in keys}
        else:
            data, done, todo = edge_init_data
        self._ensure_tile()
        if not self._has('flats'):
            self.find_flats()
        if not (uca_resident and self._has('uca')):                           # (a resumed tile holds its own uca on the host)
            self.uca = np.asarray(uca_init).astype('float64')                 # :744
        self._push('elev', 'mag', 'direction', 'flats', 'uca')
        opt = self._options()
        logger.info("Starting edge resolution round")
        self._tile.uca_edge_update(opt, [data[k] for k in keys], [done[k] for k in keys], [todo[k] for k in keys],
                                   incremental=incremental and 'edge_done' in self._on_device)
        self._produced('uca', 'edge_todo', 'edge_done', 'mag', 'flats', 'section', 'proportion')

    def calc_twi(self):
        """Topographic wetness index; returns the un-scaled array, stores 10x in self.twi (:1647-1677)."""
        self.run_twi()
        return self._tile.download(_ffi.TWI)

    def run_twi(self):
        """calc_twi without bringing the result back to the host."""
        if not self._has('uca'):
            self.run_uca()
        self._ensure_tile()
        self._push('uca', 'mag')
        self._tile.twi(self._options())
        self._twi10 = None
        self._twi_on_device = True
