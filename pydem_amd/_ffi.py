"""ctypes binding of libpydem_hip.so (C-ABI declared in include/pydem_hip.h).

The product path has no CPU fallback: if the library is missing or no MI355X is visible the
calls raise.  Nothing here imports torch or the oracle.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libpydem_hip.so')

# enum pydem_field
ELEV, MAG, DIRECTION, FLATS, SECTION, PROPORTION, UCA, TWI, EDGE_TODO, EDGE_DONE, WEIGHT, UCA_WEIGHTED = range(12)
FIELD_DTYPE = {ELEV: np.float64, MAG: np.float64, DIRECTION: np.float64, FLATS: np.uint8,
               SECTION: np.int8, PROPORTION: np.float64, UCA: np.float64, TWI: np.float64,
               EDGE_TODO: np.uint8, EDGE_DONE: np.uint8, WEIGHT: np.float64, UCA_WEIGHTED: np.float64}
# enum pydem_dtype
_DTYPES = {np.dtype('float64'): 0, np.dtype('float32'): 1, np.dtype('int16'): 2, np.dtype('int32'): 3,
           np.dtype('uint8'): 4, np.dtype('int8'): 5, np.dtype('bool'): 4}


class Options(C.Structure):
    """struct pydem_options (defaults = DEMProcessor traits, reference dem_processing.py:105-154)"""
    _fields_ = [('drain_pits', C.c_int32), ('drain_pits_min_border', C.c_int32),
                ('drain_pits_max_iter', C.c_int32), ('drain_pits_max_dist', C.c_int32),
                ('drain_pits_max_dist_XY', C.c_double), ('apply_uca_limit_edges', C.c_int32),
                ('apply_twi_limits', C.c_int32), ('apply_twi_limits_on_uca', C.c_int32),
                ('circular_ref_maxcount', C.c_int32), ('uca_saturation_limit', C.c_double),
                ('twi_min_slope', C.c_double), ('twi_min_area', C.c_double)]


class Timings(C.Structure):
    """struct pydem_timings"""
    _fields_ = [('slopes_directions_ms', C.c_double), ('stencil_kernel_ms', C.c_double),
                ('flats_ms', C.c_double), ('graph_ms', C.c_double), ('pits_ms', C.c_double),
                ('sweep_ms', C.c_double), ('twi_ms', C.c_double), ('sweep_rounds', C.c_int64),
                ('sweep_kernel_launches', C.c_int64), ('n_flats', C.c_int64), ('n_pit_edges', C.c_int64),
                ('n_pits_undrained', C.c_int64), ('n_unresolved', C.c_int64), ('sweep_tile_passes', C.c_int64),
                ('n_pits', C.c_int64), ('n_pits_row', C.c_int64), ('n_pits_wave', C.c_int64), ('n_pits_big', C.c_int64),
                ('uca_weighted_ms', C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/pydem_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_PP = C.POINTER(C.c_void_p)
SYMBOLS = {
    'pydem_hip_last_error': (C.c_char_p, []),
    'pydem_hip_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'pydem_hip_device_memory': (C.c_int, [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'pydem_hip_release_scratch': (C.c_int, []),
    'pydem_hip_poison_stats': (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'pydem_hip_device_name': (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    'pydem_tile_create': (C.c_int, [C.c_int64, C.c_int64, C.c_int, _PP]),
    'pydem_tile_destroy': (C.c_int, [_P]),
    'pydem_tile_set_spacing': (C.c_int, [_P, _P, _P, _P, _P]),
    'pydem_tile_upload': (C.c_int, [_P, C.c_int, _P, C.c_int]),
    'pydem_tile_download': (C.c_int, [_P, C.c_int, _P]),
    'pydem_tile_get_line': (C.c_int, [_P, C.c_int, C.c_int, C.c_int64, _P]),
    'pydem_tile_set_line': (C.c_int, [_P, C.c_int, C.c_int, C.c_int64, _P]),
    'pydem_tile_get_lines': (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    'pydem_cond_pit_artifacts': (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int32, C.c_double, C.c_int, _P]),
    'pydem_cond_fill_flats': (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int32, C.c_double, C.c_int, C.c_int]),
    'pydem_cond_pit_paths': (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P, C.c_int, C.c_int,
                                       C.c_double, C.c_int, _P, _P]),
    'pydem_tiff_lzw_encode': (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P]),
    'pydem_tile_synchronize': (C.c_int, [_P]),
    'pydem_tile_timings': (C.c_int, [_P, C.POINTER(Timings)]),
    'pydem_tile_device_bytes': (C.c_int64, [_P]),
    'pydem_tile_synth_fractal': (C.c_int, [_P, C.c_uint32, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                           C.c_double, C.c_double]),
    'pydem_fill_flats': (C.c_int, [_P, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _P]),
    'pydem_fill_depressions': (C.c_int, [_P, C.POINTER(C.c_double), _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    'pydem_fill_seam_begin': (C.c_int, [_P, _P, _P, _P, _P, _P, C.POINTER(C.c_double)]),
    'pydem_fill_seam_relax': (C.c_int, [_P, C.c_double, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    'pydem_fill_seam_get_lines': (C.c_int, [_P, C.c_int, _P, _P, _P]),
    'pydem_fill_seam_end': (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    'pydem_fill_seam_label': (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'pydem_fill_seam_label_roots': (C.c_int, [_P, C.c_int64, _P, _P]),
    'pydem_fill_seam_get_id_lines': (C.c_int, [_P, C.c_int, _P, _P, _P]),
    'pydem_fill_seam_inventory': (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.POINTER(C.c_double)]),
    'pydem_fill_seam_labels': (C.c_int, [_P, _P, _P, C.POINTER(C.c_double)]),
    'pydem_depressions': (C.c_int, [_P, _P, C.c_double, C.c_int64, C.c_double, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P,
                                    C.POINTER(C.c_int64), _P]),
    'pydem_depressions_table': (C.c_int, [_P, C.c_int64, _P]),
    'pydem_hand_table': (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    'pydem_terrain_attributes': (C.c_int, [_P, C.c_int, _P, C.c_double, _P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'pydem_horizon': (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'pydem_pit_candidates': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    'pydem_pit_candidates_read': (C.c_int, [_P, C.c_int64, _P, _P]),
    'pydem_pit_paths': (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    'pydem_slopes_directions': (C.c_int, [_P]),
    'pydem_find_flats': (C.c_int, [_P]),
    'pydem_tile_flats_state': (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    'pydem_uca': (C.c_int, [_P, C.POINTER(Options)]),
    'pydem_uca_weighted': (C.c_int, [_P, C.POINTER(Options), C.c_int]),
    'pydem_dist_down': (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_double, _P, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]),
    'pydem_dist_up': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'pydem_rev_accum': (C.c_int, [_P, C.c_int, _P, _P, C.c_double, _P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'pydem_fwd_accum': (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'pydem_tree_accum': (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_double, C.c_int, _P, _P, C.c_int64, _P, C.POINTER(C.c_double),
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'pydem_stream_network': (C.c_int, [_P, _P, C.c_double, _P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64)]),
    'pydem_build_graph': (C.c_int, [_P, C.POINTER(Options)]),
    'pydem_uca_edge_update': (C.c_int, [_P, C.POINTER(Options), _PP, _PP, _PP]),
    'pydem_uca_edge_round_inc': (C.c_int, [_P, C.POINTER(Options), _PP, _PP, _PP]),
    'pydem_uca_edge_round_inc_dev': (C.c_int, [_P, C.POINTER(Options)]),
    'pydem_uca_edge_flush': (C.c_int, [_P]),
    'pydem_twi': (C.c_int, [_P, C.POINTER(Options)]),
    'pydem_tile_pit_edges': (C.c_int, [_P, C.POINTER(C.c_int64), _P, _P, _P]),
    'pydem_tile_graph_words': (C.c_int, [_P, _P]),
    'pydem_tile_restore_pit_slopes': (C.c_int, [_P]),
    'pydem_bench_stencil': (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    'pydem_drain_area': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, C.c_int]),
    'pydem_drain_connections': (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_uint8, C.c_int]),
    'pydem_comm_unique_id': (C.c_int, [C.c_char_p]),
    'pydem_comm_create': (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_int, _PP]),
    'pydem_comm_destroy': (C.c_int, [_P]),
    'pydem_comm_begin': (C.c_int, [_P, C.c_int64]),
    'pydem_comm_pack_line': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int64, C.c_int64]),
    'pydem_comm_pack_lines': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P]),
    'pydem_comm_put': (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    'pydem_comm_allreduce': (C.c_int, [_P, C.c_int64, C.c_int, _P]),
    'pydem_board_create': (C.c_int, [C.c_int, C.c_int, C.c_int64, _PP]),
    'pydem_board_destroy': (C.c_int, [_P]),
    'pydem_board_set_desc': (C.c_int, [_P, C.c_int, C.c_int32, C.c_int32, _P, _P, _P]),
    'pydem_board_set_lines': (C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, _P, C.c_int, _P, _P, _P, _P]),
    'pydem_board_refresh': (C.c_int, [_P, _P, C.c_int, _P]),
    'pydem_board_refresh_stage': (C.c_int, [_P, C.c_int, _P, _P, C.c_int64, _P]),
    'pydem_board_refresh_unstage': (C.c_int, [_P, C.c_int, _P, _P, C.c_int64]),
    'pydem_board_eval': (C.c_int, [_P, C.c_int, _P, _P, _P]),
    'pydem_board_download': (C.c_int, [_P, _P]),
    'pydem_board_run_waves': (C.c_int, [_P, _P, C.c_int, _P, _P]),
    'pydem_board_prepare_waves': (C.c_int, [_P, C.c_int, C.c_uint64]),
    'pydem_board_run_waves_ex': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P]),
    'pydem_comm_count': (C.c_int, [_P, _P]),
    'pydem_tile_edge_queue_ready': (C.c_int, [_P]),
}

_lib = None


def load():
    """dlopen the library and bind every declared symbol (fails loudly if anything is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libpydem_hip.so is not built (%s); run `python -m pydem_amd.build`. "
                               "There is no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)   # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class HipError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise HipError("libpydem_hip error %d: %s" % (rc, load().pydem_hip_last_error().decode()))


def _ptr(a):
    """The array's buffer as a void* argument; None is the null pointer."""
    return a.ctypes.data_as(_P) if a is not None else None


def _sweep(fn, *args):
    """One flow-graph sweep export, whose last three parameters are double *ms, int64_t *levels, int64_t *n_unresolved:
    (device ms, levels, unresolved cells)."""
    ms, levels, left = C.c_double(0), C.c_int64(0), C.c_int64(0)
    check(fn(*(args + (C.byref(ms), C.byref(levels), C.byref(left)))))
    return ms.value, int(levels.value), int(left.value)


def device_count():
    n = C.c_int(0)
    check(load().pydem_hip_device_count(C.byref(n)))
    return n.value


def release_scratch():
    """Return the per-device scratch arenas of the conditioning stages to the driver."""
    check(load().pydem_hip_release_scratch())


def poison_stats():
    """(blocks, bytes) of device memory that PYDEM_MEM_POISON has filled at hand-out in this process."""
    n, b = C.c_int64(0), C.c_int64(0)
    check(load().pydem_hip_poison_stats(C.byref(n), C.byref(b)))
    return n.value, b.value


def device_memory(device=0):
    """(free, total) bytes of the device's HBM."""
    f, tot = C.c_int64(0), C.c_int64(0)
    check(load().pydem_hip_device_memory(int(device), C.byref(f), C.byref(tot)))
    return f.value, tot.value


class Tile(object):
    """Owns one device-resident tile handle."""

    def __init__(self, n_rows, n_cols, device=0):
        self.lib = load()
        self.shape = (int(n_rows), int(n_cols))
        self._h = C.c_void_p()
        check(self.lib.pydem_tile_create(n_rows, n_cols, device, C.byref(self._h)))

    def close(self):
        if self._h:
            self.lib.pydem_tile_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mask(self, a, what):
        """`a` as a uint8 mask (nonzero: set) of the tile's shape"""
        mask = np.ascontiguousarray(np.asarray(a) != 0, np.uint8)
        if mask.shape != self.shape:
            raise ValueError("%s of shape %r for a tile of shape %r" % (what, mask.shape, self.shape))
        return mask

    def _plane(self, a, what):
        """`a` as a float64 plane of the tile's shape"""
        a = np.ascontiguousarray(a, np.float64)
        if a.shape != self.shape:
            raise ValueError("%s of shape %r for a tile of shape %r" % (what, a.shape, self.shape))
        return a

    def set_spacing(self, dX, dY, dX2, dY2):
        arrs = [np.ascontiguousarray(a, np.float64) for a in (dX, dY, dX2, dY2)]
        n = self.shape[0]
        assert arrs[0].size == n - 1 and arrs[1].size == n - 1 and arrs[2].size == n and arrs[3].size == n
        check(self.lib.pydem_tile_set_spacing(self._h, *[a.ctypes.data_as(_P) for a in arrs]))

    def upload(self, field, arr):
        arr = np.ascontiguousarray(arr)
        if arr.shape != self.shape:
            raise ValueError("field %d: array of shape %r uploaded to a tile of shape %r" % (field, arr.shape, self.shape))
        if FIELD_DTYPE[field] != np.float64:
            arr = np.ascontiguousarray(arr.astype(FIELD_DTYPE[field], copy=False))
            dt = _DTYPES[arr.dtype]
        else:
            if arr.dtype not in _DTYPES or arr.dtype == np.bool_:
                arr = np.ascontiguousarray(arr, np.float64)
            dt = _DTYPES[arr.dtype]
        check(self.lib.pydem_tile_upload(self._h, field, arr.ctypes.data_as(_P), dt))

    def download(self, field):
        out = np.empty(self.shape, FIELD_DTYPE[field])
        check(self.lib.pydem_tile_download(self._h, field, out.ctypes.data_as(_P)))
        return out

    def get_line(self, field, axis, index):
        out = np.empty(self.shape[1] if axis == 0 else self.shape[0], FIELD_DTYPE[field])
        check(self.lib.pydem_tile_get_line(self._h, field, axis, index, out.ctypes.data_as(_P)))
        return out

    def get_lines(self, requests):
        """requests: [(field, axis, index)] -> list of 1-D arrays, one device synchronisation for all."""
        k = len(requests)
        outs = [np.empty(self.shape[1] if axis == 0 else self.shape[0], FIELD_DTYPE[field]) for field, axis, _ in requests]
        fields = (C.c_int * k)(*[r[0] for r in requests])
        axes = (C.c_int * k)(*[r[1] for r in requests])
        idx = (C.c_int64 * k)(*[r[2] for r in requests])
        dsts = (C.c_void_p * k)(*[o.ctypes.data for o in outs])
        check(self.lib.pydem_tile_get_lines(self._h, k, fields, axes, idx, dsts))
        return outs

    def set_line(self, field, axis, index, values):
        v = np.ascontiguousarray(values, FIELD_DTYPE[field])
        assert v.size == (self.shape[1] if axis == 0 else self.shape[0])
        check(self.lib.pydem_tile_set_line(self._h, field, axis, index, v.ctypes.data_as(_P)))

    def synth_fractal(self, seed=0, row0=0, col0=0, n_octaves=12, top_shift=12, zmin=1.0, zrange=1000.0):
        check(self.lib.pydem_tile_synth_fractal(self._h, seed, row0, col0, n_octaves, top_shift, zmin, zrange))

    def slopes_directions(self):
        check(self.lib.pydem_slopes_directions(self._h))

    def find_flats(self):
        check(self.lib.pydem_find_flats(self._h))

    def flats_state(self):
        """(state, full passes, pit-only passes, elided calls) of pydem_tile_flats_state"""
        st, cnt = C.c_int(0), (C.c_int64 * 3)()
        check(self.lib.pydem_tile_flats_state(self._h, C.byref(st), cnt))
        return st.value, int(cnt[0]), int(cnt[1]), int(cnt[2])

    def fill_flats(self, max_pit_area, below_sea, source_tol, peaks, pits, artefacts_only=False):
        """Conditioning on the resident elevation; returns False when the tile must go through the host path (NaN cells)."""
        flag = C.c_int(0)
        check(self.lib.pydem_fill_flats(self._h, float(max_pit_area or 0.0), int(bool(below_sea)), float(source_tol), int(bool(peaks)),
                                        int(bool(pits)), int(bool(artefacts_only)), C.byref(flag)))
        return flag.value == 0

    def fill_depressions(self, epsilon=None, outlets=None, want_depth=False):
        """pydem_fill_depressions on the resident elevation: (depth or None, epsilon used, raised cells, maximum depth, passes,
        device ms).  epsilon: None (or < 0) is automatic; outlets: a mask of the tile's shape or None."""
        eps = C.c_double(-1.0 if epsilon is None else float(epsilon))
        mask = None if outlets is None else self._mask(outlets, 'outlets mask')
        depth = np.empty(self.shape, np.float64) if want_depth else None
        raised, dmax, passes, ms = C.c_int64(0), C.c_double(0), C.c_int64(0), C.c_double(0)
        check(self.lib.pydem_fill_depressions(self._h, C.byref(eps), _ptr(mask), _ptr(depth), C.byref(raised), C.byref(dmax),
                                              C.byref(passes), C.byref(ms)))
        return depth, eps.value, int(raised.value), dmax.value, int(passes.value), ms.value

    # the fill across tiles: a session on the tile (pydem_fill_seam_*); lines are keyed 'top', 'bottom', 'left', 'right'
    SEAM_SIDES = ('top', 'bottom', 'left', 'right')

    def _side_lines(self, lines, dtype, what):
        """the four optional lines of `lines` (a dict by side, or None) as contiguous arrays of `dtype` (None: NULL)"""
        out = []
        for side in self.SEAM_SIDES:
            a = None if lines is None else lines.get(side)
            if a is not None:
                a = np.ascontiguousarray(np.asarray(a) != 0, np.uint8) if dtype == np.uint8 else np.ascontiguousarray(a, dtype)
                want = self.shape[1] if side in ('top', 'bottom') else self.shape[0]
                if a.shape != (want,):
                    raise ValueError("%s line %r of shape %r for a tile of shape %r" % (what, side, a.shape, self.shape))
            out.append(a)
        return out

    def fill_seam_begin(self, seam=None, outlets=None):
        """pydem_fill_seam_begin: max |z| of the resident elevation.  seam: {'top' | 'bottom' | 'left' | 'right': mask line}."""
        mask = None if outlets is None else self._mask(outlets, 'outlets mask')
        lines = self._side_lines(seam, np.uint8, 'seam')
        amax = C.c_double(0)
        check(self.lib.pydem_fill_seam_begin(self._h, _ptr(mask), *([_ptr(a) for a in lines] + [C.byref(amax)])))
        return amax.value

    def fill_seam_relax(self, eps, caps=None):
        """pydem_fill_seam_relax: (cells that fell, passes, device ms).  caps: {side: float64 line}; a missing side is unchanged."""
        lines = self._side_lines(caps, np.float64, 'cap')
        low, passes, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        check(self.lib.pydem_fill_seam_relax(self._h, float(eps), *([_ptr(a) for a in lines] + [C.byref(low), C.byref(passes), C.byref(ms)])))
        return int(low.value), int(passes.value), ms.value

    def fill_seam_lines(self, requests):
        """pydem_fill_seam_get_lines: [(axis, index)] -> list of float64 lines of the session's W, one synchronisation for all."""
        k = len(requests)
        outs = [np.empty(self.shape[1] if axis == 0 else self.shape[0], np.float64) for axis, _ in requests]
        if k:
            axes = (C.c_int * k)(*[int(r[0]) for r in requests])
            idx = (C.c_int64 * k)(*[int(r[1]) for r in requests])
            dsts = (C.c_void_p * k)(*[o.ctypes.data for o in outs])
            check(self.lib.pydem_fill_seam_get_lines(self._h, k, axes, idx, dsts))
        return outs

    def fill_seam_end(self, commit=True, want_depth=False):
        """pydem_fill_seam_end: (depth or None, raised cells, maximum depth); an abort (commit=False) returns (None, 0, 0.0)."""
        depth = np.empty(self.shape, np.float64) if (want_depth and commit) else None
        raised, dmax = C.c_int64(0), C.c_double(0)
        check(self.lib.pydem_fill_seam_end(self._h, int(bool(commit)), _ptr(depth), C.byref(raised), C.byref(dmax)))
        return depth, int(raised.value), dmax.value

    # the session's inventory part (pydem_fill_seam_label ...): the tile's share of the depression inventory of the mosaic
    _seam_n_local = -1            # local ids of the last fill_seam_label (the library reads that many lookup entries, and entry 0)

    def fill_seam_label(self):
        """pydem_fill_seam_label + _label_roots: (roots, levels, largest depth, device ms) -- the first cell (int32 linear index) and
        the level of each local component of W > z, in the order of their local ids 1 .. len(roots)."""
        k, dmax, ms = C.c_int64(0), C.c_double(0), C.c_double(0)
        check(self.lib.pydem_fill_seam_label(self._h, C.byref(k), C.byref(dmax), C.byref(ms)))
        roots, levels = np.empty(k.value, np.int32), np.empty(k.value, np.float64)
        check(self.lib.pydem_fill_seam_label_roots(self._h, k.value, _ptr(roots), _ptr(levels)))
        self._seam_n_local = int(k.value)
        return roots, levels, dmax.value, ms.value

    def fill_seam_id_lines(self, requests):
        """pydem_fill_seam_get_id_lines: [(axis, index)] -> list of int32 lines of the session's id plane, one synchronisation for all."""
        k = len(requests)
        outs = [np.empty(self.shape[1] if axis == 0 else self.shape[0], np.int32) for axis, _ in requests]
        if k:
            axes = (C.c_int * k)(*[int(r[0]) for r in requests])
            idx = (C.c_int64 * k)(*[int(r[1]) for r in requests])
            dsts = (C.c_void_p * k)(*[o.ctypes.data for o in outs])
            check(self.lib.pydem_fill_seam_get_id_lines(self._h, k, axes, idx, dsts))
        return outs

    def fill_seam_inventory(self, lut, n_rows, owner, halo_ids, halo_W, row_area, shift_area, shift_volume, outlets=None):
        """pydem_fill_seam_inventory: (partial table, uint64 [13, n_rows]; device ms).  The shapes are checked here, the values by
        the library."""
        n, m = self.shape
        lut = np.ascontiguousarray(lut, np.int32)
        owner = self._mask(owner, 'owner plane')
        mask = None if outlets is None else self._mask(outlets, 'outlets mask')
        halo_ids = np.ascontiguousarray(halo_ids, np.int32)
        halo_W = np.ascontiguousarray(halo_W, np.float64)
        row_area = np.ascontiguousarray(row_area, np.float64)
        ring = 2 * m + 2 * n + 4
        if halo_ids.shape != (ring,) or halo_W.shape != (ring,) or row_area.shape != (n,) or lut.ndim != 1:
            raise ValueError("fill_seam_inventory: halo of %r / %r entries (%d wanted), row_area of shape %r for a tile of shape %r"
                             % (halo_ids.shape, halo_W.shape, ring, row_area.shape, self.shape))
        table = np.zeros((13, int(n_rows)), np.uint64)
        ms = C.c_double(0)
        # (the library reads n_local + 1 lookup entries: the length is checked against the labels it holds)
        self._seam_lut_check(lut)
        check(self.lib.pydem_fill_seam_inventory(self._h, _ptr(lut), int(n_rows), _ptr(owner), _ptr(mask), _ptr(halo_ids), _ptr(halo_W),
                                                 _ptr(row_area), int(shift_area), int(shift_volume), _ptr(table), C.byref(ms)))
        return table, ms.value

    def _seam_lut_check(self, lut):
        """ValueError unless `lut` has one entry per local id of the session's labels, plus entry 0"""
        if lut.shape != (self._seam_n_local + 1,):
            raise ValueError("fill_seam: a lookup of shape %r for %d local ids (one entry each, and entry 0)" % (lut.shape, self._seam_n_local))

    def fill_seam_labels(self, lut):
        """pydem_fill_seam_labels: (int32 label plane, device ms); lut: local id -> label, entry 0 unused."""
        lut = np.ascontiguousarray(lut, np.int32)
        self._seam_lut_check(lut)
        label = np.empty(self.shape, np.int32)
        ms = C.c_double(0)
        check(self.lib.pydem_fill_seam_labels(self._h, _ptr(lut), _ptr(label), C.byref(ms)))
        return label, ms.value

    # struct pydem_depression (include/pydem_hip.h)
    DEPRESSION_ROW = np.dtype([(nm, np.int64) for nm in ('cells', 'r0', 'r1', 'c0', 'c1', 'bottom', 'pour', 'n_sills', 'open_sill')] +
                              [(nm, np.float64) for nm in ('spill_elev', 'bottom_elev', 'max_depth', 'area', 'volume')])
    DEPRESSION_PARTS = ('total', 'relax', 'local', 'merge', 'flatten', 'number', 'stats', 'table', 'label')

    def depressions(self, outlets=None, min_depth=0.0, min_cells=1, min_volume=0.0, want_labels=True):
        """pydem_depressions on the resident elevation: (label raster or None, rows (DEPRESSION_ROW), info) with info =
        {'n_found', 'quanta': (area, volume), 'passes', 'ms': {part: device ms}}.  outlets: a mask of the tile's shape or None."""
        mask = None if outlets is None else self._mask(outlets, 'outlets mask')
        label = np.empty(self.shape, np.int32) if want_labels else None
        found, kept, passes = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        quanta, ms = np.zeros(2), np.zeros(len(self.DEPRESSION_PARTS))
        check(self.lib.pydem_depressions(self._h, _ptr(mask), float(min_depth), int(min_cells), float(min_volume), _ptr(label),
                                         C.byref(found), C.byref(kept), _ptr(quanta), C.byref(passes), _ptr(ms)))
        rows = np.zeros(int(kept.value), self.DEPRESSION_ROW)
        check(self.lib.pydem_depressions_table(self._h, int(kept.value), rows.ctypes.data_as(_P)))
        return label, rows, dict(n_found=int(found.value), quanta=(float(quanta[0]), float(quanta[1])), passes=int(passes.value),
                                 ms=dict(zip(self.DEPRESSION_PARTS, ms.tolist())))

    HAND_TABLE_PARTS = ('total', 'maxima', 'sums')

    def hand_table(self, zone, stages, K, hand=None):
        """pydem_hand_table: (int64 [K, S, 4] -- cells, area, area x HAND, bed area per zone and bin --, int64 [K, 2] -- NaN cells,
        cells above the top stage --, quanta (area, area x HAND, bed area), {part: device ms}).  zone: int32 ids of the tile's
        shape, 1..K; hand: float64 of the tile's shape, or None: the result plane of the last dist_down as it stands on the
        device.  The library checks the stages and the ids (HipError -2)."""
        zone = np.ascontiguousarray(zone, np.int32)
        if zone.shape != self.shape:
            raise ValueError("zone plane of shape %r for a tile of shape %r" % (zone.shape, self.shape))
        h = None if hand is None else self._plane(hand, 'HAND plane')
        st = np.ascontiguousarray(stages, np.float64).ravel()
        K = int(K)
        ints = np.zeros((max(K, 0), st.size, 4), np.int64)
        skipped = np.zeros((max(K, 0), 2), np.int64)
        quanta, ms = np.zeros(3), np.zeros(len(self.HAND_TABLE_PARTS))
        check(self.lib.pydem_hand_table(self._h, _ptr(zone), _ptr(h), _ptr(st), st.size, K, _ptr(ints), _ptr(skipped), _ptr(quanta),
                                        _ptr(ms)))
        return ints, skipped, tuple(float(v) for v in quanta), dict(zip(self.HAND_TABLE_PARTS, ms.tolist()))

    # enum pydem_terrain_attr, in its order
    TERRAIN_ATTRS = ('dzdx', 'dzdy', 'gradient', 'aspect', 'profile', 'plan', 'tangential', 'mean', 'hillshade')

    def terrain_attributes(self, which, half_width, light=None, z_factor=1.0, out=None):
        """pydem_terrain_attributes: ({name: float64 [n, m]} for the names in `which`, device ms, defined cells).  light: the unit
        vector to the sun (east, north, up), needed for 'hillshade'; out: {name: array} to fill instead of new arrays (C-contiguous
        float64 of the tile's shape).  The library checks the rest (HipError -2)."""
        planes = {nm: np.empty(self.shape, np.float64) if out is None else out[nm] for nm in which}
        for nm, a in planes.items():
            if a.shape != self.shape or a.dtype != np.float64 or not a.flags.c_contiguous:
                raise ValueError("plane %r must be a C-contiguous float64 array of shape %r" % (nm, self.shape))
        outs = (C.c_void_p * len(self.TERRAIN_ATTRS))(*[planes[nm].ctypes.data if nm in planes else None for nm in self.TERRAIN_ATTRS])
        lv = None if light is None else np.ascontiguousarray(light, np.float64).reshape(3)
        ms, count = C.c_double(0), C.c_int64(0)
        check(self.lib.pydem_terrain_attributes(self._h, int(half_width), _ptr(lv), float(z_factor), outs, C.byref(ms), C.byref(count)))
        return planes, ms.value, int(count.value)

    def horizon(self, table, edge_nan=True, want_horizon=False, want_svf=True, out=None):
        """pydem_horizon: ({'horizon': float64 [n_dir, n, m] tangents, 'svf': float64 [n, m]} as asked for, device ms, defined
        cells).  table: a horizon.RayTable (start int32 [n_dir + 1], dr / dc int16, w float64); out: {name: array} to fill instead
        of new arrays (C-contiguous float64).  The library checks the rest (HipError -2)."""
        start = np.ascontiguousarray(table.start, np.int32)
        dr, dc = np.ascontiguousarray(table.dr, np.int16), np.ascontiguousarray(table.dc, np.int16)
        w = np.ascontiguousarray(table.w, np.float64)
        n_dir = int(start.size) - 1
        if n_dir < 1 or not (dr.size == dc.size == w.size) or (start.size and int(start[-1]) != w.size):
            raise ValueError("the ray table's arrays do not fit together")
        shapes = {}
        if want_horizon:
            shapes['horizon'] = (n_dir,) + self.shape
        if want_svf:
            shapes['svf'] = self.shape
        planes = {nm: np.empty(shp, np.float64) if out is None else out[nm] for nm, shp in shapes.items()}
        for nm, a in planes.items():
            if a.shape != shapes[nm] or a.dtype != np.float64 or not a.flags.c_contiguous:
                raise ValueError("plane %r must be a C-contiguous float64 array of shape %r" % (nm, shapes[nm]))
        hor = (C.c_void_p * n_dir)(*[planes['horizon'][d].ctypes.data for d in range(n_dir)]) if want_horizon else None
        ms, count = C.c_double(0), C.c_int64(0)
        check(self.lib.pydem_horizon(self._h, n_dir, _ptr(start), _ptr(dr), _ptr(dc), _ptr(w), int(bool(edge_nan)), hor,
                                     _ptr(planes.get('svf')), C.byref(ms), C.byref(count)))
        return planes, ms.value, int(count.value)

    def pit_drain_paths(self, below_sea, max_iter, max_dist, max_dist_XY, sort_dtype=None):
        """calc_pit_drain_paths on the resident elevation.  Returns (n_failed, iterations used, rounds), or None when the tile
        must go through the host loop (no-data cells, float32 surface, or the parallel schedule gave up: surface restored)."""
        import time
        t0 = time.perf_counter()
        n = C.c_int64(0)
        check(self.lib.pydem_pit_candidates(self._h, int(bool(below_sea)), C.byref(n)))
        if n.value < 0:
            return None
        cells = np.empty(max(n.value, 1), np.int32); elev = np.empty(max(n.value, 1), np.float64)
        check(self.lib.pydem_pit_candidates_read(self._h, n.value, cells.ctypes.data_as(_P), elev.ctypes.data_as(_P)))
        cells, elev = cells[:n.value], elev[:n.value]
        t1 = time.perf_counter()
        # the reference's call (:450) on the array's own dtype: the tie order of numpy's sort is part of the result and differs between dtypes
        keys = elev if sort_dtype is None or np.dtype(sort_dtype) == np.float64 else elev.astype(sort_dtype)
        order = np.ascontiguousarray(cells[np.argsort(keys)], np.int32)
        t2 = time.perf_counter()
        failed, used, rounds, flag = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
        check(self.lib.pydem_pit_paths(self._h, order.ctypes.data_as(_P), n.value, int(max_iter), int(max_dist or 0),
                                       float(max_dist_XY) if max_dist_XY else 0.0, C.byref(failed), C.byref(used), C.byref(rounds),
                                       C.byref(flag)))
        if os.environ.get('PYDEM_PATHS_DEBUG'):
            import sys
            sys.stderr.write("pit paths host side: candidates %.1f ms, argsort %.1f ms, pydem_pit_paths %.1f ms\n"
                             % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3))
        if flag.value:
            return None
        return int(failed.value), int(used.value), int(rounds.value)

    def uca(self, opt):
        check(self.lib.pydem_uca(self._h, C.byref(opt)))

    def uca_weighted(self, opt, scale_by_cell_area=True):
        check(self.lib.pydem_uca_weighted(self._h, C.byref(opt), int(bool(scale_by_cell_area))))

    DIST_KINDS = {'h': 0, 'v': 1, 's': 2}
    DIST_STATS = {'ave': 0, 'min': 1, 'max': 2}

    def dist_down(self, kind, stat, target=None, uca_threshold=None, download=True):
        """pydem_dist_down on the tile's flow graph: (float64 [n, m], device ms, levels, unresolved cells).  `target`: a mask
        of the tile's shape, or None with `uca_threshold`.  download=False: the sweep alone (None instead of the array)."""
        out = np.empty(self.shape, np.float64) if download else None
        mask = None if target is None else self._mask(target, 'target mask')
        return (out,) + _sweep(self.lib.pydem_dist_down, self._h, self.DIST_KINDS[kind], self.DIST_STATS[stat], _ptr(mask),
                               float(uca_threshold) if mask is None else 0.0, _ptr(out))

    def dist_up(self, kind, stat, edge_nan=True, download=True):
        """pydem_dist_up on the tile's flow graph: (float64 [n, m], device ms, levels, unresolved cells).  download=False: the
        sweep alone (None instead of the array)."""
        out = np.empty(self.shape, np.float64) if download else None
        return (out,) + _sweep(self.lib.pydem_dist_up, self._h, self.DIST_KINDS[kind], self.DIST_STATS[stat], int(bool(edge_nan)), _ptr(out))

    REV_OPS = {'sum': 0, 'max': 1}

    def rev_accum(self, op, seed=None, absorb=None, absorb_value=1.0, download=True):
        """pydem_rev_accum on the tile's flow graph: (float64 [n, m], device ms, levels, unresolved cells).  op: 'sum' / 0 or
        'max' / 1; seed: float64 of the tile's shape or None (0 everywhere); absorb: a mask of the tile's shape or None.
        download=False: the sweep alone (None instead of the array)."""
        out = np.empty(self.shape, np.float64) if download else None
        sd = None if seed is None else self._plane(seed, 'seed')
        mask = None if absorb is None else self._mask(absorb, 'absorb mask')
        return (out,) + _sweep(self.lib.pydem_rev_accum, self._h, int(self.REV_OPS.get(op, op)), _ptr(sd), _ptr(mask), float(absorb_value),
                               _ptr(out))

    def fwd_accum(self, load, mult=None, cap=None, edge_nan=True, inflow=False, download=True):
        """pydem_fwd_accum on the tile's flow graph: (float64 [n, m], inflow [n, m] or None, device ms, levels, unresolved
        cells).  load: float64 of the tile's shape; mult, cap: the same or None.  inflow: bring the inflow plane back too.
        download=False: the sweep alone (None instead of the arrays; the inflow pass still runs if asked for)."""
        out = np.empty(self.shape, np.float64) if download else None
        planes = [None if a is None else self._plane(a, name) for name, a in (('load', load), ('mult', mult), ('cap', cap))]
        # (download=False with inflow: the pass runs and its plane comes back -- the C-ABI has no other way to ask for it)
        flow = np.empty(self.shape, np.float64) if inflow else None
        return (out, flow) + _sweep(self.lib.pydem_fwd_accum, self._h, _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]),
                                    int(bool(edge_nan)), _ptr(out), _ptr(flow))

    TREE_OPS = {'sum': 0, 'max': 1, 'min': 2}

    def tree_accum(self, load, op='sum', streams=None, uca_threshold=None, edge_nan=True, at=None, download=True):
        """pydem_tree_accum on the tile's flow graph: (float64 [n, m], values at the flat cells `at` or None, device ms, levels,
        unresolved cells).  load: float64 of the tile's shape; op: 'sum' / 0, 'max' / 1 or 'min' / 2.  The accumulation is cut at
        the link boundaries exactly when a stream set is given: `streams`, a mask of the tile's shape, or `uca_threshold`.
        download=False: the sweep (and the gather) alone, None instead of the plane."""
        ld = self._plane(load, 'load')
        mask = None if streams is None else self._mask(streams, 'stream mask')
        cut = mask is not None or uca_threshold is not None
        out = np.empty(self.shape, np.float64) if download else None
        cells = vals = None
        if at is not None:
            cells = np.asarray(at)
            if cells.size and (cells.min() < -2 ** 31 or cells.max() >= 2 ** 31):
                raise ValueError("`at` holds cells outside the int32 range")
            cells = np.ascontiguousarray(cells.ravel(), np.int32)
            vals = np.empty(cells.size, np.float64)
        return (out, vals) + _sweep(self.lib.pydem_tree_accum, self._h, int(self.TREE_OPS.get(op, op)), _ptr(ld), int(cut), _ptr(mask),
                                    float(uca_threshold) if mask is None and uca_threshold is not None else 0.0,
                                    int(bool(edge_nan)), _ptr(out), _ptr(cells), cells.size if cells is not None else 0, _ptr(vals))

    def stream_network(self, streams=None, uca_threshold=None, receiver=True, order=True, link=True, basin=True):
        """pydem_stream_network on the tile's flow graph: ({'receiver', 'order', 'link', 'basin'}: int32 [n, m] or None, device ms
        (receiver pass, forward sweep, reverse sweep), levels (forward, reverse), unresolved cells (forward, reverse)).
        `streams`: a mask of the tile's shape, or None with `uca_threshold`; neither is needed for the receivers alone.  The
        four flags say which planes to bring back: link and basin hold the raw labels (head cell + 1)."""
        want = dict(receiver=receiver, order=order, link=link, basin=basin)
        planes = {k: np.empty(self.shape, np.int32) if v else None for k, v in want.items()}
        ms, levels, left = (C.c_double * 3)(), (C.c_int64 * 2)(), (C.c_int64 * 2)()
        mask = None if streams is None else self._mask(streams, 'stream mask')
        if mask is None and uca_threshold is None and (order or link or basin):
            raise ValueError("order, link and basin need a stream mask or a uca_threshold")
        check(self.lib.pydem_stream_network(self._h, _ptr(mask), float(uca_threshold) if mask is None and uca_threshold is not None else 0.0,
                                            _ptr(planes['receiver']), _ptr(planes['order']), _ptr(planes['link']), _ptr(planes['basin']),
                                            ms, levels, left))
        return planes, tuple(ms), tuple(int(v) for v in levels), tuple(int(v) for v in left)

    def build_graph(self, opt):
        check(self.lib.pydem_build_graph(self._h, C.byref(opt)))

    def uca_edge_update(self, opt, data, done, todo, incremental=False):
        """data/done/todo: sequences (left, right, top, bottom) of 1-D arrays.  incremental: pydem_uca_edge_round_inc."""
        n, m = self.shape
        lens = (n, n, m, m)
        d = [np.ascontiguousarray(np.asarray(a, np.float64).ravel()) for a in data]
        dn = [np.ascontiguousarray(np.asarray(a).ravel().astype(np.uint8)) for a in done]
        td = [np.ascontiguousarray(np.asarray(a).ravel().astype(np.uint8)) for a in todo]
        for arrs in (d, dn, td):
            assert [a.size for a in arrs] == list(lens), "edge strips must have n_rows / n_cols entries"
        pack = lambda xs: (C.c_void_p * 4)(*[x.ctypes.data_as(C.c_void_p) for x in xs])
        fn = self.lib.pydem_uca_edge_round_inc if incremental else self.lib.pydem_uca_edge_update
        check(fn(self._h, C.byref(opt), pack(d), pack(dn), pack(td)))

    def uca_edge_flush(self):
        check(self.lib.pydem_uca_edge_flush(self._h))

    def edge_queue_ready(self):
        """Can the next rounds of this tile be queued behind a device-side wave selection (Board.run_waves)?"""
        return bool(self.lib.pydem_tile_edge_queue_ready(self._h))

    def uca_edge_round_dev(self, opt):
        """Incremental edge round with the strips the edge board wrote into the tile's buffers."""
        check(self.lib.pydem_uca_edge_round_inc_dev(self._h, C.byref(opt)))

    def twi(self, opt):
        check(self.lib.pydem_twi(self._h, C.byref(opt)))

    def graph_words(self):
        """The packed graph word of every cell (static bits: in-mask, out flags, pit flags, facet), uint32 [n, m]."""
        out = np.empty(self.shape, np.uint32)
        check(self.lib.pydem_tile_graph_words(self._h, out.ctypes.data_as(_P)))
        return out

    def pit_edges(self):
        """(pit, drain, weight) triplets of the last uca() call, in emission order."""
        n = C.c_int64(0)
        check(self.lib.pydem_tile_pit_edges(self._h, C.byref(n), None, None, None))
        src = np.empty(n.value, np.int32); dst = np.empty(n.value, np.int32); w = np.empty(n.value, np.float64)
        if n.value:
            check(self.lib.pydem_tile_pit_edges(self._h, C.byref(n), src.ctypes.data_as(_P), dst.ctypes.data_as(_P),
                                                w.ctypes.data_as(_P)))
        return src, dst, w

    def restore_pit_slopes(self):
        check(self.lib.pydem_tile_restore_pit_slopes(self._h))

    def bench_stencil(self, iters):
        ms = C.c_double(0)
        check(self.lib.pydem_bench_stencil(self._h, iters, C.byref(ms)))
        return ms.value

    def synchronize(self):
        check(self.lib.pydem_tile_synchronize(self._h))

    def timings(self):
        tm = Timings()
        check(self.lib.pydem_tile_timings(self._h, C.byref(tm)))
        return tm.as_dict()

    def device_bytes(self):
        return self.lib.pydem_tile_device_bytes(self._h)


class Board(object):
    """Device-resident edge board (include/pydem_hip.h, pydem_board_*)."""

    def __init__(self, device, n_tiles, n_doubles):
        self.lib = load()
        self.n_tiles, self.n_doubles = n_tiles, n_doubles
        self._h = C.c_void_p()
        check(self.lib.pydem_board_create(device, n_tiles, n_doubles, C.byref(self._h)))
        self._out = np.zeros((n_tiles, 8), np.uint64)

    def close(self):
        if self._h:
            self.lib.pydem_board_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_desc(self, index, n, m, offsets28, flags8, tile=None):
        o = np.ascontiguousarray(offsets28, np.int64); f = np.ascontiguousarray(flags8, np.int32)
        assert o.size == 28 and f.size == 8
        check(self.lib.pydem_board_set_desc(self._h, index, n, m, o.ctypes.data_as(_P), f.ctypes.data_as(_P),
                                            tile._h if tile is not None else None))

    def set_lines(self, index, mb_start, size, tile=None, lines=()):
        """lines: [(field, axis, index, rel_offset)] of `tile` (a tile of this process), or nothing for a remote tile."""
        k = len(lines)
        fields = (C.c_int * max(k, 1))(*[l[0] for l in lines]); axes = (C.c_int * max(k, 1))(*[l[1] for l in lines])
        idx = (C.c_int64 * max(k, 1))(*[l[2] for l in lines]); offs = (C.c_int64 * max(k, 1))(*[l[3] for l in lines])
        check(self.lib.pydem_board_set_lines(self._h, index, int(mb_start), int(size), tile._h if tile is not None else None,
                                             k, fields, axes, idx, offs))

    def refresh(self, comm, tiles, host_sum=None):
        """Replicate the lines of `tiles` on the board: pack, sum over ranks, scatter.  comm: an RCCL communicator (or None in
        a single process); host_sum: a function that sums a float64 array over all ranks in place, for transports without
        RCCL (the staging buffer then makes the round trip through host memory)."""
        tiles = list(tiles)
        for k0 in range(0, len(tiles), 64):
            part = tiles[k0:k0 + 64]
            arr = (C.c_int * len(part))(*part)
            if host_sum is None:
                check(self.lib.pydem_board_refresh(self._h, comm._h if comm is not None else None, len(part), arr))
                continue
            buf = np.empty(self.n_doubles, np.float64)
            n = C.c_int64(0)
            check(self.lib.pydem_board_refresh_stage(self._h, len(part), arr, buf.ctypes.data_as(_P), buf.size, C.byref(n)))
            part_buf = buf[:n.value]
            host_sum(part_buf)
            check(self.lib.pydem_board_refresh_unstage(self._h, len(part), arr, part_buf.ctypes.data_as(_P), n.value))

    def eval(self, tiles, full):
        k = len(tiles)
        t = (C.c_int * max(k, 1))(*tiles); f = (C.c_int * max(k, 1))(*[int(v) for v in full])
        check(self.lib.pydem_board_eval(self._h, k, t, f, self._out.ctypes.data_as(_P)))
        return self._out

    def download(self):
        out = np.empty(self.n_doubles, np.float64)
        check(self.lib.pydem_board_download(self._h, out.ctypes.data_as(_P)))
        return out

    # layout of the queued waves' state (csrc/comm.hip, SCH_*)
    SCH_OK, SCH_STOP, SCH_NWAVES, SCH_LIMIT, SCH_GRAPH, SCH_ND, SCH_PD, SCH_HASH, SCH_HAS, SCH_READERS, SCH_NBRS, SCH_LOG, SCH_NTB, SCH_TBLOG, SCH_WORDS = \
        0, 1, 2, 3, 7, 8, 72, 136, 200, 264, 328, 392, 521, 522, 528

    def prepare_waves(self, staged, ok_tiles):
        """Everything a batch of queued waves over the tiles `ok_tiles` (bit mask) needs that can fail on this rank alone
        (pydem_board_prepare_waves); nothing is enqueued.  Raises HipError; with several ranks the caller lets the ranks agree on
        the outcome before any of them calls run_waves."""
        check(self.lib.pydem_board_prepare_waves(self._h, 1 if staged else 0, C.c_uint64(int(ok_tiles))))

    _EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64)

    def run_waves(self, comm, k_waves, state, exchange=None):
        """Up to k_waves waves without a host look (pydem_board_run_waves); `state` (uint64[528]) is updated in place; returns the
        scalars of all tiles like eval().  `exchange` (instead of a communicator): an object with sum_bytes_inplace(uint8 array)
        and max_inplace(float64 array) that reduce over the ranks -- the staging buffer then goes through the host once per
        wave (pydem_board_run_waves_ex; the multi-process tests on one GPU)."""
        assert state.dtype == np.uint64 and state.size == self.SCH_WORDS and state.flags.c_contiguous
        if exchange is None:
            check(self.lib.pydem_board_run_waves(self._h, comm._h if comm is not None else None, int(k_waves), state.ctypes.data_as(_P),
                                                 self._out.ctypes.data_as(_P)))
            return self._out
        failure = []

        def cb(_ctx, op, buf, n):
            try:
                if op == 0:
                    exchange.sum_bytes_inplace(np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), shape=(int(n),)))
                else:
                    exchange.max_inplace(np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_double)), shape=(int(n),)))
                return 0
            except Exception as exc:          # (an exception must not unwind through the C frames)
                failure.append(exc)
                return 1
        fn = self._EXCHANGE(cb)
        rc = self.lib.pydem_board_run_waves_ex(self._h, None, int(k_waves), state.ctypes.data_as(_P), self._out.ctypes.data_as(_P), fn, None)
        if failure:
            raise failure[0]
        check(rc)
        return self._out


class Comm(object):
    """RCCL communicator handle (one per process / GPU)."""

    def __init__(self, world, rank, uid, device=0):
        self.lib = load()
        self.world, self.rank, self.device = world, rank, device
        self._h = C.c_void_p()
        check(self.lib.pydem_comm_create(world, rank, uid, device, C.byref(self._h)))

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(load().pydem_comm_unique_id(buf))
        return buf.raw

    def count(self):
        """Ranks behind the communicator as RCCL reports them (ncclCommCount)."""
        n = C.c_int(0)
        check(self.lib.pydem_comm_count(self._h, C.byref(n)))
        return int(n.value)

    def close(self):
        if self._h:
            self.lib.pydem_comm_destroy(self._h)
            self._h = C.c_void_p()

    def begin(self, n):
        check(self.lib.pydem_comm_begin(self._h, n))

    def pack_line(self, tile, field, axis, index, offset):
        check(self.lib.pydem_comm_pack_line(self._h, tile._h, field, axis, index, offset))

    def pack_lines(self, tile, lines):
        """lines: [(field, axis, index, offset)] of ONE tile; no host synchronisation (see comm.hip)."""
        k = len(lines)
        fields = (C.c_int * k)(*[l[0] for l in lines]); axes = (C.c_int * k)(*[l[1] for l in lines])
        idx = (C.c_int64 * k)(*[l[2] for l in lines]); offs = (C.c_int64 * k)(*[l[3] for l in lines])
        check(self.lib.pydem_comm_pack_lines(self._h, tile._h, k, fields, axes, idx, offs))

    def put(self, values, offset=0):
        v = np.ascontiguousarray(values, np.float64)
        check(self.lib.pydem_comm_put(self._h, v.ctypes.data_as(_P), v.size, offset))

    def allreduce(self, n, op=0):
        out = np.empty(n, np.float64)
        check(self.lib.pydem_comm_allreduce(self._h, n, op, out.ctypes.data_as(_P)))
        return out
