/*
 * pydem_hip.h -- C-ABI of libpydem_hip.so: the MI355X (gfx950) implementation of pyDEM's
 * per-tile terrain hot path.  Plain pointers and sizes only; every call returns 0 on success
 * and a negative code on failure, with the message available from pydem_hip_last_error().
 *
 * What each entry point replaces in the reference (creare-com/pydem v1.2.1; paths relative to
 * the reference checkout):
 *
 *   pydem_slopes_directions   DEMProcessor.calc_slopes_directions  pydem/dem_processing.py:587-619
 *                             (= _tarboton_slopes_directions :1753-1903, _find_flats_edges :657-680)
 *   pydem_find_flats          DEMProcessor.find_flats              pydem/dem_processing.py:305-306
 *   pydem_uca                 DEMProcessor.calc_uca (uca_init=None) pydem/dem_processing.py:682-776,
 *                             _calc_uca_chunk :864-987, _calc_uca_section_proportion :1021-1070,
 *                             _mk_adjacency_matrix :1072-1153, _mk_connectivity_pits :1269-1382 and
 *                             the native loop cyutils.drain_area   pydem/cyfuncs/cyutils.pyx:78-187
 *   pydem_uca_weighted        the sweep of pydem_uca from a per-cell weight (_calc_uca_chunk :883-972, cyutils.pyx:78-187
 *                             with the initial areas replaced; TauDEM AreaDinf with a weight grid) -- no reference method
 *   pydem_uca_edge_update     DEMProcessor.calc_uca(uca_init=, edge_init_data=) :724-771,
 *                             _calc_uca_chunk_update :778-862, cyutils.drain_connections
 *                             pydem/cyfuncs/cyutils.pyx:35-72
 *   pydem_dist_down           downslope distance to a target set / HAND on the same flow graph (reverse sweep) -- no reference method
 *   pydem_dist_up             upslope flow-path distance from the divides (longest flow path) on the same flow graph (forward
 *                             sweep of a path statistic) -- no reference method
 *   pydem_rev_accum           upslope dependence (watersheds) and reverse accumulation on the same flow graph (reverse sweep of a
 *                             linear or max recursion over the out-edges) -- no reference method
 *   pydem_fwd_accum           decaying and transport-limited accumulation on the same flow graph (forward sweep of a linear
 *                             recursion over the in-edges with a per-source multiplier and a per-cell cap) -- no reference method
 *   pydem_stream_network      receivers, Strahler order, links and sub-basins on the same flow graph (a forward and a reverse
 *                             sweep of a labelling over the tree of heaviest out-edges) -- no reference method
 *   pydem_fill_depressions    depression filling of the resident elevation (PitRemove / priority-flood + epsilon: the greatest
 *                             fixed point of a monotone recursion, by coloured LDS block relaxation) -- no reference method
 *   pydem_fill_seam_*         the same fill across the tiles of a mosaic: a resumable relaxation per tile with caps on the lines
 *                             that neighbouring tiles share; and, on the W it ends with, the tile's part of the depression
 *                             inventory of the mosaic (_label, _label_roots, _get_id_lines, _inventory, _labels) -- no reference method
 *   pydem_depressions         the depression inventory of the resident elevation (the classic fill in scratch, a block union-find
 *                             over the raised cells, integer per-label reductions) -- no reference method
 *   pydem_hand_table          per zone and water stage, the cells, flooded area, area x HAND and wetted bed area of a HAND plane (one
 *                             pass, fixed-point sums under integer atomics) -- no reference method
 *   pydem_terrain_attributes  gradient, aspect, profile / plan / tangential / mean curvature and hillshade of the resident elevation from
 *                             a least-squares quadratic over a (2k+1)^2 window (Evans 1980, Wood 1996) -- no reference method
 *   pydem_horizon             the horizon tangent per azimuth and the sky-view factor of the resident elevation along nearest-cell
 *                             rays of a host-built table (cast shadows follow on the host) -- no reference method
 *   pydem_twi                 DEMProcessor.calc_twi               pydem/dem_processing.py:1647-1677
 *
 * Ownership: the caller owns every host buffer it passes; the library owns device memory behind
 * the opaque pydem_tile handle (create / upload / run / download / destroy).  Nothing allocated
 * by the library is ever returned to the caller.  One HIP stream per handle; calls on different
 * handles may run from different host threads.
 */
#ifndef PYDEM_HIP_H
#define PYDEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pydem_tile pydem_tile;

/* device-resident per-tile fields, for pydem_tile_upload / pydem_tile_download */
enum pydem_field {
    PYDEM_ELEV = 0,        /* float64 [n,m]  conditioned elevation                              */
    PYDEM_MAG = 1,         /* float64 [n,m]  slope magnitude, -1 on flats                       */
    PYDEM_DIRECTION = 2,   /* float64 [n,m]  D-infinity direction (rad), -1 on flats            */
    PYDEM_FLATS = 3,       /* uint8   [n,m]  flats mask                                         */
    PYDEM_SECTION = 4,     /* int8    [n,m]  facet index 0..7, -1 on flats                      */
    PYDEM_PROPORTION = 5,  /* float64 [n,m]  share of flow to the facet's first neighbour       */
    PYDEM_UCA = 6,         /* float64 [n,m]  upstream contributing area, NaN on flats           */
    PYDEM_TWI = 7,         /* float64 [n,m]  ln(uca / (mag + min_slope)) (un-scaled)            */
    PYDEM_EDGE_TODO = 8,   /* uint8   [n,m]  inlet edge cells still waiting for a neighbour     */
    PYDEM_EDGE_DONE = 9,   /* uint8   [n,m]                                                    */
    PYDEM_WEIGHT = 10,     /* float64 [n,m]  per-cell weight of pydem_uca_weighted (upload; the call consumes it) */
    PYDEM_UCA_WEIGHTED = 11, /* float64 [n,m]  weighted upstream accumulation, NaN on flats     */
    PYDEM_FIELD_COUNT = 12
};

/* element types accepted by pydem_tile_upload for PYDEM_ELEV (held as float64 on the device; a PYDEM_F32 elevation
 * keeps the reference's float32 subtraction of elevations, dem_processing.py:1958-1962 / :1361) */
enum pydem_dtype { PYDEM_F64 = 0, PYDEM_F32 = 1, PYDEM_I16 = 2, PYDEM_I32 = 3, PYDEM_U8 = 4, PYDEM_I8 = 5 };

/* options of the hot path; names and defaults follow the DEMProcessor traits
 * (pydem/dem_processing.py:105-154) */
typedef struct pydem_options {
    int32_t drain_pits;              /* 1   :112 */
    int32_t drain_pits_min_border;   /* 0   :114 */
    int32_t drain_pits_max_iter;     /* 300 :117 */
    int32_t drain_pits_max_dist;     /* 32  :118 (0 = None) */
    double  drain_pits_max_dist_XY;  /* NaN = None :119 */
    int32_t apply_uca_limit_edges;   /* 0   :123 */
    int32_t apply_twi_limits;        /* 0   :125 */
    int32_t apply_twi_limits_on_uca; /* 0   :127 */
    int32_t circular_ref_maxcount;   /* 50  :151 */
    double  uca_saturation_limit;    /* 32  :146 */
    double  twi_min_slope;           /* 1e-3 :147 */
    double  twi_min_area;            /* +inf :148 (in/out: min(dX2*dY2) is folded in by pydem_uca) */
} pydem_options;

/* per-stage device time of the last call of each stage, milliseconds (hipEvent pairs) */
typedef struct pydem_timings {
    double slopes_directions_ms;  /* stencil + perimeter                      */
    double stencil_kernel_ms;     /* the interior 3x3 stencil kernel alone    */
    double flats_ms;              /* flats-edge labelling                     */
    double graph_ms;              /* section/proportion + pits + in-degree    */
    double pits_ms;               /* pit -> drain assignment alone            */
    double sweep_ms;              /* frontier sweep                           */
    double twi_ms;
    int64_t sweep_rounds;         /* frontier rounds of the last sweep        */
    int64_t sweep_kernel_launches;
    int64_t n_flats;              /* cells in the flats mask after slopes_directions */
    int64_t n_pit_edges;          /* pit -> drain edges built                  */
    int64_t n_pits_undrained;     /* the reference's "pits had no place to drain" count */
    int64_t n_unresolved;         /* cells still unfinished after the re-seed loop (circular drainage, dem_processing.py:951-964) */
    int64_t sweep_tile_passes;    /* LDS tile-local passes run before the queue rounds */
    int64_t n_pits;               /* pit candidates of the last pit search (all of them enter the lane pass)              */
    int64_t n_pits_row;           /* ... that entered the row pass (16 lanes per pit; 0: pass not run, PYDEM_PITS_ROW=0)  */
    int64_t n_pits_wave;          /* ... that entered the wavefront pass (128 x 128 window)                               */
    int64_t n_pits_big;           /* ... that entered the 256 x 256 wavefront pass or the workgroup pass behind it        */
    double uca_weighted_ms;       /* last pydem_uca_weighted: seed, level re-arm and weighted sweep (the other fields keep pydem_uca's) */
} pydem_timings;

const char *pydem_hip_last_error(void);
int pydem_hip_device_count(int *count);
int pydem_hip_device_name(int device, char *buf, int buflen);
/* free / total bytes of the device's HBM (hipMemGetInfo): what a directory run sizes `tiles_in_flight` against, and the leak
 * check of the test suite (no counterpart in the reference, whose tiles live in host memory). */
int pydem_hip_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);

/* The conditioning stages (pydem_fill_flats, pydem_pit_candidates_read, pydem_pit_paths) lease one scratch arena per device
 * for the duration of a call (it grows to the largest request seen: ~6 GB + up to 17 GB for the large-window simulations
 * of a 8192 x 8192 tile); this returns every arena to the driver.  It also empties the per-device free lists on which
 * pydem_tile_destroy leaves the planes of a tile for the next tile of the same shape (PYDEM_PLANE_CACHE_GB, default 32;
 * a failing allocation empties them as well) and the pinned chunks / streams of the whole-plane transfers.  No counterpart in
 * the reference (host arrays). */
int pydem_hip_release_scratch(void);

/* PYDEM_MEM_POISON=<0..255> (read at every hand-out) fills every device block the library hands out -- planes off the free
 * lists or mapped anew, scratch blocks, the whole conditioning arena at the start of a lease -- with that byte before the
 * pointer is used: a debug mode that makes "whatever the last owner left" a known pattern.  This returns the process totals
 * of what was filled (0, 0 while the variable has never been set). */
int pydem_hip_poison_stats(int64_t *blocks, int64_t *bytes);

int pydem_tile_create(int64_t n_rows, int64_t n_cols, int device, pydem_tile **out);
int pydem_tile_destroy(pydem_tile *t);
/* dX, dY: n_rows-1 values; dX2, dY2: n_rows values (DEMProcessor.__init__ :229-258) */
int pydem_tile_set_spacing(pydem_tile *t, const double *dX, const double *dY,
                           const double *dX2, const double *dY2);
int pydem_tile_upload(pydem_tile *t, int field, const void *src, int dtype);
int pydem_tile_download(pydem_tile *t, int field, void *dst);
/* one row (axis 0, n_cols elements) or one column (axis 1, n_rows elements) of a field, in the
 * field's own element type: the strips neighbouring tiles exchange in the directory flow
 * (reference pydem/process_manager.py:131-145 and :252-255 read/write them through zarr) */
int pydem_tile_get_line(pydem_tile *t, int field, int axis, int64_t index, void *dst);
int pydem_tile_set_line(pydem_tile *t, int field, int axis, int64_t index, const void *src);
/* `count` lines at once (fields[k], axes[k], indices[k] -> dsts[k]) with a single synchronisation: what one
 * calc_uca_ec of the reference reads from its neighbours' stores (process_manager.py:246-274) */
int pydem_tile_get_lines(pydem_tile *t, int count, const int *fields, const int *axes, const int64_t *indices,
                         void *const *dsts);
int pydem_tile_synchronize(pydem_tile *t);
int pydem_tile_timings(pydem_tile *t, pydem_timings *out);
int64_t pydem_tile_device_bytes(pydem_tile *t);

/* deterministic synthetic fractal DEM written straight into the tile's elevation
 * (bit-identical to pydem_amd/synth.py:fractal; bench / test input only) */
int pydem_tile_synth_fractal(pydem_tile *t, uint32_t seed, int64_t row0, int64_t col0,
                             int n_octaves, int top_shift, double zmin, double zrange);

/* Elevation conditioning on the resident elevation (csrc/cond_device.hip): DEMProcessor.calc_fill_flats
 * (pydem/dem_processing.py:551-579: quantisation artefacts :396-426 when max_pit_area > 0, then _fill_flat :308-394 for
 * every labelled flat), or only DEMProcessor.calc_fill_pit_artifacts with artefacts_only.  The elevation stays on the
 * device (float64 after the flats step, the values of the input dtype after the artefact step alone).  *needs_host = 1
 * and an untouched tile when the tile has no-data cells: the caller uses the host implementation
 * (pydem_cond_pit_artifacts / pydem_cond_fill_flats below) for those. */
int pydem_fill_flats(pydem_tile *t, double max_pit_area, int below_sea, double source_tol, int peaks, int pits, int artefacts_only,
                     int *needs_host);
/* DEMProcessor.calc_pit_drain_paths (pydem/dem_processing.py:428-548) on the resident float64 elevation
 * (csrc/cond_paths.hip).  Three calls because the processing order is numpy's: pydem_pit_candidates finds the strict local
 * minima (:444-449; *npits = -1 when the tile has no-data cells), pydem_pit_candidates_read returns their cells
 * (ascending) and elevations, the caller sorts them with np.argsort like the reference (:450-452 -- the tie order of
 * that call is part of the result) and pydem_pit_paths carves the paths in that order.  *needs_host = 1 (surface
 * restored) when the order-preserving parallel schedule had to give up; the host loop pydem_cond_pit_paths takes over. */
int pydem_pit_candidates(pydem_tile *t, int below_sea, int64_t *npits);
int pydem_pit_candidates_read(pydem_tile *t, int64_t npits, int32_t *cells, double *elev);
int pydem_pit_paths(pydem_tile *t, const int32_t *order, int64_t npits, int max_iter, int max_dist, double max_dist_XY,
                    int64_t *n_failed, int64_t *iter_used, int64_t *rounds, int *needs_host);
/* Depression filling on the resident float64 elevation z (csrc/fill_depressions.hip): TauDEM's PitRemove, Planchon & Darboux 2001,
 * priority-flood + epsilon (Barnes et al. 2014); no reference method.  The other two conditioning stages leave every depression
 * wider than their reach a sink; this one leaves none.  NaN is no data; a +-inf in z is refused (-2).  A cell is OPEN when
 *     its elevation is finite and it lies on the tile's border (row 0, row n-1, column 0, column m-1), or
 *     its elevation is finite and one of its 8 neighbours is NaN (no data is "outside", as in pydem_dist_up's edge rule), or
 *     the caller marks it in `outlets` (uint8 [n,m] on the host, may be NULL): known sinks that must stay (TauDEM's depression mask).
 * The filled surface W is
 *     W[c] = NaN                                                      where z[c] is NaN,
 *     W[c] = z[c]                                                     on open cells,
 *     W[c] = max(z[c], min over the finite 8-neighbours v of (W[v] + eps))    on every other cell
 * (a plain fp64 add, a plain compare that keeps z[c] unless the sum is greater, the same eps for all eight neighbours), and of the
 * solutions of that recursion the GREATEST: what relaxing downward from +inf and a priority flood from the open cells both compute.
 * The recursion is monotone in W, in floating point too, so the result does not depend on the order of the relaxation: it is
 * compared bit for bit with a heap-ordered flood on the host (pydem_amd/conditioning.py: fill_depressions).  With eps == 0 this is
 * the classic fill: lakes become flats and every value of W is a value of z.  With eps > 0 every cell that is not open has a
 * neighbour lower by at least eps, so no interior pit or flat remains -- and flat areas that are NOT depressions get the same
 * gradient of eps per step toward the open cells.
 *   *epsilon (in/out): a finite value >= 0 is used as given; < 0 is automatic, 2^-32 times the smallest power of two >= max |z| over
 *   the finite cells (1.0 if that maximum is 0); the value used is written back.  -2 for a non-finite value and for an eps > 0 with
 *   amax + eps == amax (amax = max |z|): it would vanish at the surface's magnitude.
 *   depth (float64 [n,m] on the host, may be NULL): W - z, exact, NaN where z is NaN.  *n_raised: cells with W > z.  *max_depth:
 *   the largest W - z.  *passes: full passes over the grid of 32 x 32 blocks, the last one, which changed nothing, included.
 *   *ms: device time (a hipEvent pair).
 * The call replaces the resident elevation by W and, like the other conditioning stages, invalidates the flow graph and every
 * field computed from the elevation (PYDEM_MAG onward).  With eps > 0 the elevation counts as float64 from then on; with eps == 0
 * it keeps the dtype of its upload (its values are still values of that dtype).  Scratch comes from the conditioning arena:
 * pydem_tile_device_bytes is what it was before.  -2 (bad arguments, checked before the surface is touched); -5 when
 * PYDEM_FILL_MAX_PASSES passes (default 100000, read per call) did not reach the fixed point: W lives in scratch until the end,
 * so the elevation is then exactly what it was.  PYDEM_FILL_LOCAL=0 (read per call): a block visit makes one relaxation step
 * instead of iterating to its local fixed point -- the same result by another schedule, for the tests.  Per tile: a depression
 * cut by the tile's border drains off the tile (pydem_fill_seam_* below fills across tiles). */
int pydem_fill_depressions(pydem_tile *t, double *epsilon, const uint8_t *outlets, double *depth, int64_t *n_raised, double *max_depth,
                           int64_t *passes, double *ms);
/* The same fill ACROSS tiles (csrc/fill_depressions.hip): a session of four calls on a tile, driven from outside so that the tiles
 * of a mosaic end at the fill of the whole mosaic, bit for bit (pydem_amd/process_manager.py: process_fill_depressions; the host
 * twin is pydem_amd/conditioning.py: SeamFill).  The tiles are windows of one pixel lattice and neighbouring tiles share at least
 * one line.  A border cell of a tile is a SEAM cell when all 8 of its lattice neighbours are held by some tile; the caller says
 * which are.  A seam cell is not open by position (it stays open beside no data and where `outlets` marks it); every other border
 * cell is open as in pydem_fill_depressions.  The session computes the greatest solution of
 *     W[c] = z[c]                                                                        on open cells,
 *     W[c] = max(z[c], min(X[c], min over the in-tile finite neighbours v of (W[v] + eps)))    elsewhere,
 * where the cap X[c] is +inf except on seam cells, and there the smallest current W[c] of the OTHER tiles that hold c, taken as
 * it is (no + eps; NaN counts as +inf).  The recursion is monotone in W and in X, so W at its fixed point for caps X is a valid
 * start for any caps X' <= X: the caller exchanges lines and relaxes again until no cap falls, and every copy of a cell then
 * holds the value of the whole-mosaic fill.  Caps may only fall.  The elevation must not be replaced while a session is open.
 *   pydem_fill_seam_begin: seam_top / seam_bottom (m entries), seam_left / seam_right (n entries): uint8 on the host, nonzero = seam
 *   cell, NULL = none; a corner is a seam cell if either of its lines says so.  Holds three device blocks until the end, counted
 *   by pydem_tile_device_bytes: W (8 n m bytes), the flag words of the 32 x 32 blocks (4 ceil(n/32) ceil(m/32) bytes) and the cap
 *   lines (8 (2 m + 2 n) bytes).  W = z on open cells, +inf elsewhere, NaN kept.  *amax: max |z| over the finite cells.  -2 for
 *   +-inf in z and for a second begin without an end (nothing is held then).
 *   pydem_fill_seam_relax: cap_top / cap_bottom (m), cap_left / cap_right (n): float64 on the host, NULL = unchanged; where two
 *   lines meet at a corner the smaller value counts.  An entry above the one the session holds: -2, nothing changes.  The blocks
 *   whose caps fell are flagged (all blocks on the first call) and the pass loop of pydem_fill_depressions runs to the fixed
 *   point.  eps: finite, >= 0, the same in every relax of a session, not vanishing at *amax (-2).  *n_lowered: cells whose W is
 *   lower after the call than before it (0: the tile did not move).  *passes, *ms as in pydem_fill_depressions.  Reads
 *   PYDEM_FILL_LOCAL, PYDEM_FILL_MAX_PASSES and PYDEM_FILL_CHECK_EVERY per call; -5 at the pass bound: the session stays open (W is
 *   still an upper bound, the caps are taken), the elevation is untouched.
 *   pydem_fill_seam_get_lines: rows (axes[k] == 0, m doubles) and columns (axes[k] == 1, n doubles) of W at indices[k] (negative: from
 *   the end) into dsts[k], with one synchronisation.  A neighbour that shares `overlap` lines needs line overlap - 1, not only line 0.
 *   pydem_fill_seam_end: commit != 0: -5 while W still holds +inf (the session stays open); otherwise elev = W with depth, *n_raised,
 *   *max_depth, the dtype rule and the invalidations of pydem_fill_depressions.  commit == 0: the elevation and everything computed
 *   from it stay bit for bit what they were.  Either way the three blocks go back and pydem_tile_device_bytes is what it was before
 *   begin.  pydem_tile_destroy with an open session frees it.  -2 without an open session.
 * THE INVENTORY ACROSS TILES (csrc/depressions.hip; pydem_amd/process_manager.py: process_depressions; host twin: SeamFill.label /
 * id_lines / inventory / labels).  Once no cap falls at eps = 0 the session's W is the tile's window of the whole-mosaic classic
 * fill, and five more calls of the session give the tile's part of pydem_depressions of the whole mosaic.  They read z and W and
 * change nothing of the tile; the session is then ended with commit == 0.
 *   pydem_fill_seam_label: the 8-connected components of W > z INSIDE the tile, numbered 1 .. *n_local in ascending order of their
 *   smallest linear index r*m + c, with the union-find of pydem_depressions (PYDEM_DEPR_LOCAL as there).  The plane of local ids
 *   (int32: 0 not raised, -1 no data) stays on the device as a fourth session block of 4 n m bytes, counted by
 *   pydem_tile_device_bytes from this call until pydem_fill_seam_end.  *max_depth: the largest W - z of the tile.  -5 while W holds
 *   +inf.  *ms: device-clock time of the call (also in _inventory and _labels).
 *   pydem_fill_seam_label_roots: roots[k], levels[k] (count == *n_local entries): the smallest linear index of local component
 *   k + 1, and its level W there.
 *   pydem_fill_seam_get_id_lines: as pydem_fill_seam_get_lines, for rows and columns of the id plane (int32).
 *   pydem_fill_seam_inventory: the tile's PARTIAL TABLE.  The caller has joined the local components of all tiles into the
 *   mosaic's depressions and numbered those this tile can meet 1 .. n_rows.  lut (int32, *n_local + 1 entries, lut[0] unused):
 *   local id -> row.  owner (uint8 [n,m]): nonzero where this tile is the one that counts the lattice cell; every lattice cell has
 *   one owner.  halo_ids, halo_W (2 m + 2 n + 4 entries): the ring just outside the window -- the row above over columns -1 .. m,
 *   the row below over the same columns, the column left over rows 0 .. n-1, the column right -- as the row of the depression the
 *   cell lies in (0: finite and not raised, -1: no data or held by no tile) and its W.  row_area (n doubles), shift_area,
 *   shift_volume: the terms and the fixed-point shifts of area and volume (a cell adds llrint(ldexp(p, shift)), as in
 *   pydem_depressions; the caller derives the shifts from the whole mosaic).  outlets as in pydem_fill_seam_begin, may be NULL.
 *   table: 13 columns of n_rows uint64 words, column-major: cells, r0, r1, c0, c1 (local, over the owned raised cells of the row),
 *   the order-preserving pattern of their lowest z, the smallest local index among the owned cells at that z, the smallest local
 *   index among the owned sill cells, their number, 1 when one of them is open, the two fixed-point sums, the bits of z at the
 *   bottom cell.  An owned finite cell that is not raised is a sill cell of every row whose level equals its z among its 8
 *   neighbours, in the window or in the halo, once per row; it is open when a neighbour is -1 or `outlets` marks it.  A row
 *   without owned cells keeps ~0 in the minimum columns and 0 elsewhere.  -2 for a lookup or halo entry outside 0 (-1) .. n_rows.
 *   pydem_fill_seam_labels: label (int32 [n,m] on the host) = lut[local id] on raised cells, 0 and -1 as in the id plane.
 * Limits: one pixel size, overlap >= 1, one process. */
int pydem_fill_seam_begin(pydem_tile *t, const uint8_t *outlets, const uint8_t *seam_top, const uint8_t *seam_bottom,
                          const uint8_t *seam_left, const uint8_t *seam_right, double *amax);
int pydem_fill_seam_relax(pydem_tile *t, double eps, const double *cap_top, const double *cap_bottom, const double *cap_left,
                          const double *cap_right, int64_t *n_lowered, int64_t *passes, double *ms);
int pydem_fill_seam_get_lines(pydem_tile *t, int count, const int *axes, const int64_t *indices, void *const *dsts);
int pydem_fill_seam_end(pydem_tile *t, int commit, double *depth, int64_t *n_raised, double *max_depth);
int pydem_fill_seam_label(pydem_tile *t, int64_t *n_local, double *max_depth, double *ms);
int pydem_fill_seam_label_roots(pydem_tile *t, int64_t count, int32_t *roots, double *levels);
int pydem_fill_seam_get_id_lines(pydem_tile *t, int count, const int *axes, const int64_t *indices, void *const *dsts);
int pydem_fill_seam_inventory(pydem_tile *t, const int32_t *lut, int64_t n_rows, const uint8_t *owner, const uint8_t *outlets,
                              const int32_t *halo_ids, const double *halo_W, const double *row_area, int shift_area, int shift_volume,
                              uint64_t *table, double *ms);
int pydem_fill_seam_labels(pydem_tile *t, const int32_t *lut, int32_t *label, double *ms);
/* The depression inventory of the resident float64 elevation z (csrc/depressions.hip): which closed depressions there are, and for
 * each where it is, how large, how deep, what volume, where it spills and where its bottom lies; no reference method.
 * DEFINITION.  W is the classic fill of z: pydem_fill_depressions with eps = 0, the same open cells (border, beside no data, the
 * caller's `outlets`: uint8 [n,m] on the host, may be NULL).  W lives in the conditioning arena: the call changes NEITHER the
 * elevation NOR its dtype, the flow graph or any field computed from z, and pydem_tile_device_bytes is what it was before.  A
 * depression is an 8-connected component of the cells with W > z.  With eps = 0 two adjacent raised cells have the same W, so a
 * component has ONE level, its spill elevation S, and at least one sill cell: a finite cell that is not raised, is 8-adjacent to
 * the component and has W == z == S.  Depressions are numbered 1..K in ascending order of their smallest linear cell index
 * r*m + c.  Every value below follows from z, `outlets` and the spacing alone: the device code uses integers only (indices,
 * counts, order-preserving bit patterns of doubles, fixed-point sums), so every schedule gives the same bits, and the host twin
 * (pydem_amd/conditioning.py: label_depressions) is compared with array_equal.
 * LABELS (int32 [n,m] on the host, may be NULL): the number of the kept depression a cell belongs to, 0 where no depression is
 * kept, -1 where z is NaN.
 * TABLE, one pydem_depression per kept depression, read with pydem_depressions_table after the call:
 *   cells                  its cells
 *   r0, r1, c0, c1         its bounding box (inclusive)
 *   spill_elev             S (a copy of a value of z)
 *   bottom, bottom_elev    the smallest linear index among its cells of lowest z (-0.0 and 0.0 are equal), and that cell's z
 *   max_depth              spill_elev - bottom_elev, one fp64 subtraction
 *   pour, n_sills          the smallest linear index among its sill cells, and their number (a sill cell counts once per
 *                          depression, however many of its cells it touches)
 *   open_sill              1 when a sill cell is an open cell: the lake spills straight off the tile, into no data or into an
 *                          outlet, so the tile may have cut it
 *   area, volume           sums over its cells of p = row_area[r] (= dX2[r] * dY2[r]) and of p = fl((W - z) * row_area[r]), in FIXED
 *                          POINT: with E from frexp of the largest term possible (max row_area; fl(largest W - z of the tile * max
 *                          row_area)), B = min(40, 62 - ceil(log2(max(n*m, 2)))) fraction bits and the quantum q = 2^(E - B), a cell
 *                          adds llrint(p / q) (ties to even) to an int64 with an integer atomic, and the column is (double)sum * q.
 *                          One result whatever the order, and |column - sum of p| <= cells * q / 2.  quanta[0], quanta[1]: the
 *                          quanta of area and volume.
 * FILTERS: a depression with max_depth < min_depth, cells < min_cells or volume < min_volume is dropped from the table and its
 * label becomes 0; the survivors are renumbered 1..K' in the same order (0, 1, 0 keep everything).  The host decides this from the
 * full table.  *n_found = K, *n_kept = K'.
 * *passes: passes of the relaxation.  ms (9 doubles, may be NULL): device-clock time (hipEvent pairs) of the call and of its parts:
 * relaxation, marking the raised cells + block-local labelling, seam merge, flatten, numbering (scan, ids), statistics, table
 * (its download, the host's filter, the upload of the lookup: mostly host time), label write.
 * ERRORS: -2 bad arguments (a negative or NaN filter) and +-inf in z, before any result exists; -3 without a spacing
 * (pydem_tile_set_spacing); -5 from the fill's pass bound (PYDEM_FILL_MAX_PASSES) and for a table that contradicts the definition;
 * -6 when the device cannot hold the table of K depressions (K can reach (n/2)(m/2)): nothing is returned, never a truncated
 * table.  PYDEM_DEPR_LOCAL=0 (read per call): no block-local labelling, every raised cell starts as its own root and every union
 * goes through the global merge -- the same result by another schedule, for the tests; PYDEM_FILL_LOCAL=0 does the same to the
 * relaxation.  Per tile: a depression cut by the tile's border is open there; the nested hierarchy of depressions is not
 * computed. */
typedef struct pydem_depression {
    int64_t cells, r0, r1, c0, c1, bottom, pour, n_sills, open_sill;
    double spill_elev, bottom_elev, max_depth, area, volume;
} pydem_depression;
int pydem_depressions(pydem_tile *t, const uint8_t *outlets, double min_depth, int64_t min_cells, double min_volume, int32_t *label,
                      int64_t *n_found, int64_t *n_kept, double *quanta, int64_t *passes, double *ms);
/* The table of the last pydem_depressions on this tile: `rows` must be its *n_kept (-2 otherwise). */
int pydem_depressions_table(pydem_tile *t, int64_t rows, pydem_depression *table);
/* The HAND hydraulic table: per zone (a reach's catchment) and per water stage, the cells, the flooded area, the area-weighted
 * HAND and the wetted bed area of a HAND plane -- what a synthetic rating curve is made of; no reference method.
 * INPUTS.  The tile's spacing and the resident PYDEM_MAG (-3 without either).  zone: host int32 [n,m]; 1..K are zones, anything
 * < 1 is skipped, a value > K is an error (-2).  hand: host float64 [n,m], or NULL: the result plane of the last pydem_dist_down
 * as it stands on the device (RESIDENT HAND below).  stages: host float64 [S], finite, strictly ascending, 1 <= S <= 1024 (-2
 * otherwise).  K = n_zones >= 0.
 * DEFINITION.  Row r has the cell area a = dX2[r] * dY2[r], one multiply.  A cell c of zone k with h = hand[c]:
 *   h is NaN                      adds 1 to nan[k];
 *   h > stages[S-1] (+inf too)    adds 1 to above[k];
 *   otherwise it is COUNTED in bin b = the number of stages < h (np.searchsorted(stages, h, 'left'): h == stages[j] lies in bin j,
 *                                 -0.0 == 0.0; a negative h is allowed and lies in bin 0 when h <= stages[0]).
 * A counted cell adds to the four int64 words of (k, b):  1;  llrint(ldexp(p, shift)) for p_a = a;  the same for p_m = fl(a * h)
 * (signed);  the same for p_b = fl(a * sqrt(fl(1 + fl(mag*mag)))) with the correctly rounded square root and mag = PYDEM_MAG[c]
 * (a non-finite mag counts as slope 0: p_b = a).  The three shifts are those of pydem_depressions: with E from frexp of the
 * largest term -- max p_a, max |p_m|, max p_b over the counted cells, 0 when there are none -- and B = min(40, 62 -
 * ceil(log2(max(n*m, 2)))) fraction bits, shift = B - E and the quantum is q = 2^(E - B).  A first kernel finds the three maxima
 * with integer atomicMax on the bit patterns of the magnitudes; the host forms the shifts.  Integers only from there on: every
 * schedule gives the same bits, the host twin (pydem_amd/hydraulics.py: hand_table_ref) is compared with array_equal, and per
 * word |word * q - sum of p| <= cells * q / 2.  A term that is not finite (h = -inf, an overflowing slope) is refused: -2.
 * OUTPUTS (host).  table: int64 [K, S, 4]: cells, area, area x HAND, bed area of (zone, bin) -- per bin, NOT cumulated over the
 * stages.  skipped: int64 [K, 2]: nan, above.  quanta[3]: q_a, q_m, q_b.  ms[3] (may be NULL): device time (hipEvent pairs) of
 * the two kernels together, of the maxima, of the sums (the table's memset included).
 * MEMORY.  The table and the uploaded planes are leased from the conditioning arena; nothing stays with the tile, and
 * pydem_tile_device_bytes is what it was before.  -6 with a message, before any kernel runs, when the device cannot hold the
 * K * S * 4 + K * 2 words of the table.
 * RESIDENT HAND (hand == NULL).  The tile carries a tag that says its result plane holds a finished pydem_dist_down: set at the
 * successful end of pydem_dist_down alone; cleared when any sweep that shares that plane (pydem_dist_down / _dist_up / _rev_accum /
 * _fwd_accum / _stream_network / _tree_accum) takes it, and wherever the flow graph is invalidated (an upload of elevation, slope,
 * direction or flats, a conditioning stage, pydem_slopes_directions ...).  -3 when the tag is not set.  The plane is only read.
 * Both ways give the same bytes.
 * PYDEM_HANDTAB_LOCAL=0 (read once per process): no reduction across the wavefront, every lane issues its own atomics -- the
 * same result by another schedule, for the tests.  Writes no field, flag or timing of the tile. */
int pydem_hand_table(pydem_tile *t, const int32_t *zone /* [n,m] host */, const double *hand /* [n,m] host, or NULL */,
                     const double *stages /* [n_stages] host */, int64_t n_stages, int64_t n_zones, int64_t *table /* [K,S,4] host */,
                     int64_t *skipped /* [K,2] host */, double *quanta /* [3] */, double *ms /* [3] */);
/* Terrain attributes of the resident float64 elevation at a chosen scale: the least-squares quadratic over the (2k+1)^2 window of
 * every cell (Evans 1980 at k = 1, Wood 1996 above) and what follows from its five derivatives; no reference method.  PYDEM_MAG /
 * PYDEM_DIRECTION are the steepest of eight triangular facets, not the gradient of the surface; these planes are, and the second
 * derivatives exist nowhere else.  Apart from one atan2 every plane is a fixed sequence of + - * / sqrt, every one of them correctly
 * rounded and none contracted, so the host twin (pydem_amd/terrain.py: terrain_attributes_ref) gives the same bits.
 * DEFINITION, for the cell (r, c) and the half width k.  N = 2k + 1.  Z(j, i) = elev[r + j, c + i] for row offsets j and column
 * offsets i in -k .. k.  gx = dX2[r], gy = dY2[r]: the centre row's cell size, taken as constant over the window (an approximation
 * on geographic tiles).  x points east (increasing column), y north (decreasing row).
 *   Row moments, for each j, each sum started at 0.0 and added in ascending i:
 *     R0_j = sum Z(j, i);   R1_j = sum (double)i * Z(j, i);   R2_j = sum (double)(i*i) * Z(j, i).
 *   Window moments, each sum started at 0.0 and added in ascending j:
 *     M00 = sum R0_j;  M10 = sum R1_j;  M20 = sum R2_j;  M01 = sum (double)j * R0_j;  M02 = sum (double)(j*j) * R0_j;  M11 = sum (double)j * R1_j.
 *   (A running sum over a sliding window gives other bits and is not the contract.)
 *   Constants, exact integers held as doubles:  S2 = k(k+1)(2k+1)/3;  S4 = k(k+1)(2k+1)(3k^2+3k-1)/15;  D1 = N * S2;
 *     D2 = N * S4 - S2 * S2;  D11 = S2 * S2.
 *   The fit in index units:  d = M10 / D1;  e = M01 / D1;  cxy = M11 / D11;  h = (S2 * M00) / N;  a = (M20 - h) / D2;  b = (M02 - h) / D2.
 *   Ground units:  p = d / gx;  q = -(e / gy);  r = (2 * a) / (gx * gx);  t = (2 * b) / (gy * gy);  s = -(cxy / (gx * gy)).
 *   g2 = p*p + q*q;  w = 1.0 + g2;  pq2 = 2 * (p*q);  A = ((p*p)*r + pq2*s) + (q*q)*t;  B = ((q*q)*r - pq2*s) + (p*p)*t.
 * PLANES (enum pydem_terrain_attr).  Signs follow Florinsky / Shary: positive is convex (ridges, noses, shoulders), negative concave.
 *   DZDX, DZDY    p, q
 *   GRADIENT      sqrt(g2): rise over run, the unit of PYDEM_MAG
 *   ASPECT        the azimuth of the downslope direction, clockwise from north, radians: atan2(-p, -q), plus 2 pi (the double
 *                 6.283185307179586) when negative; -1 where g2 == 0, as PYDEM_DIRECTION on flats
 *   PROFILE       -A / (g2 * (w * sqrt(w)));  0 where g2 == 0
 *   PLAN          -B / (g2 * sqrt(g2)), the contour curvature;  0 where g2 == 0
 *   TANGENTIAL    -B / (g2 * sqrt(w));  0 where g2 == 0
 *   MEAN          -(((1 + q*q)*r - pq2*s) + (1 + p*p)*t) / (2 * (w * sqrt(w)))
 *   HILLSHADE     with zp = z_factor * p, zq = z_factor * q and the unit vector to the sun light = (Le, Ln, Lu) (east, north, up):
 *                 v = ((Lu - zp*Le) - zq*Ln) / sqrt(1 + (zp*zp + zq*zq));  v where v > 0, else 0
 * UNDEFINED CELLS.  A cell is defined when its window lies inside the tile and M00 is not NaN, i.e. the window holds no NaN
 * elevation (+-inf is not no data: it goes through the arithmetic).  Every requested plane is NaN (0x7ff8000000000000) at a cell
 * that is not defined; a tile smaller than the window is all NaN, which is no error.  *n_defined: the defined cells -- on finite
 * elevations the cells that are not NaN -- counted with an integer reduction across the wavefront and integer atomics.
 * ARGUMENTS.  half_width = k, 1 .. 7.  outs: PYDEM_TA_COUNT host planes [n,m] of float64, NULL = not wanted: only the planes
 * asked for are computed, stored and downloaded.  light: three doubles, may be NULL unless outs[PYDEM_TA_HILLSHADE] is set;
 * z_factor: finite, > 0.  *ms: device time of the kernel (a hipEvent pair).  -2 (before any launch) for half_width outside 1 .. 7,
 * no plane asked for, a hillshade without light and a z_factor that is not finite or not > 0; -3 without a spacing or an elevation.
 * KERNELS (csrc/terrain.hip).  k = 1 marches rows in registers, one lane per column, as the D-infinity stencil does.  k >= 2
 * stages a block of 30 rows x (64 + 2k) columns with its halo in LDS, forms R0 / R1 / R2 once per staged row and combines them
 * vertically, one lane per cell.  The cap k <= 7 (a window of 15) is that path's LDS budget: 30 rows x ((64 + 2k) + 3 x 64)
 * doubles = 64 800 bytes at k = 7, so that two workgroups share the 160 KiB of a CU and 16 of the 30 staged rows are output
 * rows.  Both paths keep the operand order above and give the same bits at k = 1; PYDEM_TA_GENERIC=1 (read per call) sends k = 1
 * through the general path, for the tests.
 * MEMORY.  The planes of a call and its counter are one device block of the tile (8192 bytes + 8 n m bytes per requested plane), grown
 * to the largest request so far, counted by pydem_tile_device_bytes and freed with the tile.  Reads the elevation and dX2 / dY2;
 * needs no slope, flats or flow graph.  Writes no field of the tile, no timing and no state of any other analysis. */
enum pydem_terrain_attr {
    PYDEM_TA_DZDX = 0, PYDEM_TA_DZDY = 1, PYDEM_TA_GRADIENT = 2, PYDEM_TA_ASPECT = 3, PYDEM_TA_PROFILE = 4, PYDEM_TA_PLAN = 5,
    PYDEM_TA_TANGENTIAL = 6, PYDEM_TA_MEAN = 7, PYDEM_TA_HILLSHADE = 8, PYDEM_TA_COUNT = 9
};
int pydem_terrain_attributes(pydem_tile *t, int half_width /* k, 1..7 */,
                             const double *light /* Le, Ln, Lu; may be NULL when no hillshade is asked */, double z_factor,
                             double *const *outs /* PYDEM_TA_COUNT host planes [n,m]; NULL = not wanted */, double *ms,
                             int64_t *n_defined);
/* Horizon and sky-view factor of the resident float64 elevation: what the terrain around a cell hides from it; no reference method.
 * pydem_terrain_attributes describes the surface inside a window of at most 15 cells; this call looks along rays of up to 1024 cells.
 * A horizon tangent is the maximum of a fixed set of products and the sky-view factor a fixed sequence of * + /, none contracted and
 * the division correctly rounded, so the host twin (pydem_amd/horizon.py: horizon_ref) gives the same bits.
 * RAY TABLE, built on the host (pydem_amd/horizon.py: ray_table) so that the device and the twin read the same integers and doubles.
 * One cell size gx x gy holds for the whole call (the caller takes dX2 / dY2 of the tile's middle row: exact on projected tiles, an
 * approximation on geographic ones).  Direction d = 0 .. n_dir - 1 has the azimuth a_d = azimuth0 + d * 360 / n_dir degrees
 * clockwise from north; rows grow to the south, columns to the east.  Its ground direction (sin a, cos a) (east, north) becomes the
 * index-space direction (sc, sr) = (sin a / gx, -cos a / gy), scaled so that max(|sr|, |sc|) == 1.  Step k = 1, 2, ... samples the
 * cell (dr_k, dc_k) = (round(k * sr), round(k * sc)), halves rounded away from zero, at the distance of that cell's centre,
 * dist_k = sqrt((dc_k * gx)^2 + (dr_k * gy)^2); steps are kept while dist_k <= max_dist, at most 1024 per direction, and
 * w_k = z_factor / dist_k.  start[n_dir + 1] (int32, start[0] == 0): direction d owns the steps start[d] .. start[d + 1] - 1 of
 * dr, dc (int16) and w (float64).  A direction without a step is legal; its tangent is 0.
 * DEFINITION, for a cell (r, c) with z0 = elev[r, c] not NaN, and a direction d:
 *     T_d = 0.0
 *     for every step k of d whose sample (r + dr_k, c + dc_k) lies inside the tile:
 *         v = (elev[r + dr_k, c + dc_k] - z0) * w_k         one subtraction, one multiplication
 *         if v > T_d: T_d = v                               a NaN sample compares false: no data does not obstruct
 *   T_d >= 0 is the tangent of the horizon's elevation angle; the horizon is never below the horizontal.  The set of v is fixed by
 *   the table, so every sample order gives the same bits.  A cell with NaN elevation is NaN (0x7ff8000000000000) in every plane.
 *   With edge_nan, T_d is NaN wherever any sample of d's steps falls outside the tile: a finite value is a complete one.  Without,
 *   samples off the tile are skipped.
 *   svf = (sum over d of 1.0 / (1.0 + T_d * T_d)) / (double)n_dir, the sum started at 0.0 and added in ascending d: the mean of
 *   cos^2 of the horizon angle, NaN if any T_d is NaN.
 *   *n_defined: the cells with a finite svf; when no svf is asked for, the cells whose T_d are all finite.  Counted with an integer
 *   reduction across the wavefront and integer atomics spread over 64 words.
 * ARGUMENTS.  n_dir 1 .. 64.  horizon: n_dir host planes [n,m] of float64 (the tangents), or NULL; svf: a host plane [n,m], or
 * NULL; only what is asked for is downloaded.  *ms: device time of the kernels (a hipEvent pair).  -2 (before anything is
 * allocated, launched or written) for n_dir outside 1 .. 64, a missing table array, neither horizon nor svf, a NULL among the
 * horizon planes, start[0] != 0, a direction with fewer than 0 or more than 1024 steps, a weight that is not finite, not > 0 or above
 * the one before it in its direction, and a segment (at most 32 consecutive steps of a direction) whose row or column offsets span more than 32 cells
 * (no ray does: an offset moves by at most one cell per step); -3 without a spacing or an elevation.
 * KERNEL (csrc/horizon.hip).  A workgroup of four wavefronts owns 32 rows x 64 columns, a lane per column and eight rows per lane,
 * with z0, T_d and the svf sum in registers.  It walks a ray in segments of at most 32 steps: the source region of a segment --
 * the block shifted by the segment's offsets, at most 64 x 96 doubles (49 664 bytes of LDS), cells off the tile as NaN -- is staged in LDS,
 * and every lane takes its samples from there.  A launch takes consecutive directions of at most 512 steps in all (one direction at
 * least); the svf sum passes from launch to launch through its plane, in ascending d on one stream, so the additions keep their
 * order.
 * MEMORY.  One device block of the tile: 8192 bytes, the table (16 bytes per step, a segment's steps padded to a multiple of 4, and 32 per segment and direction, each part
 * rounded up to 256), 8 n m bytes for the svf sum (held whether svf is asked for or not) and 8 n m bytes per direction when the
 * horizon planes are asked for; grown to the largest request so far, counted by pydem_tile_device_bytes and freed with the tile.
 * Reads the elevation; needs no slope, flats or flow graph.  Writes no field of the tile, no timing and no state of any other
 * analysis. */
int pydem_horizon(pydem_tile *t, int n_dir /* 1..64 */, const int32_t *start /* [n_dir+1] */, const int16_t *dr, const int16_t *dc,
                  const double *w /* [start[n_dir]] each */, int edge_nan, double *const *horizon /* n_dir host planes [n,m], or NULL */,
                  double *svf /* host plane [n,m], or NULL */, double *ms, int64_t *n_defined);
int pydem_slopes_directions(pydem_tile *t);
int pydem_find_flats(pydem_tile *t);
/* What the tile knows about its flats mask against its slopes, and what the pydem_find_flats calls on it have launched so far
 * (the call only does the work its result needs; PYDEM_STEP_LEAN=0: always the full pass).  *state: 0 nothing known, 1 flats ==
 * (mag == -1) everywhere, 2 as 1 except at the pits pydem_tile_restore_pit_slopes has just restored.  counts[3]: calls that ran
 * the full pass over the tile, calls that only set the restored pits, calls that had nothing to do.  Either pointer may be NULL. */
int pydem_tile_flats_state(pydem_tile *t, int *state, int64_t *counts);
int pydem_uca(pydem_tile *t, pydem_options *opt);
/* Weighted flow accumulation: the sweep of pydem_uca over the same flow graph (pit -> drain edges, the on-edge skip and
 * the circular-drainage re-seed loop included) started from a per-cell seed instead of the cell area --
 *     W[c] = seed[c] + sum over in-edges u -> c of W[u] * factor(u -> c),   seed = w * dX2 * dY2 (scale_by_cell_area) or w,
 * NaN on flats -- i.e. DEMProcessor._calc_uca_chunk (pydem/dem_processing.py:883-972) and cyutils._drain_area
 * (pydem/cyfuncs/cyutils.pyx:78-187) with their initial area array (:885, :901) replaced, as AreaDinf with a weight grid
 * does.  Weights: PYDEM_WEIGHT, uploaded before every call (any finite value, zero and negative included; the call scales
 * the plane in place and consumes it); result: PYDEM_UCA_WEIGHTED.  With w = 1 the result is pydem_uca's uca bit for bit.
 * The flow graph is the tile's when the last graph stage ran with the same graph options as `opt` (drain_pits, _min_border,
 * _max_iter, _max_dist, _max_dist_XY); otherwise the call runs the graph stage of pydem_uca itself and does not keep the graph:
 * mag / flats are put back as they were (the pit patch undone; a temporary 12 bytes per flat cell), and so are section,
 * proportion and edge_todo when the tile holds them (a temporary copy, 10 bytes per cell); only the pit-edge list
 * (pydem_tile_pit_edges) is then that of the graph built here.  No edge masks, twi_min_area is not
 * touched; uca, every other field and all of pydem_uca's timings (the graph stage's included) stay as they were, the next
 * edge round rebuilds its work state.  uca_weighted_ms: seed, level re-arm and weighted sweep, not the graph stage. */
int pydem_uca_weighted(pydem_tile *t, pydem_options *opt, int scale_by_cell_area);
/* Downslope distance to a target set along the D-infinity flow paths, and with kind = 1, stat = 0 the height above the nearest
 * drainage (HAND): a reverse (outlet-to-source) sweep over the flow graph pydem_uca sweeps forward (TauDEM's DinfDistDown next
 * to its AreaDinf; no reference method).  The out-edges of a cell c are the edges of column c of the adjacency matrix of
 * _mk_adjacency_matrix (pydem/dem_processing.py:1072-1153): the regular edges that survive the keep-filter (:1136-1137), of
 * weights p and 1 - p, and the pit -> drain edges with theirs.  With T the target set,
 *     D[c] = 0                      where T[c];
 *     D[c] = NaN                    otherwise, when c has no out-edge (undrained pits, flats without a drain, cells whose flow
 *                                   only leaves the tile);
 *     otherwise, with t_e = D[v_e] + cost(c, v_e) over the out-edges e = c -> v_e of weight w_e,
 *       stat 0 (ave): D[c] = sum(w_e * t_e) / sum(w_e)   (normalised by the surviving weights: a dropped edge does not bias it)
 *       stat 1 (min) / 2 (max): the minimum / maximum of t_e, NaN if any t_e is NaN.
 * NaN propagates upstream in all three: a value is finite only when every flow path from the cell ends in a target inside the
 * tile (TauDEM's edge-contamination rule).  Cells on or upstream of a drainage cycle (pit edges can close one) never become
 * ready: they are NaN and counted in *n_unresolved; there is no re-seed loop.
 * cost(c, v) for c = (r, j), v = (r', j'):  kind 0 (h): hypot((j' - j) * dX2[r], (r' - r) * dY2[r]) -- the source row's cell
 * size, pit edges of any offset included; kind 1 (v): elev[c] - elev[v], signed, on the tile's float64 elevation, not clamped;
 * kind 2 (s): hypot(h, v).
 * Targets: `target`, a host mask [n,m] (non-zero = target), or, when target == NULL, uca >= uca_threshold (finite, >= 0) on the
 * tile's current uca (pending incremental edge rounds are flushed first, as a download of PYDEM_UCA does; NaN is never a
 * target).  out: [n,m] host doubles (may be NULL); *ms: device time of the sweep (hipEvent pair); *levels: dependent steps of
 * the reverse sweep (the initial level, tile passes that finished something, levels of the queue that takes the rest).  One lane finishes a cell from the final values of its out-neighbours in ascending
 * destination order (a regular edge before a pit edge to the same cell): no floating-point atomics, results identical from
 * run to run.  Needs the tile's flow graph: -3 when no pydem_uca / pydem_build_graph has run since the elevation, slope,
 * direction or flats last changed.  Writes no field of the tile, no timing and no state of the forward sweep or of the edge
 * fix-up: the result plane, a queue and the mask (13 bytes per cell) are the call's own, allocated by the first call and
 * freed with the tile. */
int pydem_dist_down(pydem_tile *t, int kind /* 0 h, 1 v, 2 s */, int stat /* 0 ave, 1 min, 2 max */,
                    const uint8_t *target /* [n,m] host, or NULL */, double uca_threshold /* used when target == NULL */,
                    double *out /* [n,m] host */, double *ms, int64_t *levels, int64_t *n_unresolved);
/* Upslope flow-path distance: the distance along the D-infinity flow paths from the divides down to each cell -- the forward
 * (divide-to-outlet) sweep of the path statistic that pydem_dist_down sweeps in reverse (TauDEM's DinfDistUp next to its
 * DinfDistDown and AreaDinf; no reference method).  stat 2 (max) is the longest flow path into the cell.  The in-edges of a
 * cell c are the edges u -> c of the adjacency matrix of _mk_adjacency_matrix (pydem/dem_processing.py:1072-1153), the matrix
 * pydem_dist_down reads: the regular edges that survive the keep-filter (:1136-1137), of weight p or 1 - p of the SOURCE u (c
 * is u's first or second facet neighbour), and the pit -> drain edges with theirs.  cost(u, c) is pydem_dist_down's cost of
 * the edge u -> c: for u = (r, j), c = (r', j'): kind 0 (h): hypot((j' - j) * dX2[r], (r' - r) * dY2[r]) -- the SOURCE row's
 * cell size, pit edges of any offset included; kind 1 (v): elev[u] - elev[c], signed, on the tile's float64 elevation, not
 * clamped; kind 2 (s): hypot(h, v).
 *     U[c] = NaN                    where the elevation of c is NaN;
 *     U[c] = 0                      where c has no in-edge (divides, and isolated cells such as undrained flats without inflow);
 *     otherwise, once every u_e is final, with t_e = U[u_e] + cost(u_e, c) over the in-edges e = u_e -> c of weight w_e,
 *       stat 0 (ave): U[c] = sum(w_e * t_e) / sum(w_e)
 *       stat 1 (min) / 2 (max): the minimum / maximum of t_e;
 *     NaN if any t_e is NaN.
 * The in-edges are taken in ascending source order, a regular edge before a pit edge from the same source, by ONE lane per
 * cell: no floating-point atomics, results identical from run to run and from schedule to schedule.
 * edge_nan != 0 is TauDEM's edge-contamination rule: a cell on the tile's border (row 0, row n - 1, column 0, column m - 1) is
 * NaN whatever its in-edges, and so is a cell with an 8-neighbour whose elevation is NaN.  NaN propagates downstream, so a
 * value is finite only where no flow path into the cell can start outside the tile's data.  With edge_nan == 0 the values are
 * those of the paths inside the tile: a lower bound for max.
 * Cells on or downstream of a drainage cycle (pit edges can close one) never become ready: they are NaN and counted in
 * *n_unresolved; there is no re-seed loop.  (A cell that the edge rule makes NaN is final from the start and not counted.)
 * out: [n,m] host doubles (may be NULL); *ms: device time of the sweep (hipEvent pair); *levels: dependent steps of the sweep
 * (the initial level, tile passes that finished something, levels of the queue that takes the rest).  Needs the tile's flow
 * graph: -3 when no pydem_uca / pydem_build_graph has run since the elevation, slope, direction or flats last changed.
 * Writes no field of the tile, no timing, no level field of the graph words and no state of the forward sweep or of the edge
 * fix-up.  Its state is pydem_dist_down's (the result plane and the int32 plane, 12 bytes per cell, and four words per 32 x 32
 * block; allocated by the first call of either, freed with the tile): a call overwrites the other's result ON THE DEVICE; arrays
 * already returned are host copies. */
int pydem_dist_up(pydem_tile *t, int kind /* 0 h, 1 v, 2 s */, int stat /* 0 ave, 1 min, 2 max */, int edge_nan,
                  double *out /* [n,m] host */, double *ms, int64_t *levels, int64_t *n_unresolved);
/* Reverse accumulation: a linear (op 0) or max (op 1) recursion over the OUT-edges of the D-infinity flow graph, swept from
 * the outlets to the sources like pydem_dist_down (TauDEM's DinfUpDependence and DinfRevAccum next to its AreaDinf; no
 * reference method).  The out-edges of a cell c are those pydem_dist_down reads: the regular edges that survive the keep-filter
 * of _mk_adjacency_matrix (pydem/dem_processing.py:1136-1137), of weights p and 1 - p, and the pit -> drain edges with theirs.
 * Rules, in this order:
 *     V[c] = NaN                    where the elevation of c is NaN;
 *     V[c] = absorb_value           where absorb[c] != 0: the cell is final from the start, its own out-edges do not matter;
 *     V[c] = seed[c]                where c has no out-edge (undrained pits and flats, cells whose flow only leaves the tile);
 *     otherwise, once every v_e is final, over the out-edges e = c -> v_e of weight w_e,
 *       op 0 (sum): acc = 0; acc += w_e * V[v_e]; V[c] = seed[c] + acc   (NOT normalised by the surviving weights: flow that
 *                   leaves the tile reaches nothing inside it)
 *       op 1 (max): V[c] = max(seed[c], max_e V[v_e]);
 *     NaN if any operand is NaN, stored as the canonical NaN.
 * The out-edges are taken in ascending destination order, a regular edge before a pit edge to the same cell (the order of
 * pydem_dist_down), by ONE lane per cell that pulls final values: no floating-point atomics, results identical from run to run
 * and from schedule to schedule.  Cells on or upstream of a drainage cycle (pit edges can close one) never become ready: they
 * are NaN and counted in *n_unresolved; there is no re-seed loop.
 * What it is used for: the upslope dependence of a target set T (the share of a cell's flow that reaches T; > 0 is T's
 * D-infinity watershed) is op 0, seed NULL, absorb = T, absorb_value = 1; the reverse accumulation of a load w (the weighted
 * sum of w over everything downslope of a cell) is op 0, seed = w, absorb NULL; the maximum downslope load is op 1, seed = w.
 * seed: [n,m] host doubles, or NULL = 0 everywhere (op 0 only); absorb: [n,m] host mask (non-zero = absorbing), or NULL = none;
 * absorb_value: finite.  out: [n,m] host doubles (may be NULL); *ms and *levels as for pydem_dist_down: device time of the sweep
 * (hipEvent pair), and the dependent steps of the reverse sweep (the initial level, tile passes that finished something, levels
 * of the queue that takes the rest).  -2 for op out of range, op 1 without a seed and a non-finite absorb_value; -3 (no flow
 * graph) when no pydem_uca / pydem_build_graph has run since the elevation, slope, direction or flats last changed.
 * Writes no field of the tile, no timing and no state of the forward sweep or of the edge fix-up.  The result plane, the int32
 * plane, the counter block and the byte mask are pydem_dist_down's (allocated by the first call of any of the three, freed with
 * the tile): a call overwrites the other calls' result ON THE DEVICE; arrays already returned are host copies.  The seed is one
 * more plane of the call's own (8 bytes per cell), allocated by the first call that passes a seed and freed with the tile. */
int pydem_rev_accum(pydem_tile *t, int op /* 0 sum, 1 max */,
                    const double *seed /* [n,m] host, or NULL = 0 everywhere (op 0 only) */,
                    const uint8_t *absorb /* [n,m] host mask, or NULL = none */, double absorb_value,
                    double *out /* [n,m] host, may be NULL */, double *ms, int64_t *levels, int64_t *n_unresolved);
/* Forward accumulation with a per-cell rule: a load that is multiplied on its way out of every cell and capped on its way into
 * every cell, swept from the divides to the outlets like pydem_dist_up (TauDEM's DinfDecayAccum and DinfTransLimAccum next to its
 * AreaDinf; no reference method).  The in-edges of a cell c are those pydem_dist_up reads: the regular edges u -> c that survive
 * the keep-filter of _mk_adjacency_matrix (pydem/dem_processing.py:1136-1137), of weight p or 1 - p of the SOURCE u, and the
 * pit -> drain edges with theirs.  V is the result, I the inflow:
 *     V[c] = I[c] = NaN             where the elevation of c is NaN and, with edge_nan != 0, where pydem_dist_up's edge rule makes
 *                                   a cell NaN (the tile's border, the 8-neighbours of a NaN elevation);
 *     I[c] = 0, tot = load[c]       where c has no in-edge;
 *     otherwise, once every u_e is final, over the in-edges e = u_e -> c of weight w_e,
 *       acc = 0; acc += w_e * (mult[u_e] * V[u_e])   (mult NULL: acc += w_e * V[u_e]);   I[c] = acc;   tot = load[c] + acc;
 *     V[c] = tot                    (cap NULL),      V[c] = tot is NaN ? NaN : min(tot, cap[c])      (cap).
 * A NaN that flows in stays NaN through the cap; every NaN is stored as the canonical NaN.  The in-edges are taken in ascending
 * source order, a regular edge before a pit edge from the same source (the order of pydem_dist_up), by ONE lane per cell that
 * pulls final values: no floating-point atomics, results identical from run to run and from schedule to schedule.  Cells on or
 * downstream of a drainage cycle (pit edges can close one) never become ready: V and I are NaN there and the cells are counted in
 * *n_unresolved; there is no re-seed loop.  The values are the tile's own: flow that enters through the border is not in them,
 * and with edge_nan != 0 a value is finite only where no flow path into the cell can start outside the tile's data.
 * What it is used for: the weighted accumulation over the graph's in-edges is mult NULL, cap NULL; a load that decays on its way
 * down (decay in [0, 1]: the share of a cell's V that leaves it) is mult = decay; a supply routed under a transport capacity is
 * load = supply, cap = capacity: V is the transport, (supply + I) - V the deposition.
 * load: [n,m] host doubles; mult, cap: [n,m] host doubles or NULL (cap: +inf allowed, NaN refused on the host before any device
 * work).  out: [n,m] host doubles (may be NULL); out_inflow: [n,m] host doubles or NULL -- I, bit for bit the acc that produced
 * V, from one more pass over the rows that runs only when it is asked for.  *ms: device time of the sweep and of that pass
 * (hipEvent pairs); *levels as for pydem_dist_up.  -2 when load is NULL or cap holds a NaN; -3 (no flow graph) when no pydem_uca /
 * pydem_build_graph has run since the elevation, slope, direction or flats last changed.
 * Writes no field of the tile, no timing and no state of the forward sweep or of the edge fix-up.  The result plane, the int32
 * plane and the counter block are pydem_dist_down's, the plane of the load is pydem_rev_accum's seed (allocated by the first call
 * that needs them, freed with the tile): a call overwrites the other calls' result ON THE DEVICE; arrays already returned are host
 * copies.  mult, cap and the inflow are three more planes of the call's own (8 bytes per cell each), each allocated by the first
 * call that uses it and freed with the tile. */
int pydem_fwd_accum(pydem_tile *t, const double *load /* [n,m] host */, const double *mult /* [n,m] host, or NULL = 1 */,
                    const double *cap /* [n,m] host, or NULL = none */, int edge_nan, double *out /* [n,m] host, may be NULL */,
                    double *out_inflow /* [n,m] host, may be NULL */, double *ms, int64_t *levels, int64_t *n_unresolved);
/* The stream network on the D-infinity flow graph: the receiver of every cell, the Strahler order and the link of every stream
 * cell, the sub-basin of every cell (TauDEM's StreamNet / GridNet, done there on D8; no reference method).  The graph is the one
 * pydem_dist_down reads.  The out-edges of a cell, in the order of that call, are the regular edges that survive the keep-filter
 * of _mk_adjacency_matrix (pydem/dem_processing.py:1136-1137), of weights p and 1 - p, and the kept pit -> drain edges with
 * theirs: ascending destination, a regular edge before a pit edge to the same cell.
 *     recv[c]    the destination of the first out-edge of greatest weight in that order; -1 where c has no out-edge or a NaN
 *                elevation.  It depends on the graph alone.  Every cell has at most one receiver: the receivers form a forest
 *                (plus the cycles that pit edges can close).
 *     S          the stream set: `streams`, a host mask [n,m] (non-zero = stream), or, when streams == NULL, uca >= uca_threshold
 *                (finite, >= 0) on the tile's current uca (pending incremental edge rounds are flushed first; NaN is never a
 *                stream).  Cells with a NaN elevation are never in S.
 *     the stream inflows of c in S: the cells u in S with recv[u] == c, each counted once.
 *     order[c]   (forward sweep, divides to outlets)  0 off S; 1 for c in S without a stream inflow; otherwise, with M the greatest
 *                order among its stream inflows and k the number of inflows that have it, M + 1 if k >= 2, else M (Strahler).
 *     link[c]    (the same sweep)  c in S is a link head iff its number of stream inflows is not 1; a cell with exactly one
 *                belongs to that inflow's link.  The raw label of a link is its head cell + 1; 0 off S.
 *     basin[c]   (reverse sweep, outlets to sources)  link[c] on S; off S basin[recv[c]]; 0 where recv[c] == -1.
 * Readiness is that of pydem_dist_up and pydem_dist_down: a cell of the forward sweep waits for ALL its graph in-neighbours (the
 * cells off S are final from the start), a cell of the reverse sweep for ALL its out-neighbours (the cells of S are); only the
 * value rule looks at receivers.  ONE lane finishes a cell from final values, and every value is an integer: results identical
 * from run to run and from schedule to schedule.  Cells of S on or downstream of a drainage cycle never become ready in the
 * forward sweep: order and link are -1 there, and n_unresolved[0] counts them.  basin is -1 on or upstream of a cycle and
 * wherever the link that is reached is -1; n_unresolved[1] counts the cells whose basin is -1.  There is no re-seed loop.
 * receiver, order, link, basin: [n,m] host int32, each may be NULL.  receiver alone (all else NULL) runs only the pass over the
 * rows and needs no stream set; basin != NULL runs the reverse sweep, and the forward one before it even if order and link are
 * NULL.  ms[3]: device time of the receiver pass, the forward and the reverse sweep (hipEvent pairs; 0 for what did not run);
 * levels[2], n_unresolved[2]: forward, reverse, levels as for pydem_dist_up / pydem_dist_down.  -2 for a uca_threshold that is not
 * finite or negative when a sweep runs without a mask; -3 (no flow graph) when no pydem_uca / pydem_build_graph has run since
 * the elevation, slope, direction or flats last changed, and for a threshold without the tile's uca.
 * Writes no field of the tile, no timing and no state of the forward sweep of pydem_uca or of the edge fix-up.  The result plane,
 * the int32 plane, the counter block and the byte mask are pydem_dist_down's and the plane that carries the forward result into
 * the reverse sweep is pydem_rev_accum's seed: a call overwrites the other calls' result ON THE DEVICE; arrays already returned
 * are host copies.  The receivers are two more planes of the call's own (int32 destination and a byte that says which edge it
 * is -- 0..7: the neighbour direction NW N NE W E SW S SE, 8: a pit edge, 255: none; 5 bytes per cell), allocated by the first
 * call and freed with the tile. */
int pydem_stream_network(pydem_tile *t, const uint8_t *streams /* [n,m] host, or NULL */, double uca_threshold,
                         int32_t *receiver, int32_t *order, int32_t *link, int32_t *basin /* [n,m] host, each may be NULL */,
                         double *ms /* [3] */, int64_t levels[2], int64_t n_unresolved[2] /* forward, reverse */);
/* Accumulation along the receiver tree of the D-infinity flow graph: the single-flow-direction (D8-style) accumulation on the
 * steepest D-infinity receiver and, cut at the link boundaries, the per-reach catchment totals of a stream network (the columns
 * of TauDEM's StreamNet table; no reference method).  recv / code are exactly those of pydem_stream_network: the same pass over
 * the rows, the same tie rule.
 *     the tree in-neighbours of c: the cells u with recv[u] == c, each counted once (a source with two pit entries to c counts once).
 *     S          the stream set, read only when cut != 0 and then taken exactly as pydem_stream_network takes its own: `streams`,
 *                a host mask [n,m], or, when streams == NULL, uca >= uca_threshold; a NaN elevation is never in S.  cut == 0: S is empty.
 *     the stream inflows of c: the tree in-neighbours of c that are in S.
 *     taken      c takes the tree edge u -> c unless cut != 0, u is in S, and c is not the continuation of u's link -- c is not in
 *                S, or c does not have exactly one stream inflow.  Edges from cells off S are always taken.
 *     V[c]       NaN where the elevation is NaN and, with edge_nan != 0, on the tile's border cells and on the neighbours of NaN
 *                elevations (pydem_dist_up's rule); those cells are final from the start.  load[c] where no graph edge enters c.
 *                Every other cell is finished once EVERY graph in-neighbour is final (the readiness of pydem_dist_up, with all
 *                in-neighbours, not only the tree's): op 0: acc = 0; acc += V[u] over the taken tree in-neighbours in ascending
 *                source index; V = load + acc.  op 1 / 2: max(load, max V[u]) / min(load, min V[u]) over the same cells.  NaN if
 *                any operand is NaN, stored canonical.
 * NaN therefore spreads along taken tree edges only, and a cut stops it: with cut and edge_nan, a finite value at a link's tail says
 * that link's own catchment lies wholly inside the tile's data, even where a link above it does not.  With cut, load = 1, op 0, the
 * value at a link's tail is the number of cells of the link's sub-basin.  ONE lane finishes a cell from final values in that
 * operand order: results identical from run to run and from schedule to schedule.  Cells on or downstream of a drainage cycle
 * never become ready: NaN, counted in *n_unresolved; there is no re-seed loop.
 * load: [n,m] host doubles.  out: [n,m] host doubles (may be NULL).  at / n_at / at_out: after the sweep one small kernel gathers
 * the values at the flat cells at[0..n_at) into at_out (NULL / 0: no gather) -- a reach table needs K doubles, not a plane.  *ms:
 * device time of the two passes over the rows (receivers, codes) and the sweep (hipEvent pairs); *levels as for pydem_dist_up.
 * -2 for an op outside 0..2, a NULL load, a uca_threshold that is not finite or negative when it is read (cut without a mask) and
 * an `at` entry outside [0, n m), all before any device work; -3 (no flow graph) when no pydem_uca / pydem_build_graph has run
 * since the elevation, slope, direction or flats last changed, and for a threshold without the tile's uca.
 * Writes no field of the tile, no timing and no state of the forward sweep of pydem_uca or of the edge fix-up.  The result plane,
 * the int32 plane, the counter block and the byte mask are pydem_dist_down's, the plane of the load is pydem_rev_accum's seed, the
 * receiver planes are pydem_stream_network's: a call overwrites the other calls' result ON THE DEVICE; arrays already returned
 * are host copies.  One more byte plane of the call's own (receiver code + stream bit), allocated by the first call and freed
 * with the tile. */
int pydem_tree_accum(pydem_tile *t, int op /* 0 sum, 1 max, 2 min */, const double *load /* [n,m] host */,
                     int cut /* 0 whole tree, 1 stop at link boundaries */,
                     const uint8_t *streams /* [n,m] host or NULL */, double uca_threshold /* both read only when cut */,
                     int edge_nan, double *out /* [n,m] host, may be NULL */,
                     const int32_t *at, int64_t n_at, double *at_out /* values at the flat cells `at`; may be NULL / 0 */,
                     double *ms, int64_t *levels, int64_t *n_unresolved);
/* the flow graph of pydem_uca (section / proportion / adjacency / pit edges, dem_processing.py:1021-1382) for a tile whose
 * elevation, slope, aspect and flats were uploaded instead of computed -- what the reference's edge worker rebuilds from
 * its stores before every round (process_manager.py:227-240) and a resumed directory job needs once; it resets the tile's
 * edge masks, so upload stored masks afterwards */
int pydem_build_graph(pydem_tile *t, pydem_options *opt);
/* strips in the order left, right, top, bottom; left/right have n_rows entries, top/bottom
 * n_cols; data = neighbour uca (+uca_edges), done/todo = uint8 (process_manager.py:252-255) */
int pydem_uca_edge_update(pydem_tile *t, pydem_options *opt,
                          const double *const data[4], const uint8_t *const done[4],
                          const uint8_t *const todo[4]);
/* The same edge-resolution step for the multi-worker schedule of ProcessManager.process_uca_edges
 * (pydem/process_manager.py:1214-1246, here deterministic waves): the state of the fix-up stays on the device
 * between rounds -- a cell is processed once, when the last unresolved inlet upstream of it resolves, instead of
 * once per round -- so a round costs the cells it finishes, not everything downstream of its seeds.  Masks after
 * a round (edge_todo / edge_done, :848-856) and the areas of finished cells are those of pydem_uca_edge_update;
 * areas of cells that are still downstream of an unresolved inlet lag behind until pydem_uca_edge_flush, which
 * hands them what their finished upstream cells hold (call it when the fix-up ends; pydem_uca_edge_update,
 * pydem_twi and downloads of PYDEM_UCA do it implicitly).  Not available with opt->apply_uca_limit_edges (-6). */
int pydem_uca_edge_round_inc(pydem_tile *t, pydem_options *opt,
                             const double *const data[4], const uint8_t *const done[4],
                             const uint8_t *const todo[4]);
/* the same round with the strips already in the tile's device buffers (written by pydem_board_eval) */
int pydem_uca_edge_round_inc_dev(pydem_tile *t, pydem_options *opt);
int pydem_uca_edge_flush(pydem_tile *t);
int pydem_twi(pydem_tile *t, pydem_options *opt);

/* The pit -> drain triplets built by the last pydem_uca (the reference's local pit_i, pit_j,
 * pit_prop, pydem/dem_processing.py:1378-1380), in emission order.  Call with src == NULL to get
 * the count. */
int pydem_tile_pit_edges(pydem_tile *t, int64_t *n, int32_t *src, int32_t *dst, double *w);

/* The flow graph the sweep runs on, one packed word per cell [n,m] -- the device's form of the adjacency matrix A of
 * _mk_adjacency_matrix (pydem/dem_processing.py:1072-1153; A is never materialised here): bits 0-7 = which of the 8
 * neighbours (NW N NE W E SW S SE) drain into the cell, bit 8 / 9 = the regular out-edge to the facet's first / second
 * neighbour survived the keep-filter (:1136-1137; weights = proportion, 1 - proportion), bit 10 / 11 = the cell has pit
 * out- / in-edges (pydem_tile_pit_edges), bits 12-14 = facet index.  For tests and debugging (the edge set can be held
 * against scipy's / the oracle's triplets). */
int pydem_tile_graph_words(pydem_tile *t, uint32_t *out);

/* Undo the slope patch of the drained pits (mag[pit] = -1 again, flats untouched).  In the
 * reference's directory flow the calc_uca worker never writes its patched slope back to the store
 * (pydem/process_manager.py:192-194), so later phases see slope == -1 at drained pits; the
 * ProcessManager drop-in calls this to keep that behaviour. */
int pydem_tile_restore_pit_slopes(pydem_tile *t);

/* Kernel-only timing hook for bench.py: runs the interior stencil `iters` times on the tile's
 * resident elevation and returns the average kernel time (ms) measured with hipEvents on the
 * tile's stream. */
int pydem_bench_stencil(pydem_tile *t, int iters, double *avg_ms);

/* ---- the reference's own native boundary, on a generic scipy CSC/CSR graph ----------------------
 * Same arguments and in-place behaviour as the Cython functions (host arrays in, updated in place):
 *   pydem_drain_area         cyutils.drain_area        pydem/cyfuncs/cyutils.pyx:78-116 (loop :119-187)
 *   pydem_drain_connections  cyutils.drain_connections pydem/cyfuncs/cyutils.pyx:35-46  (loop :49-72)
 * edge_todo / edge_todo_no_mask may be NULL.  The DEMProcessor entry points above do not use these
 * (they never materialise the matrix); they exist so code written against cyutils keeps working. */
int pydem_drain_area(double *area, uint8_t *done, uint8_t *ids, const int32_t *col_indptr, const int32_t *col_indices,
                     const double *col_data, const int32_t *row_indptr, const int32_t *row_indices, int64_t n_rows,
                     int64_t n_cols, double *edge_todo, double *edge_todo_no_mask, int skip_edge, int device);
int pydem_drain_connections(uint8_t *arr, uint8_t *ids, const int32_t *indptr, const int32_t *indices, int64_t n,
                            uint8_t set_to, int device);

/* ---- RCCL transport for the edge strips of the directory flow -------------------------------
 * Replaces the shared zarr store the reference's workers exchange strips through
 * (pydem/process_manager.py:243-255, write-verify-retry :362-381).  One communicator per process
 * (one process per GPU); rank 0 creates the 128-byte id and hands it to the other ranks by any
 * out-of-band channel.  A gather step is: begin(n) -> pack_line(...) for the lines this rank
 * owns -> allreduce(sum) -> every rank holds all lines (host copy in host_out). */
typedef struct pydem_comm pydem_comm;
int pydem_comm_unique_id(char *out128);
int pydem_comm_create(int world, int rank, const char *uid128, int device, pydem_comm **out);
int pydem_comm_destroy(pydem_comm *c);
int pydem_comm_begin(pydem_comm *c, int64_t n_doubles);
int pydem_comm_pack_line(pydem_comm *c, pydem_tile *t, int field, int axis, int64_t index, int64_t offset);
/* several lines of one tile without a host synchronisation (stream events order clear -> packs -> collective) */
int pydem_comm_pack_lines(pydem_comm *c, pydem_tile *t, int count, const int *fields, const int *axes, const int64_t *indices,
                          const int64_t *offsets);
int pydem_comm_put(pydem_comm *c, const double *host_in, int64_t n_doubles, int64_t offset);
int pydem_comm_allreduce(pydem_comm *c, int64_t n_doubles, int op /* 0 sum, 1 max */, double *host_out);

/* ---- edge board: the strips of ProcessManager.process_uca_edges stay on the device (comm.hip).
 * Replaces what the reference's edge worker and manager do on the host for every round: reading the neighbour
 * lines from the store, the corner rules and rule :274 (pydem/process_manager.py:243-274), the metrics
 * (calc_uca_ec_metrics :199-221).  The board holds every line some tile reads (doubles; masks as 0 / 1) at fixed
 * offsets, identically on every rank.
 *   pydem_board_set_desc  where tile `index` finds its lines: offsets28 = own_todo[4], own_done[4], nb_uca[4],
 *                         nb_done[4], nb_todo[4] (sides left, right, top, bottom), cnr_done[4], cnr_uca[4] (diagonal
 *                         pixel of the corners tl, tr, bl, br); -1 = missing; flags8 = nb_self[4] (the edge table
 *                         points the tile at its own line), cnr_1ov[4] (check_1overlap :286-293); `tile` = the
 *                         resident tile whose strip buffers the evaluation fills (NULL: a tile of another rank)
 *   pydem_board_set_lines which part of the board holds the lines of tile `index` (mb_start, size) and, for a tile of
 *                         this rank, the lines to gather from it (field / axis / index -> rel_offset inside that part); for a
 *                         tile of another rank (`tile` NULL) the same list gives the layout only (which lines are areas, which
 *                         masks: the queued waves carry masks as bytes through the collective)
 *   pydem_board_refresh   after a wave (the same tile list on every rank): the tiles of this rank gather their lines
 *                         into the wave staging buffer, one ncclAllReduce(sum) over disjoint fills when `c` is given,
 *                         then the staging buffer is copied into the board
 *   pydem_board_eval      strips (data, done, todo after the corner rules, rule :274 -- everywhere if full[k], else
 *                         only on the mosaic border -- and the adoption of finished neighbour values) into the
 *                         tiles' buffers, and 8 words per tile to `out` (all tiles of the board): cells 'todo' and
 *                         facing a finished neighbour, cells 'todo', 'todo' pixels the border rule / full rule :274
 *                         would drop, seeds, a hash of the strips */
typedef struct pydem_board pydem_board;
int pydem_board_create(int device, int n_tiles, int64_t n_doubles, pydem_board **out);
int pydem_board_destroy(pydem_board *b);
int pydem_board_set_desc(pydem_board *b, int index, int32_t n, int32_t m, const int64_t *offsets28, const int32_t *flags8,
                         pydem_tile *tile);
int pydem_board_set_lines(pydem_board *b, int index, int64_t mb_start, int64_t size, pydem_tile *tile, int count,
                          const int *fields, const int *axes, const int64_t *indices, const int64_t *rel_offsets);
int pydem_board_refresh(pydem_board *b, pydem_comm *c, int n_wave, const int *wave_tiles);
/* the same refresh with the sum over ranks done by the caller on the host (transports without RCCL: the torch.distributed
 * fallback, pydem_amd/parallel.py DistTransport): stage = zero + pack this rank's lines of the wave + copy to host_out
 * (*n_doubles values, at most cap); the caller sums the buffers of all ranks; unstage files the sum on the board.
 * Replaces the same store round trip as pydem_board_refresh (process_manager.py:243-255). */
int pydem_board_refresh_stage(pydem_board *b, int n_wave, const int *wave_tiles, double *host_out, int64_t cap, int64_t *n_doubles);
int pydem_board_refresh_unstage(pydem_board *b, int n_wave, const int *wave_tiles, const double *host_in, int64_t n_doubles);
int pydem_board_eval(pydem_board *b, int count, const int *tiles, const int *full, unsigned long long *out);
/* Up to k_waves (<= 64) waves of the same schedule queued back to back WITHOUT a look from the manager (the reference's manager
 * loop, pydem/process_manager.py:1214-1246, polls its workers and re-ranks after every completion; for a mosaic of at most
 * 2 * n_workers tiles the ranking :1177-1188 selects every tile with a positive metric, so the wave can be chosen by a
 * kernel): per wave a selection kernel (candidates = positive metric or 'todo' pixels dropped on the mosaic border, strips
 * changed since the tile's last round), for every tile of this rank a condensed round + the gather of its lines gated by the
 * wave's member word, one ncclAllReduce(sum, bytes) of the whole staging buffer (areas as doubles, masks as bytes) when `c` is
 * given, the unpacking onto the board and the
 * evaluation of the tiles that read the wave's lines.  `state`: 528 64-bit words in and out --
 *   [0] bit per tile: its rounds may be queued (a candidate without the bit stops the batch BEFORE its wave: the host runs
 *   that wave, e.g. a tile's first round, which builds its fix-up state), [1] out: 0 = all k_waves ran, 1 = the fix-up
 *   is over (no candidate, and no tile drops a 'todo' pixel under rule :274 everywhere -- while one does, the tile that
 *   drops the most runs alone with its strips evaluated under that rule: the tie-break wave of the schedule, also chosen by the
 *   kernel), 2 = a candidate needs the host, 3 = wave limit,
 *   [2] out: waves run, [3] waves allowed, [8+a] / [72+a] metric numerator / denominator of tile a as the schedule holds
 *   them (stale for diagonal neighbours like check_mets :1116-1136), [136+a] / [200+a] strip hash of a's last round / whether
 *   it has one, [264+a] bit mask of the tiles reading a line of a, [328+a] a and its four side neighbours, [392+w] out: the
 *   members of wave w, [7] out: the waves ran as captured hipGraphs (one launch per wave; default without a communicator, plain launches with one; PYDEM_EDGE_GRAPH=0 / 1 forces either),
 *   [456+a] scratch (round stamps), [521] out: tie-break waves of the batch, [522] out: bit w = wave w was one.
 *   `scal_out` as `out` of pydem_board_eval.  pydem_tile_edge_queue_ready: 1 when the tile's rounds can be queued (condensed fix-up state built by its first round, strips buffers attached by pydem_board_set_desc). */
int pydem_board_run_waves(pydem_board *b, pydem_comm *c, int k_waves, unsigned long long *state, unsigned long long *scal_out);
/* A batch contains collectives, so everything that can fail on ONE rank alone is a call of its own:
 *   pydem_board_prepare_waves  checks / builds what a batch over the tiles `ok_tiles` (bit per tile, = state[0]) needs -- the
 *       tiles' fix-up state, watched lines, the staging layout (`staged` != 0: the batch sums its staging buffer over the ranks)
 *       and the device tables -- and enqueues nothing.  With several ranks the caller lets the ranks agree on its verdict
 *       (one allreduce) before any of them calls pydem_board_run_waves; that call then only enqueues.  (A single process may
 *       skip it: run_waves prepares what is not prepared.)
 *   pydem_board_run_waves_ex   the same batch with the sum over the ranks done by the CALLER (`exchange`, not RCCL: processes
 *       sharing one GPU, transports without RCCL): per wave the staging buffer goes to the host, exchange(ctx, 0, bytes, n)
 *       sums it byte-wise in place, and -- what RCCL cannot do -- exchange(ctx, 1, doubles, 8) (maximum in place) first
 *       checks that every rank selected the SAME wave (-8 and a message otherwise).  One host look per wave: the tested
 *       restatement of the queued path (every rank runs the selection kernel from replicated numbers), not the fast one.
 * A batch that does not come back within PYDEM_EDGE_TIMEOUT seconds (default 300, 0 = wait for ever) returns -7 with the last
 * wave selected on this rank in the message and aborts the communicator (ncclCommAbort): ranks whose schedules disagree
 * would otherwise sit in ncclAllReduce without a word.  Replaces the manager's poll loop, process_manager.py:1214-1246.
 *   pydem_comm_count           ranks behind the communicator (ncclCommCount) */
typedef int (*pydem_exchange_fn)(void *ctx, int op, void *buf, int64_t n);
int pydem_board_prepare_waves(pydem_board *b, int staged, unsigned long long ok_tiles);
int pydem_board_run_waves_ex(pydem_board *b, pydem_comm *c, int k_waves, unsigned long long *state, unsigned long long *scal_out,
                             pydem_exchange_fn exchange, void *ctx);
int pydem_comm_count(pydem_comm *c, int *count);
int pydem_tile_edge_queue_ready(pydem_tile *t);
int pydem_board_download(pydem_board *b, double *out);

/* ---- elevation conditioning: host-side inner loops (no device work; pydem_amd/conditioning.py keeps the
 * vectorised prologues -- 3x3 filters, scipy.ndimage.label, the numpy argsort whose tie order is part of the
 * result -- and calls these for the per-region / per-pit loops of the reference)
 *   pydem_cond_pit_artifacts: calc_fill_pit_artifacts (dem_processing.py:396-426); lab = labels (1..nlab) of the
 *       candidate depressions, raise[c] = 1 where the cell is lifted by one unit
 *   pydem_cond_fill_flats:    _fill_flat (:308-394) for every labelled flat of calc_fill_flats (:551-579);
 *       data = unmodified surface (float64, NaN = masked), built = copy of it that receives the new flats
 *   pydem_cond_pit_paths:     calc_pit_drain_paths (:428-548) for the pits in the given order, surface edited in place */
int pydem_cond_pit_artifacts(const double *elev, int64_t n_rows, int64_t n_cols, const int32_t *lab, int32_t nlab,
                             double max_area, int f32 /* the surface holds float32 values */, uint8_t *raise);
int pydem_cond_fill_flats(const double *data, double *built, int64_t n_rows, int64_t n_cols, const int32_t *lab,
                          int32_t nlab, double source_tol, int peaks, int pits);
int pydem_cond_pit_paths(double *elev, int64_t n_rows, int64_t n_cols, const int64_t *pits, int64_t npits,
                         const double *dX, int64_t n_dX, const double *dY, int max_iter, int max_dist,
                         double max_dist_XY, int dtype_mode /* 0 float64, 1 integer, 2 float32 surface (values as float64) */,
                         int64_t *n_failed, int64_t *iter_used);

/* TIFF LZW encoder for the GeoTIFF export (host code): the reference writes its exports with rasterio's compress='lzw'
 * (pydem/process_manager.py:905, :930).  dst must hold up to n * 3 / 2 + 16 bytes (incompressible data grows by 12 %);
 * *out_n = bytes written.  The stream is libtiff's for the same input. */
int pydem_tiff_lzw_encode(const uint8_t *src, int64_t n, uint8_t *dst, int64_t cap, int64_t *out_n);

#ifdef __cplusplus
}
#endif
#endif /* PYDEM_HIP_H */
