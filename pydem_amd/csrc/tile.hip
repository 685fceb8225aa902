// tile.hip -- handle management, spacing tables, upload/download and the extern "C" surface.
#include "internal.h"
#include "line_gather.h"
#include "uca_graph.h"      // CI_STATIC_MASK, CS_FLAT_SAVE
#include <cmath>
#include <stdarg.h>
#include <string.h>

static thread_local char g_err[1024] = "";

void pydem_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

template <typename T>      // (its counterpart k_line_gather: line_gather.h)
__global__ void k_line_scatter(const T *__restrict__ src, int64_t stride, int64_t count, T *__restrict__ dst)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) dst[k * stride] = src[k];
}

__global__ void k_restore_pit_slopes(const int32_t *__restrict__ src, int64_t n, double *mag)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        if (src[e] >= 0) mag[src[e]] = -1.0;      // unused output slots hold -1
}

// pydem_uca_weighted on a tile without a (current) flow graph: the graph stage patches mag / flats at the drained pits
// (:1369-1371), and pits are flat cells (the pit search's candidates: flats && elev > 0).  Saving (cell, mag) of every flat
// cell before the stage and writing both back afterwards restores the two planes exactly.
__global__ void k_flat_save(const uint8_t *__restrict__ flats, const double *__restrict__ mag, int64_t NN, int32_t *__restrict__ cells,
                            double *__restrict__ vals, int64_t cap, unsigned long long *count)
{
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {     // (uniform per workgroup)
        const int64_t c = c0 + threadIdx.x;
        const bool f = c < NN && flats[c] != 0;
        const unsigned long long b = __ballot(f);
        if (!b) continue;
        const int lane = (int)__lane_id(), leader = __ffsll((long long)b) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(b));
        base = __shfl(base, leader);
        const int64_t k = (int64_t)base + __popcll(b & ((1ull << lane) - 1ull));
        if (f && cells && k < cap) { cells[k] = (int32_t)c; vals[k] = mag[c]; }
    }
}

__global__ void k_flat_restore(const int32_t *__restrict__ cells, const double *__restrict__ vals, int64_t n, double *__restrict__ mag,
                               uint8_t *__restrict__ flats)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        mag[cells[k]] = vals[k];
        flats[cells[k]] = 1;
    }
}

template <typename S>
__global__ void k_convert_to_f64(const S *__restrict__ src, double *__restrict__ dst, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (double)src[i];
}

// pydem_find_flats behind pydem_tile_restore_pit_slopes: the mask only differs from mag == -1 at the restored pits
__global__ void k_find_flats_pits(const int32_t *__restrict__ src, int64_t n, uint8_t *flats)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        if (src[e] >= 0) flats[src[e]] = 1;
}

__global__ void k_find_flats(const double *__restrict__ mag, uint8_t *__restrict__ flats, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) flats[i] = (mag[i] == -1.0);    // dem_processing.py:305-306
}

size_t dtype_size(int dt)
{
    switch (dt) {
        case PYDEM_F64: return 8;
        case PYDEM_F32: return 4;
        case PYDEM_I16: return 2;
        case PYDEM_I32: return 4;
        case PYDEM_U8: return 1;
        case PYDEM_I8: return 1;
    }
    return 0;
}

int field_ptr(pydem_tile *t, int field, void ***pp, size_t *elem)
{
    switch (field) {
        case PYDEM_ELEV: *pp = (void **)&t->elev; *elem = 8; return 0;
        case PYDEM_MAG: *pp = (void **)&t->mag; *elem = 8; return 0;
        case PYDEM_DIRECTION: *pp = (void **)&t->dir; *elem = 8; return 0;
        case PYDEM_FLATS: *pp = (void **)&t->flats; *elem = 1; return 0;
        case PYDEM_SECTION: *pp = (void **)&t->section; *elem = 1; return 0;
        case PYDEM_PROPORTION: *pp = (void **)&t->prop; *elem = 8; return 0;
        case PYDEM_UCA: *pp = (void **)&t->uca; *elem = 8; return 0;
        case PYDEM_TWI: *pp = (void **)&t->twi; *elem = 8; return 0;
        case PYDEM_EDGE_TODO: *pp = (void **)&t->edge_todo; *elem = 1; return 0;
        case PYDEM_EDGE_DONE: *pp = (void **)&t->edge_done; *elem = 1; return 0;
        case PYDEM_WEIGHT: *pp = (void **)&t->weight; *elem = 8; return 0;
        case PYDEM_UCA_WEIGHTED: *pp = (void **)&t->uca_w; *elem = 8; return 0;
    }
    pydem_set_error("unknown field id %d", field);
    return -2;
}

int ensure_field(pydem_tile *t, int field)
{
    void **pp; size_t elem;
    PYDEM_TRY(field_ptr(t, field, &pp, &elem));
    if (elem == 8) return tile_alloc(t, (double **)pp, (size_t)t->NN);
    return tile_alloc(t, (uint8_t **)pp, (size_t)t->NN);
}

}  // namespace

int ensure_fields(pydem_tile *t, std::initializer_list<int> fields)
{
    for (int f : fields) PYDEM_TRY(ensure_field(t, f));
    return 0;
}

extern "C" {

const char *pydem_hip_last_error(void) { return g_err; }

int pydem_hip_release_scratch(void)
{
    devmem_release_all();
    return 0;
}

int pydem_hip_device_count(int *count)
{
    HIP_TRY(hipGetDeviceCount(count));
    return 0;
}

int pydem_hip_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes)
{
    size_t f = 0, tot = 0;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemGetInfo(&f, &tot));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)tot;
    return 0;
}

int pydem_hip_device_name(int device, char *buf, int buflen)
{
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return 0;
}

static int tile_init(pydem_tile *t)
{
    HIP_TRY(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&t->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_join, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_snap, hipEventDisableTiming));
    for (int i = 0; i < 8; i++) HIP_TRY(hipEventCreate(&t->ev[i]));
    PYDEM_TRY(tile_alloc(t, &t->counters, 64));
    HIP_TRY(hipHostMalloc((void **)&t->h_counters, 64 * sizeof(int32_t), hipHostMallocDefault));
    return 0;
}

int pydem_tile_create(int64_t n_rows, int64_t n_cols, int device, pydem_tile **out)
{
    if (n_rows < 3 || n_cols < 3) { pydem_set_error("tile must be at least 3x3 (got %lld x %lld)", (long long)n_rows, (long long)n_cols); return -2; }
    if (n_rows * n_cols >= (int64_t)INT32_MAX) { pydem_set_error("tile too large for int32 cell ids"); return -2; }
    HIP_TRY(hipSetDevice(device));
    pydem_tile *t = new pydem_tile();
    t->n = n_rows; t->m = n_cols; t->NN = n_rows * n_cols; t->device = device;
    const int rc = tile_init(t);
    if (rc != 0) { pydem_tile_destroy(t); return rc; }      // (the half-built handle goes; the error text stays)
    *out = t;
    return 0;
}

int pydem_tile_destroy(pydem_tile *t)
{
    if (!t) return 0;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    // (a stage that returned early between the fork and the join of the side stream may have left kernels there that still
    // write edge_todo / todo_work / prop: the planes go to the free lists -- i.e. to the next tile -- only once both streams are idle)
    if (t->stream2) (void)hipStreamSynchronize(t->stream2);
    tile_release_all(t);
    if (t->h_counters) (void)hipHostFree(t->h_counters);
    if (t->h_strip_d) (void)hipHostFree(t->h_strip_d);
    if (t->h_stage) (void)hipHostFree(t->h_stage);
    if (t->h_strip_f) (void)hipHostFree(t->h_strip_f);
    if (t->dd_h_ctr) (void)hipHostFree(t->dd_h_ctr);
    for (int i = 0; i < 2; i++) if (t->dd_ev[i]) (void)hipEventDestroy(t->dd_ev[i]);
    for (int i = 0; i < 8; i++) if (t->ev[i]) (void)hipEventDestroy(t->ev[i]);
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    if (t->ev_join) (void)hipEventDestroy(t->ev_join);
    if (t->ev_snap) (void)hipEventDestroy(t->ev_snap);
    if (t->stream2) { (void)hipStreamSynchronize(t->stream2); (void)hipStreamDestroy(t->stream2); }
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
    return 0;
}

int pydem_tile_set_spacing(pydem_tile *t, const double *dX, const double *dY, const double *dX2, const double *dY2)
{
    HIP_TRY(hipSetDevice(t->device));
    const int64_t n = t->n;
    // the facet tests compare slopes by cross-multiplication with the spacings and divide with host reciprocals: both
    // assume finite, strictly positive cell sizes (the reference would run on with negative or zero ones and return
    // mirrored / infinite slopes -- not reproduced, so refuse)
    for (int64_t r = 0; r < n - 1; r++)
        if (!(dX[r] > 0 && dY[r] > 0 && std::isfinite(dX[r]) && std::isfinite(dY[r]))) {
            pydem_set_error("pydem_tile_set_spacing: dX / dY must be finite and > 0 (row %lld: %g, %g)", (long long)r, dX[r], dY[r]);
            return -2;
        }
    for (int64_t r = 0; r < n; r++)      // the sweep carries the edge_todo taint in the sign of a cell's shares: areas must be positive
        if (!(dX2[r] * dY2[r] > 0 && std::isfinite(dX2[r] * dY2[r]))) {
            pydem_set_error("pydem_tile_set_spacing: dX2 * dY2 (cell area) must be finite and > 0 (row %lld: %g, %g)", (long long)r, dX2[r], dY2[r]);
            return -2;
        }
    t->h_dX.assign(dX, dX + n - 1); t->h_dY.assign(dY, dY + n - 1);
    t->h_dX2.assign(dX2, dX2 + n); t->h_dY2.assign(dY2, dY2 + n);
    std::vector<RowTab> tab((size_t)(n - 1));
    int exotic = 0;
    for (int64_t r = 0; r < n - 1; r++) {
        RowTab &e = tab[(size_t)r];
        e.dX = dX[r]; e.dY = dY[r];
        e.hyp = sqrt(dX[r] * dX[r] + dY[r] * dY[r]);   // np.sqrt(d1**2 + d2**2), dem_processing.py:1962
        e.thA = atan2(dY[r], dX[r]);                    // np.arctan2(d2, d1), :1936 (host libm == numpy)
        e.thB = atan2(dX[r], dY[r]);
        e.rdX = 1.0 / e.dX; e.rdY = 1.0 / e.dY; e.rhyp = 1.0 / e.hyp;
        // the stencil's mask path assumes that no slope quotient can overflow into a NaN: elevations are tested per row,
        // the spacings here
        if (!(e.dX > 0x1p-500 && e.dX < 0x1p500 && e.dY > 0x1p-500 && e.dY < 0x1p500 && e.hyp < 0x1p500)) exotic = 1;
    }
    { const char *ev = getenv("PYDEM_STENCIL_EXACT"); if (ev && *ev == '1') exotic = 1; }
    t->stencil_exact_only = exotic;
    // theta per row for section/proportion: facet-0 spacing of rows 1..n-2 with the first and last
    // entries duplicated (dem_processing.py:1031-1033)
    std::vector<double> st((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        int64_t r = i - 1;
        if (r < 0) r = 0;
        if (r > n - 3) r = n - 3;
        st[(size_t)i] = atan2(dY[r], dX[r]);
    }
    PYDEM_TRY(tile_alloc(t, &t->dX, (size_t)n)); PYDEM_TRY(tile_alloc(t, &t->dY, (size_t)n));
    PYDEM_TRY(tile_alloc(t, &t->dX2, (size_t)n)); PYDEM_TRY(tile_alloc(t, &t->dY2, (size_t)n));
    PYDEM_TRY(tile_alloc(t, &t->rowtab, (size_t)n)); PYDEM_TRY(tile_alloc(t, &t->sec_theta, (size_t)n));
    HIP_TRY(hipMemcpyAsync(t->dX, dX, (n - 1) * 8, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(t->dY, dY, (n - 1) * 8, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(t->dX2, dX2, n * 8, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(t->dY2, dY2, n * 8, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(t->rowtab, tab.data(), (n - 1) * sizeof(RowTab), hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(t->sec_theta, st.data(), n * 8, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    t->spacing_set = true;
    return 0;
}

int pydem_tile_upload(pydem_tile *t, int field, const void *src, int dtype)
{
    HIP_TRY(hipSetDevice(t->device));
    // incremental edge rounds keep the deltas of cells below unresolved inlets pending until the flush: an upload between
    // two rounds must not discard them silently (a new UCA plane replaces what they would have been added to)
    if (t->einc_ready && field != PYDEM_UCA) PYDEM_TRY(stage_edge_flush(t));
    t->edge_clean = false;
    t->einc_ready = false;
    void **pp; size_t elem;
    PYDEM_TRY(field_ptr(t, field, &pp, &elem));
    PYDEM_TRY(ensure_field(t, field));
    const size_t ds = dtype_size(dtype);
    if (!ds) { pydem_set_error("unknown dtype %d", dtype); return -2; }
    if (ds == elem && (elem == 1 || dtype == PYDEM_F64)) {
        PYDEM_TRY(tile_plane_copy(t, *pp, const_cast<void *>(src), (size_t)t->NN * elem, false));
    } else {
        if (elem != 8) { pydem_set_error("dtype conversion is only supported for float64 fields"); return -2; }
        const size_t bytes = (size_t)t->NN * ds;
        PYDEM_TRY(tile_reserve(t, &t->scratch, &t->scratch_bytes, bytes, bytes, false));
        PYDEM_TRY(tile_plane_copy(t, t->scratch, const_cast<void *>(src), bytes, false));
        const int grid = (int)(cdiv(t->NN, 256) < 8192 ? cdiv(t->NN, 256) : 8192);
        double *dst = (double *)*pp;
        switch (dtype) {
            case PYDEM_F32: hipLaunchKernelGGL(k_convert_to_f64<float>, dim3(grid), dim3(256), 0, t->stream, (const float *)t->scratch, dst, t->NN); break;
            case PYDEM_I16: hipLaunchKernelGGL(k_convert_to_f64<int16_t>, dim3(grid), dim3(256), 0, t->stream, (const int16_t *)t->scratch, dst, t->NN); break;
            case PYDEM_I32: hipLaunchKernelGGL(k_convert_to_f64<int32_t>, dim3(grid), dim3(256), 0, t->stream, (const int32_t *)t->scratch, dst, t->NN); break;
            case PYDEM_U8: hipLaunchKernelGGL(k_convert_to_f64<uint8_t>, dim3(grid), dim3(256), 0, t->stream, (const uint8_t *)t->scratch, dst, t->NN); break;
            case PYDEM_I8: hipLaunchKernelGGL(k_convert_to_f64<int8_t>, dim3(grid), dim3(256), 0, t->stream, (const int8_t *)t->scratch, dst, t->NN); break;
            default: pydem_set_error("bad dtype"); return -2;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(t->stream));
    }
    t->have[field] = true;
    if (field == PYDEM_MAG || field == PYDEM_FLATS) t->flats_state = 0;
    if (field == PYDEM_ELEV) { t->elev_f32 = (dtype == PYDEM_F32); t->elev_dtype = dtype; }
    if (field == PYDEM_ELEV || field == PYDEM_MAG || field == PYDEM_DIRECTION || field == PYDEM_FLATS) tile_graph_drop(t);
    return 0;
}

int pydem_tile_download(pydem_tile *t, int field, void *dst)
{
    HIP_TRY(hipSetDevice(t->device));
    void **pp; size_t elem;
    PYDEM_TRY(field_ptr(t, field, &pp, &elem));
    if (!*pp || !t->have[field]) { pydem_set_error("field %d has not been computed or uploaded", field); return -3; }
    if (field == PYDEM_UCA) PYDEM_TRY(stage_edge_flush(t));     // incremental edge rounds: settle what is still waiting upstream
    if (field == PYDEM_EDGE_DONE || field == PYDEM_EDGE_TODO) PYDEM_TRY(stage_edge_catchup(t));   // condensed rounds: the interior masks catch up
    PYDEM_TRY(tile_plane_copy(t, *pp, dst, (size_t)t->NN * elem, true));
    return 0;
}

// one row (axis 0) or one column (axis 1) of a field: the strips the directory flow exchanges
// between neighbouring tiles (reference process_manager.py:131-145, :252-255).  Columns are
// gathered / scattered by a kernel through a contiguous staging buffer (a strided 2-D memcpy of
// 1- or 8-byte rows costs one DMA descriptor per element).
static int line_copy(pydem_tile *t, int field, int axis, int64_t index, void *host, bool to_host)
{
    HIP_TRY(hipSetDevice(t->device));
    void **pp; size_t elem;
    PYDEM_TRY(field_ptr(t, field, &pp, &elem));
    if (!*pp || !t->have[field]) { pydem_set_error("field %d has not been computed or uploaded", field); return -3; }
    const int64_t lim = axis == 0 ? t->n : t->m;
    if (index < 0) index += lim;
    if (index < 0 || index >= lim || (axis != 0 && axis != 1)) { pydem_set_error("line index out of range"); return -2; }
    if (!to_host && (field == PYDEM_MAG || field == PYDEM_FLATS)) t->flats_state = 0;
    if (to_host && (field == PYDEM_UCA || field == PYDEM_EDGE_DONE || field == PYDEM_EDGE_TODO) && !tile_line_watched(t, axis, index))
        PYDEM_TRY(stage_edge_catchup(t));                       // condensed edge rounds only keep the watched lines current
    char *base = (char *)*pp;
    // the caller's array is pageable: the transfer goes through the tile's pinned staging buffer (tile_pinned)
    const size_t nbytes = (size_t)(axis == 0 ? t->m : t->n) * elem;
    void *pin = nullptr;
    PYDEM_TRY(tile_pinned(t, nbytes, &pin));
    void *user = host;
    host = pin;
    if (!to_host) memcpy(pin, user, nbytes);
    if (axis == 0) {
        char *row = base + (size_t)index * t->m * elem;
        if (to_host) HIP_TRY(hipMemcpyAsync(host, row, (size_t)t->m * elem, hipMemcpyDeviceToHost, t->stream));
        else HIP_TRY(hipMemcpyAsync(row, host, (size_t)t->m * elem, hipMemcpyHostToDevice, t->stream));
    } else {
        const int64_t cnt = t->n;
        PYDEM_TRY(tile_alloc(t, &t->line_stage, (size_t)(t->n > t->m ? t->n : t->m)));
        const int g = (int)(cdiv(cnt, 256) < 64 ? cdiv(cnt, 256) : 64);
        char *col = base + (size_t)index * elem;
        if (to_host) {
            if (elem == 8) hipLaunchKernelGGL(k_line_gather<double>, dim3(g), dim3(256), 0, t->stream, (const double *)col, t->m, cnt, t->line_stage);
            else hipLaunchKernelGGL(k_line_gather<uint8_t>, dim3(g), dim3(256), 0, t->stream, (const uint8_t *)col, t->m, cnt, (uint8_t *)t->line_stage);
            HIP_TRY(hipMemcpyAsync(host, t->line_stage, (size_t)cnt * elem, hipMemcpyDeviceToHost, t->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(t->line_stage, host, (size_t)cnt * elem, hipMemcpyHostToDevice, t->stream));
            if (elem == 8) hipLaunchKernelGGL(k_line_scatter<double>, dim3(g), dim3(256), 0, t->stream, (const double *)t->line_stage, t->m, cnt, (double *)col);
            else hipLaunchKernelGGL(k_line_scatter<uint8_t>, dim3(g), dim3(256), 0, t->stream, (const uint8_t *)t->line_stage, t->m, cnt, (uint8_t *)col);
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(t->stream));
    if (to_host) memcpy(user, pin, nbytes);
    if (!to_host && (field == PYDEM_ELEV || field == PYDEM_MAG || field == PYDEM_DIRECTION || field == PYDEM_FLATS)) tile_graph_drop(t);
    if (!to_host && (field == PYDEM_MAG || field == PYDEM_FLATS)) t->flats_state = 0;
    return 0;
}

int pydem_tile_get_line(pydem_tile *t, int field, int axis, int64_t index, void *dst) { return line_copy(t, field, axis, index, dst, true); }

// several lines with ONE synchronisation (an edge round of the directory flow reads ~14 strips of the
// tile that just ran; one launch + copy + sync per strip is ~30 us each)
int pydem_tile_get_lines(pydem_tile *t, int count, const int *fields, const int *axes, const int64_t *indices, void *const *dsts)
{
    HIP_TRY(hipSetDevice(t->device));
    const size_t L = (size_t)(t->n > t->m ? t->n : t->m);
    if (count > 0) PYDEM_TRY(tile_reserve(t, &t->lines_stage, &t->lines_bytes, (size_t)count * L * 8, (size_t)(count < 16 ? 16 : count) * L * 8, false));
    void *pin_v = nullptr;                                  // (pinned staging: the callers' arrays are pageable)
    PYDEM_TRY(tile_pinned(t, (size_t)(count > 0 ? count : 1) * L * 8, &pin_v));
    char *pin = (char *)pin_v;
    std::vector<size_t> nbytes((size_t)(count > 0 ? count : 0));
    for (int k = 0; k < count; k++) {
        void **pp; size_t elem;
        PYDEM_TRY(field_ptr(t, fields[k], &pp, &elem));
        if (!*pp || !t->have[fields[k]]) { pydem_set_error("field %d has not been computed or uploaded", fields[k]); return -3; }
        const int64_t lim = axes[k] == 0 ? t->n : t->m;
        int64_t index = indices[k];
        if (index < 0) index += lim;
        if (index < 0 || index >= lim || (axes[k] != 0 && axes[k] != 1)) { pydem_set_error("line index out of range"); return -2; }
        if ((fields[k] == PYDEM_UCA || fields[k] == PYDEM_EDGE_DONE || fields[k] == PYDEM_EDGE_TODO) && !tile_line_watched(t, axes[k], index))
            PYDEM_TRY(stage_edge_catchup(t));
        char *base = (char *)*pp;
        if (axes[k] == 0) {
            nbytes[(size_t)k] = (size_t)t->m * elem;
            HIP_TRY(hipMemcpyAsync(pin + (size_t)k * L * 8, base + (size_t)index * t->m * elem, (size_t)t->m * elem, hipMemcpyDeviceToHost, t->stream));
        } else {
            const int64_t cnt = t->n;
            const int g = (int)(cdiv(cnt, 256) < 64 ? cdiv(cnt, 256) : 64);
            char *col = base + (size_t)index * elem;
            double *stage = (double *)t->lines_stage + (size_t)k * L;
            if (elem == 8) hipLaunchKernelGGL(k_line_gather<double>, dim3(g), dim3(256), 0, t->stream, (const double *)col, t->m, cnt, stage);
            else hipLaunchKernelGGL(k_line_gather<uint8_t>, dim3(g), dim3(256), 0, t->stream, (const uint8_t *)col, t->m, cnt, (uint8_t *)stage);
            nbytes[(size_t)k] = (size_t)cnt * elem;
            HIP_TRY(hipMemcpyAsync(pin + (size_t)k * L * 8, stage, (size_t)cnt * elem, hipMemcpyDeviceToHost, t->stream));
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    for (int k = 0; k < count; k++) memcpy(dsts[k], pin + (size_t)k * L * 8, nbytes[(size_t)k]);
    return 0;
}
int pydem_tile_set_line(pydem_tile *t, int field, int axis, int64_t index, const void *src) { return line_copy(t, field, axis, index, (void *)src, false); }

int pydem_tile_synchronize(pydem_tile *t)
{
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

int pydem_tile_timings(pydem_tile *t, pydem_timings *out) { *out = t->tm; return 0; }
int64_t pydem_tile_device_bytes(pydem_tile *t) { return t->device_bytes; }

int pydem_tile_synth_fractal(pydem_tile *t, uint32_t seed, int64_t row0, int64_t col0, int n_octaves,
                             int top_shift, double zmin, double zrange)
{
    HIP_TRY(hipSetDevice(t->device));
    tile_graph_drop(t);
    t->flats_state = 0;
    PYDEM_TRY(ensure_field(t, PYDEM_ELEV));
    PYDEM_TRY(stage_synth(t, seed, row0, col0, n_octaves, top_shift, zmin, zrange));
    t->have[PYDEM_ELEV] = true;
    t->elev_f32 = false; t->elev_dtype = PYDEM_F64;
    for (int f = PYDEM_MAG; f < PYDEM_FIELD_COUNT; f++) t->have[f] = false;
    return 0;
}

static int need(pydem_tile *t, int field, const char *what)
{
    if (!t->have[field]) { pydem_set_error("%s: required input field %d is missing", what, field); return -3; }
    return 0;
}

int pydem_slopes_directions(pydem_tile *t)
{
    HIP_TRY(hipSetDevice(t->device));
    if (t->einc_ready) PYDEM_TRY(stage_edge_flush(t));      // (the resident UCA plane survives this stage: pending deltas first)
    t->edge_clean = false;      // these stages reuse the edge-round work lists
    t->einc_ready = false;
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_slopes_directions"));
    if (!t->spacing_set) { pydem_set_error("pydem_slopes_directions: call pydem_tile_set_spacing first"); return -3; }
    PYDEM_TRY(ensure_fields(t, {PYDEM_MAG, PYDEM_DIRECTION, PYDEM_FLATS}));
    PYDEM_TRY(tile_alloc(t, &t->flat0, (size_t)t->NN));
    tile_graph_drop(t);
    t->flats_state = 0;
    PYDEM_TRY(stage_stencil(t));
    PYDEM_TRY(stage_flats(t));          // (leaves flats_state 1 when flats == (mag == -1) is known to hold)
    t->have[PYDEM_MAG] = t->have[PYDEM_DIRECTION] = t->have[PYDEM_FLATS] = true;
    return 0;
}

int pydem_fill_flats(pydem_tile *t, double max_pit_area, int below_sea, double source_tol, int peaks, int pits, int artefacts_only,
                     int *needs_host)
{
    t->edge_clean = false;
    t->einc_ready = false;
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_fill_flats"));
    tile_graph_drop(t);
    t->flats_state = 0;                 // (mag and the other planes are work planes of the conditioning)
    const int r = stage_fill_flats(t, max_pit_area, below_sea, source_tol, peaks, pits, artefacts_only);
    if (r < 0) return r;
    if (needs_host) *needs_host = r;
    for (int f = PYDEM_MAG; f < PYDEM_FIELD_COUNT; f++) t->have[f] = false;     // the work planes of the conditioning
    return 0;
}

int pydem_fill_depressions(pydem_tile *t, double *epsilon, const uint8_t *outlets, double *depth, int64_t *n_raised, double *max_depth,
                           int64_t *passes, double *ms)
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_fill_depressions"));
    if (!epsilon) { pydem_set_error("pydem_fill_depressions: epsilon is NULL"); return -2; }
    if (t->einc_ready) PYDEM_TRY(stage_edge_flush(t));      // (pending deltas of the incremental edge rounds belong to the surface as it is)
    // bad arguments and the pass limit leave the surface, and everything computed from it, as they were
    PYDEM_TRY(stage_fill_depressions(t, epsilon, outlets, depth, n_raised, max_depth, passes, ms));
    t->edge_clean = false;
    t->einc_ready = false;
    tile_graph_drop(t);
    t->flats_state = 0;
    for (int f = PYDEM_MAG; f < PYDEM_FIELD_COUNT; f++) t->have[f] = false;     // as after the other conditioning stages
    return 0;
}

// the fill across tiles: a session on the tile (fill_depressions.hip)
int pydem_fill_seam_begin(pydem_tile *t, const uint8_t *outlets, const uint8_t *seam_top, const uint8_t *seam_bottom, const uint8_t *seam_left,
                          const uint8_t *seam_right, double *amax)
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_fill_seam_begin"));
    const uint8_t *const seam[4] = {seam_top, seam_bottom, seam_left, seam_right};
    return stage_fill_seam_begin(t, outlets, seam, amax);
}

int pydem_fill_seam_relax(pydem_tile *t, double eps, const double *cap_top, const double *cap_bottom, const double *cap_left,
                          const double *cap_right, int64_t *n_lowered, int64_t *passes, double *ms)
{
    HIP_TRY(hipSetDevice(t->device));
    const double *const caps[4] = {cap_top, cap_bottom, cap_left, cap_right};
    return stage_fill_seam_relax(t, eps, caps, n_lowered, passes, ms);
}

int pydem_fill_seam_get_lines(pydem_tile *t, int count, const int *axes, const int64_t *indices, void *const *dsts)
{
    HIP_TRY(hipSetDevice(t->device));
    return stage_fill_seam_get_lines(t, count, axes, indices, dsts);
}

int pydem_fill_seam_end(pydem_tile *t, int commit, double *depth, int64_t *n_raised, double *max_depth)
{
    HIP_TRY(hipSetDevice(t->device));
    if (!commit) return stage_fill_seam_end(t, 0, nullptr, nullptr, nullptr);      // nothing of the tile but the session changes
    if (t->fs_open && t->einc_ready) PYDEM_TRY(stage_edge_flush(t));   // (pending deltas of the incremental edge rounds belong to the surface as it is)
    const int rc = stage_fill_seam_end(t, 1, depth, n_raised, max_depth);
    if (rc == -2 || rc == -5) return rc;            // refused: the surface is what it was
    t->edge_clean = false;
    t->einc_ready = false;
    tile_graph_drop(t);
    t->flats_state = 0;
    for (int f = PYDEM_MAG; f < PYDEM_FIELD_COUNT; f++) t->have[f] = false;     // as after pydem_fill_depressions
    return rc;
}

// the session's inventory part (depressions.hip): these read the elevation and the session's W and change nothing else of the tile
int pydem_fill_seam_label(pydem_tile *t, int64_t *n_local, double *max_depth, double *ms)
{
    HIP_TRY(hipSetDevice(t->device));
    return stage_fill_seam_label(t, n_local, max_depth, ms);
}

int pydem_fill_seam_label_roots(pydem_tile *t, int64_t count, int32_t *roots, double *levels)
{
    return stage_fill_seam_label_roots(t, count, roots, levels);
}

int pydem_fill_seam_get_id_lines(pydem_tile *t, int count, const int *axes, const int64_t *indices, void *const *dsts)
{
    HIP_TRY(hipSetDevice(t->device));
    return stage_fill_seam_get_id_lines(t, count, axes, indices, dsts);
}

int pydem_fill_seam_inventory(pydem_tile *t, const int32_t *lut, int64_t n_rows, const uint8_t *owner, const uint8_t *outlets,
                              const int32_t *halo_ids, const double *halo_W, const double *row_area, int shift_area, int shift_volume,
                              uint64_t *table, double *ms)
{
    HIP_TRY(hipSetDevice(t->device));
    return stage_fill_seam_inventory(t, lut, n_rows, owner, outlets, halo_ids, halo_W, row_area, shift_area, shift_volume, table, ms);
}

int pydem_fill_seam_labels(pydem_tile *t, const int32_t *lut, int32_t *label, double *ms)
{
    HIP_TRY(hipSetDevice(t->device));
    return stage_fill_seam_labels(t, lut, label, ms);
}

int pydem_depressions(pydem_tile *t, const uint8_t *outlets, double min_depth, int64_t min_cells, double min_volume, int32_t *label,
                      int64_t *n_found, int64_t *n_kept, double *quanta, int64_t *passes, double *ms)
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_depressions"));
    t->depr.clear();
    // reads the elevation and nothing else of the tile: no field, flag or pending edge delta changes
    return stage_depressions(t, outlets, min_depth, min_cells, min_volume, label, n_found, n_kept, quanta, passes, ms);
}

int pydem_depressions_table(pydem_tile *t, int64_t rows, pydem_depression *table)
{
    if (rows != (int64_t)t->depr.size() || (rows > 0 && !table)) {
        pydem_set_error("pydem_depressions_table: %lld rows asked, the last pydem_depressions kept %lld", (long long)rows, (long long)t->depr.size());
        return -2;
    }
    if (rows > 0) memcpy(table, t->depr.data(), (size_t)rows * sizeof(pydem_depression));
    return 0;
}

int pydem_hand_table(pydem_tile *t, const int32_t *zone, const double *hand, const double *stages, int64_t n_stages, int64_t n_zones,
                     int64_t *table, int64_t *skipped, double *quanta, double *ms)
{
    if (!t) { pydem_set_error("pydem_hand_table: no tile"); return -2; }
    HIP_TRY(hipSetDevice(t->device));
    // reads the slope, the spacing and (without a HAND plane) the result plane of pydem_dist_down: no field, flag or timing changes
    return stage_hand_table(t, zone, hand, stages, n_stages, n_zones, table, skipped, quanta, ms);
}

int pydem_terrain_attributes(pydem_tile *t, int half_width, const double *light, double z_factor, double *const *outs, double *ms,
                             int64_t *n_defined)
{
    if (!t) { pydem_set_error("pydem_terrain_attributes: no tile"); return -2; }
    HIP_TRY(hipSetDevice(t->device));
    // reads the elevation and the spacing: no field, flag or timing changes
    return stage_terrain_attributes(t, half_width, light, z_factor, outs, ms, n_defined);
}

int pydem_horizon(pydem_tile *t, int n_dir, const int32_t *start, const int16_t *dr, const int16_t *dc, const double *w, int edge_nan,
                  double *const *horizon, double *svf, double *ms, int64_t *n_defined)
{
    if (!t) { pydem_set_error("pydem_horizon: no tile"); return -2; }
    HIP_TRY(hipSetDevice(t->device));
    // reads the elevation: no field, flag or timing changes
    return stage_horizon(t, n_dir, start, dr, dc, w, edge_nan, horizon, svf, ms, n_defined);
}

int pydem_pit_candidates(pydem_tile *t, int below_sea, int64_t *npits)
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_pit_candidates"));
    t->flats_state = 0;
    return stage_pit_candidates(t, below_sea, npits);
}

int pydem_pit_candidates_read(pydem_tile *t, int64_t npits, int32_t *cells, double *elev)
{
    HIP_TRY(hipSetDevice(t->device));
    return stage_pit_candidates_read(t, npits, cells, elev);
}

int pydem_pit_paths(pydem_tile *t, const int32_t *order, int64_t npits, int max_iter, int max_dist, double max_dist_XY,
                    int64_t *n_failed, int64_t *iter_used, int64_t *rounds, int *needs_host)
{
    t->edge_clean = false;
    t->einc_ready = false;
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_pit_paths"));
    // the path values get the dtype of the array the reference edits (:539): integer surfaces truncate them, float32 ones round
    const int dtype_mode = t->elev_dtype == PYDEM_F64 ? 0 : (t->elev_dtype == PYDEM_F32 ? 2 : 1);
    tile_graph_drop(t);
    t->flats_state = 0;
    const int r = stage_pit_paths(t, order, npits, max_iter, max_dist, max_dist_XY, n_failed, iter_used, rounds, dtype_mode);
    if (r < 0) return r;
    if (needs_host) *needs_host = r;
    for (int f = PYDEM_MAG; f < PYDEM_FIELD_COUNT; f++) t->have[f] = false;
    return 0;
}

int pydem_find_flats(pydem_tile *t)
{
    t->edge_clean = false;      // these stages reuse the edge-round work lists
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_MAG, "pydem_find_flats"));
    const bool had_flats = t->flats != nullptr;
    PYDEM_TRY(ensure_field(t, PYDEM_FLATS));
    const bool lean = step_lean();
    // Only the work the result needs (flats_state, internal.h).  Nothing on the host reads the result, and the stream orders
    // what follows: no wait.
    if (lean && had_flats && t->have[PYDEM_FLATS] && t->flats_state == 1) {
        t->find_flats_elided++;
    } else if (lean && had_flats && t->have[PYDEM_FLATS] && t->flats_state == 2) {
        if (t->pits.n_raw > 0) {
            const int64_t g = cdiv(t->pits.n_raw, 256);
            hipLaunchKernelGGL(k_find_flats_pits, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, t->stream,
                               (const int32_t *)t->pits.raw_src, t->pits.n_raw, t->flats);
            HIP_TRY(hipGetLastError());
        }
        t->find_flats_patch++;
    } else {
        const int grid = (int)(cdiv(t->NN, 256) < 8192 ? cdiv(t->NN, 256) : 8192);
        hipLaunchKernelGGL(k_find_flats, dim3(grid), dim3(256), 0, t->stream, t->mag, t->flats, t->NN);
        HIP_TRY(hipGetLastError());
        if (!lean) HIP_TRY(hipStreamSynchronize(t->stream));
        t->find_flats_full++;
    }
    t->flats_state = 1;
    t->have[PYDEM_FLATS] = true;
    return 0;
}

int pydem_uca(pydem_tile *t, pydem_options *opt)
{
    t->edge_clean = false;      // these stages reuse the edge-round work lists
    t->einc_ready = false;
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_uca"));
    PYDEM_TRY(need(t, PYDEM_MAG, "pydem_uca"));
    PYDEM_TRY(need(t, PYDEM_DIRECTION, "pydem_uca"));
    PYDEM_TRY(need(t, PYDEM_FLATS, "pydem_uca"));
    if (!t->spacing_set) { pydem_set_error("pydem_uca: call pydem_tile_set_spacing first"); return -3; }
    PYDEM_TRY(ensure_fields(t, {PYDEM_SECTION, PYDEM_PROPORTION, PYDEM_UCA, PYDEM_EDGE_TODO, PYDEM_EDGE_DONE}));
    // the area plane is free from here to the sweep: the graph stage may leave the pit offsets in it (uca.hip: k_graph_add_pits)
    t->pit_stash_live = step_lean();
    {
        const int rc = stage_section_graph(t, opt);
        if (rc != 0) { t->pit_stash_live = false; return rc; }
    }
    t->graph_valid = true;
    {
        const int rc = stage_sweep(t, opt);
        t->pit_stash_live = false;
        if (rc != 0) return rc;
    }
    // record minimum area (dem_processing.py:897-899)
    double mn = opt->twi_min_area;
    for (int64_t i = 0; i < t->n; i++) {
        const double a = t->h_dX2[(size_t)i] * t->h_dY2[(size_t)i];
        if (a < mn) mn = a;
    }
    opt->twi_min_area = mn;
    t->have[PYDEM_SECTION] = t->have[PYDEM_PROPORTION] = t->have[PYDEM_UCA] = true;
    t->have[PYDEM_EDGE_TODO] = t->have[PYDEM_EDGE_DONE] = true;
    return 0;
}

// a tile rebuilt from stored elev / aspect / slope (process_manager.calc_uca_ec :227-240, or a resumed directory job):
// the flow graph is built once, the first time an edge round needs it
static int ensure_graph(pydem_tile *t, pydem_options *opt, const char *who)
{
    if (t->graph_valid) return 0;
    PYDEM_TRY(need(t, PYDEM_ELEV, who));
    PYDEM_TRY(need(t, PYDEM_MAG, who));
    PYDEM_TRY(need(t, PYDEM_DIRECTION, who));
    if (!t->spacing_set) { pydem_set_error("%s: call pydem_tile_set_spacing first", who); return -3; }
    PYDEM_TRY(ensure_fields(t, {PYDEM_SECTION, PYDEM_PROPORTION}));
    t->pit_stash_live = false;          // (the area plane holds the tile's uca on this path: the sweeps stash on their own)
    PYDEM_TRY(stage_section_graph(t, opt));
    t->graph_valid = true;
    t->have[PYDEM_SECTION] = t->have[PYDEM_PROPORTION] = true;
    return 0;
}

// the options the graph stage reads (pydem_uca with other values would build another graph)
static bool same_graph_options(const pydem_options &a, const pydem_options &b)
{
    if (!a.drain_pits && !b.drain_pits) return true;
    const bool xy = (a.drain_pits_max_dist_XY == b.drain_pits_max_dist_XY) ||
                    (a.drain_pits_max_dist_XY != a.drain_pits_max_dist_XY && b.drain_pits_max_dist_XY != b.drain_pits_max_dist_XY);
    return a.drain_pits == b.drain_pits && a.drain_pits_min_border == b.drain_pits_min_border &&
           a.drain_pits_max_iter == b.drain_pits_max_iter && a.drain_pits_max_dist == b.drain_pits_max_dist && xy;
}

int pydem_uca_weighted(pydem_tile *t, pydem_options *opt, int scale_by_cell_area)
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_WEIGHT, "pydem_uca_weighted"));
    const pydem_timings keep = t->tm;   // pydem_uca's timings, the graph stage's included, are put back at the end
    // The tile's flow graph when it is the one pydem_uca would build now; otherwise the graph stage runs here.  That stage patches
    // the drained pits into mag / flats (:1369-1371), which the finalisation reads; the planes are put back afterwards (exactly:
    // the patched cells are flat cells, saved with their slopes beforehand, 12 bytes per flat cell) and the graph is dropped
    // (graph_valid pairs a graph with the PATCHED planes, as pydem_uca leaves them), so every call on such a tile starts from
    // the same surface and a later pydem_uca / edge round builds its own graph.
    const bool own_graph = !t->graph_valid || !same_graph_options(t->graph_opt, *opt);
    DevTemp save, planes;
    struct Kept { void *dst; size_t bytes; size_t off; };
    std::vector<Kept> kept;             // resident results the graph stage overwrites (a tile where pydem_uca ran with other options)
    int32_t *save_cells = nullptr;
    double *save_vals = nullptr;
    int64_t nsave = 0;
    if (own_graph) {
        PYDEM_TRY(need(t, PYDEM_FLATS, "pydem_uca_weighted"));
        PYDEM_TRY(need(t, PYDEM_MAG, "pydem_uca_weighted"));
        PYDEM_TRY(ensure_fields(t, {PYDEM_EDGE_TODO, PYDEM_EDGE_DONE}));
        unsigned long long *cnt = reinterpret_cast<unsigned long long *>(t->counters + CS_FLAT_SAVE);
        const int g = (int)(cdiv(t->NN, 256) < 4096 ? cdiv(t->NN, 256) : 4096);
        HIP_TRY(hipMemsetAsync(cnt, 0, 8, t->stream));
        hipLaunchKernelGGL(k_flat_save, dim3(g), dim3(256), 0, t->stream, (const uint8_t *)t->flats, (const double *)t->mag, t->NN,
                           (int32_t *)nullptr, (double *)nullptr, (int64_t)0, cnt);
        unsigned long long hn = 0;
        HIP_TRY(hipMemcpyAsync(&hn, cnt, 8, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        nsave = (int64_t)hn;
        if (nsave > 0) {
            PYDEM_TRY(save.alloc((size_t)nsave * 12));
            save_vals = (double *)save.p;
            save_cells = (int32_t *)((char *)save.p + (size_t)nsave * 8);
            HIP_TRY(hipMemsetAsync(cnt, 0, 8, t->stream));
            hipLaunchKernelGGL(k_flat_save, dim3(g), dim3(256), 0, t->stream, (const uint8_t *)t->flats, (const double *)t->mag, t->NN,
                               save_cells, save_vals, nsave, cnt);
            HIP_TRY(hipGetLastError());
        }
        size_t off = 0;
        if (t->have[PYDEM_SECTION]) { kept.push_back({t->section, (size_t)t->NN, off}); off += (size_t)t->NN; }
        if (t->have[PYDEM_EDGE_TODO]) { kept.push_back({t->edge_todo, (size_t)t->NN, off}); off += (size_t)t->NN; }
        off = (off + 255) & ~(size_t)255;
        if (t->have[PYDEM_PROPORTION]) { kept.push_back({t->prop, (size_t)t->NN * 8, off}); off += (size_t)t->NN * 8; }
        if (off) PYDEM_TRY(planes.alloc(off));
        for (const Kept &k : kept)
            HIP_TRY(hipMemcpyAsync((char *)planes.p + k.off, k.dst, k.bytes, hipMemcpyDeviceToDevice, t->stream));
        tile_graph_drop(t);
    }
    int rc = own_graph ? ensure_graph(t, opt, "pydem_uca_weighted") : 0;
    if (rc == 0) {
        // (incremental edge rounds keep their state in the planes the sweep works in.  The upload of PYDEM_WEIGHT that every call
        // needs has settled and dropped that state already; this is for a caller that reaches here otherwise)
        if (t->einc_ready) rc = stage_edge_flush(t);
        t->einc_ready = false;
    }
    if (rc == 0) rc = ensure_field(t, PYDEM_UCA_WEIGHTED);
    if (rc == 0) rc = stage_uca_weighted(t, opt, scale_by_cell_area);
    t->have[PYDEM_WEIGHT] = false;      // the plane holds the seeds now: the next call needs the weights again
    const double w_ms = t->tm.uca_weighted_ms;
    t->tm = keep;
    if (rc == 0) t->tm.uca_weighted_ms = w_ms;
    if (own_graph) {
        if (nsave > 0) {
            const int64_t g = cdiv(nsave, 256);
            hipLaunchKernelGGL(k_flat_restore, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, t->stream, (const int32_t *)save_cells,
                               (const double *)save_vals, nsave, t->mag, t->flats);
        }
        for (const Kept &k : kept)
            HIP_TRY(hipMemcpyAsync(k.dst, (char *)planes.p + k.off, k.bytes, hipMemcpyDeviceToDevice, t->stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(t->stream));
        tile_graph_drop(t);
    }
    if (own_graph) t->flats_state = 0;      // (the graph stage patched mag / flats and they were written back: nothing is claimed about them)
    if (rc != 0) return rc;
    t->have[PYDEM_UCA_WEIGHTED] = true;
    return 0;
}

int pydem_build_graph(pydem_tile *t, pydem_options *opt)
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_FLATS, "pydem_build_graph"));
    PYDEM_TRY(ensure_fields(t, {PYDEM_EDGE_TODO, PYDEM_EDGE_DONE}));
    return ensure_graph(t, opt, "pydem_build_graph");
}

int pydem_uca_edge_update(pydem_tile *t, pydem_options *opt, const double *const data[4],
                          const uint8_t *const done[4], const uint8_t *const todo[4])
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_UCA, "pydem_uca_edge_update"));
    PYDEM_TRY(need(t, PYDEM_FLATS, "pydem_uca_edge_update"));
    PYDEM_TRY(ensure_fields(t, {PYDEM_EDGE_TODO, PYDEM_EDGE_DONE}));
    PYDEM_TRY(ensure_graph(t, opt, "pydem_uca_edge_update"));
    PYDEM_TRY(stage_edge_update(t, opt, data, done, todo));
    t->have[PYDEM_EDGE_TODO] = t->have[PYDEM_EDGE_DONE] = true;
    return 0;
}

int pydem_uca_edge_round_inc(pydem_tile *t, pydem_options *opt, const double *const data[4],
                             const uint8_t *const done[4], const uint8_t *const todo[4])
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_UCA, "pydem_uca_edge_round_inc"));
    PYDEM_TRY(need(t, PYDEM_FLATS, "pydem_uca_edge_round_inc"));
    PYDEM_TRY(need(t, PYDEM_EDGE_TODO, "pydem_uca_edge_round_inc"));
    PYDEM_TRY(need(t, PYDEM_EDGE_DONE, "pydem_uca_edge_round_inc"));
    PYDEM_TRY(ensure_graph(t, opt, "pydem_uca_edge_round_inc"));
    PYDEM_TRY(stage_edge_round_inc(t, opt, data, done, todo));
    return 0;
}

int pydem_uca_edge_round_inc_dev(pydem_tile *t, pydem_options *opt)
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_UCA, "pydem_uca_edge_round_inc_dev"));
    PYDEM_TRY(need(t, PYDEM_FLATS, "pydem_uca_edge_round_inc_dev"));
    PYDEM_TRY(need(t, PYDEM_EDGE_TODO, "pydem_uca_edge_round_inc_dev"));
    PYDEM_TRY(need(t, PYDEM_EDGE_DONE, "pydem_uca_edge_round_inc_dev"));
    PYDEM_TRY(ensure_graph(t, opt, "pydem_uca_edge_round_inc_dev"));
    if (!t->s_data || !t->s_flags) { pydem_set_error("pydem_uca_edge_round_inc_dev: no strips (pydem_board_set_desc + pydem_board_eval first)"); return -3; }
    PYDEM_TRY(stage_edge_round_inc(t, opt, nullptr, nullptr, nullptr));
    return 0;
}

int pydem_uca_edge_flush(pydem_tile *t)
{
    HIP_TRY(hipSetDevice(t->device));
    return stage_edge_flush(t);
}

int pydem_twi(pydem_tile *t, pydem_options *opt)
{
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(stage_edge_flush(t));
    PYDEM_TRY(need(t, PYDEM_UCA, "pydem_twi"));
    PYDEM_TRY(need(t, PYDEM_MAG, "pydem_twi"));
    PYDEM_TRY(ensure_field(t, PYDEM_TWI));
    PYDEM_TRY(stage_twi(t, opt));
    t->have[PYDEM_TWI] = true;
    return 0;
}

int pydem_tile_pit_edges(pydem_tile *t, int64_t *n, int32_t *src, int32_t *dst, double *w)
{
    HIP_TRY(hipSetDevice(t->device));
    const int64_t nr = t->pits.n_raw;          // slots handed out, including unused ones (src == -1)
    std::vector<int32_t> hs((size_t)nr), hd((size_t)nr);
    std::vector<double> hw((size_t)nr);
    if (nr) {
        HIP_TRY(hipMemcpyAsync(hs.data(), t->pits.raw_src, nr * 4, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipMemcpyAsync(hd.data(), t->pits.raw_dst, nr * 4, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipMemcpyAsync(hw.data(), t->pits.raw_w, nr * 8, hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
    }
    int64_t k = 0;
    for (int64_t e = 0; e < nr; e++) {
        if (hs[(size_t)e] < 0) continue;
        if (src) { src[k] = hs[(size_t)e]; dst[k] = hd[(size_t)e]; w[k] = hw[(size_t)e]; }
        k++;
    }
    *n = k;
    return 0;
}

// the static half of the packed graph word of every cell (layout: uca_graph.h)
int pydem_tile_graph_words(pydem_tile *t, uint32_t *out)
{
    HIP_TRY(hipSetDevice(t->device));
    if (!t->graph_valid || !t->cinfo) { pydem_set_error("pydem_tile_graph_words: no flow graph on this tile (pydem_uca / pydem_build_graph first)"); return -3; }
    HIP_TRY(hipMemcpyAsync(out, t->cinfo, (size_t)t->NN * 4, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    for (int64_t c = 0; c < t->NN; c++) out[c] &= CI_STATIC_MASK;
    return 0;
}

int pydem_tile_restore_pit_slopes(pydem_tile *t)
{
    t->edge_clean = false;      // these stages reuse the edge-round work lists
    HIP_TRY(hipSetDevice(t->device));
    if (t->pits.n_raw == 0) return 0;
    // mag becomes -1 at the listed pits and flats is left alone (callers read it between this call and the next pydem_find_flats):
    // behind a state 1 the mask then differs from mag == -1 at those cells only, and only where it holds 0 -- state 2, whatever the
    // list is; from any other state nothing is known
    t->flats_state = (t->flats_state == 1) ? 2 : 0;
    const int64_t g = cdiv(t->pits.n_raw, 256);
    hipLaunchKernelGGL(k_restore_pit_slopes, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, t->stream, t->pits.raw_src,
                       t->pits.n_raw, t->mag);
    HIP_TRY(hipGetLastError());
    if (!step_lean()) HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

int pydem_tile_flats_state(pydem_tile *t, int *state, int64_t *counts)
{
    if (state) *state = t->flats_state;
    if (counts) { counts[0] = t->find_flats_full; counts[1] = t->find_flats_patch; counts[2] = t->find_flats_elided; }
    return 0;
}

int pydem_bench_stencil(pydem_tile *t, int iters, double *avg_ms)
{
    t->edge_clean = false;      // these stages reuse the edge-round work lists
    t->einc_ready = false;
    HIP_TRY(hipSetDevice(t->device));
    PYDEM_TRY(need(t, PYDEM_ELEV, "pydem_bench_stencil"));
    if (!t->spacing_set) { pydem_set_error("pydem_bench_stencil: call pydem_tile_set_spacing first"); return -3; }
    PYDEM_TRY(ensure_fields(t, {PYDEM_MAG, PYDEM_DIRECTION}));
    PYDEM_TRY(tile_alloc(t, &t->flat0, (size_t)t->NN));
    t->flats_state = 0;                 // (the stencil rewrites mag without the flats stage behind it)
    return bench_stencil(t, iters, avg_ms);
}

}  // extern "C"
