// flowdist.h -- what the two sweeps of a path statistic over the tile's flow graph share: the reverse one (flowdist.hip,
// pydem_dist_down) and the forward one (flowdist_up.hip, pydem_dist_up).  The encoding of an open cell in the result plane,
// the argument block, the counter words, the wave-aggregated queue append, the accumulator of a cell's edges with its fixed
// operand order, the edge cost, and the three small kernels both schedules use.  The reverse accumulation (flowacc_rev.hip,
// pydem_rev_accum) is a third sweep on the same state and schedule; with the reverse distance it shares the part of the queue
// that depends on the graph alone (dd_release, k_dd_recount).  One call at a time owns the state (pydem_tile::dd_*): a call
// overwrites the others' device result.
#pragma once
#include "uca_graph.h"
#include <math.h>

namespace {

constexpr uint32_t DD_OPEN_HI = 0x7FFDD000u;
constexpr int DD_BATCH = 16;
constexpr int DD_T = 32, DD_H = DD_T + 2;       // tile edge, tile + halo
constexpr int DD_MAX_PASSES = 4096;
constexpr int64_t DD_MIN_PER_VISIT = 16;        // cells a tile visit of the reverse sweep has to finish on average for another pass to beat the queue
constexpr int32_t DD_STAMP_OPEN = INT32_MAX;
constexpr uint16_t DD_FL_OPEN = 0xFFFFu;
// words of the call's counter block; behind it four words per tile: open cells after its last visit, for each parity of the
// pass number the last pass of that parity in which it finished something, cells finished by its visit of the current pass
enum : int { DD_LO = 0, DD_HI = 1, DD_TAIL = 2, DD_LEVELS = 3, DD_NOPEN = 4 /* 64-bit: [4..5] */, DD_PASSDONE = 6 /* 64-bit: [6..7] */,
             DD_VISITS = 8, DD_WORDS = 16 };

struct DistArgs {
    const uint32_t *cinfo;
    const double *prop, *elev, *dX2, *dY2;
    double *D;
    int32_t *queue;
    uint8_t *mask;
    const int32_t *pit_src, *pit_dst; const double *pit_w;      // out-edges sorted by (src, dst)
    const int32_t *pin_dst, *pin_src; const double *pin_w;     // in-edges sorted by (dst, src)
    int64_t n_pit;
    int n, m, kind, stat;
    int32_t *ctr;
    int64_t qcap;                                              // queue entries (= cells: every cell enters at most once)
};

__device__ __forceinline__ double dd_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ bool dd_is_open(const DistArgs &A, int32_t c) { return reinterpret_cast<const uint32_t *>(A.D)[2 * (int64_t)c + 1] == DD_OPEN_HI; }
__device__ __forceinline__ int32_t *dd_count(const DistArgs &A, int32_t c) { return reinterpret_cast<int32_t *>(A.D) + 2 * (int64_t)c; }

// first edge of a sorted pit list whose key is >= `key` (the lists hold a few edges per drained pit: ~17 probes, only for
// the cells whose graph word carries a pit flag)
__device__ __forceinline__ int64_t dd_lower_bound(const int32_t *__restrict__ keys, int64_t n, int32_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// wave-aggregated append of the cells that became ready (call from control flow that is uniform per wavefront)
__device__ __forceinline__ void dd_push(const DistArgs &A, bool pred, int32_t cell)
{
    const unsigned long long bal = __ballot(pred);
    if (bal == 0ull) return;
    const int lane = (int)__lane_id();
    const int leader = __ffsll((long long)bal) - 1;
    int32_t base = 0;
    if (lane == leader) base = atomicAdd(A.ctr + DD_TAIL, (int32_t)__popcll(bal));
    base = __shfl(base, leader);
    const int64_t slot = (int64_t)base + __popcll(bal & ((1ull << lane) - 1ull));
    if (pred && slot < A.qcap) A.queue[slot] = cell;
}

struct DistAcc {
    double num = 0.0, den = 0.0, lo = INFINITY, hi = -INFINITY;
    bool nan = false;
};

// cost of the edge (i, j) -> (i + di, j + dj): dx, dy = cell size of row i, zc / zd = elevation of source / destination
__device__ __forceinline__ double dd_cost(int kind, int di, int dj, double dx, double dy, double zc, double zd)
{
    const double h = kind != 1 ? hypot((double)dj * dx, (double)di * dy) : 0.0;
    if (kind == 0) return h;
    const double dz = zc - zd;
    return kind == 1 ? dz : hypot(h, dz);
}

__device__ __forceinline__ void dd_add(DistAcc &S, double w, double t)
{
    S.num += w * t; S.den += w;
    S.nan = S.nan || t != t;
    S.lo = t < S.lo ? t : S.lo;
    S.hi = t > S.hi ? t : S.hi;
}

__device__ __forceinline__ double dd_result(int stat, const DistAcc &S)
{
    double r = stat == 0 ? S.num / S.den : (stat == 1 ? S.lo : S.hi);
    if (S.nan || r != r) r = dd_nan();
    return r;
}

// cells finished and tiles visited by a pass, from the tiles' own words (-1: not visited)
__global__ __launch_bounds__(256) void k_dd_pass_sum(const int32_t *__restrict__ tile_done, int ntiles, int32_t *ctr)
{
    __shared__ int32_t s_cells, s_visits;
    if (threadIdx.x == 0) { s_cells = 0; s_visits = 0; }
    __syncthreads();
    int32_t cells = 0, visits = 0;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < ntiles; k += gridDim.x * blockDim.x) {
        const int32_t d = tile_done[k];
        if (d >= 0) { cells += d; visits++; }
    }
    if (visits) { atomicAdd(&s_cells, cells); atomicAdd(&s_visits, visits); }
    __syncthreads();
    if (threadIdx.x == 0 && s_visits) {
        atomicAdd(reinterpret_cast<unsigned long long *>(ctr + DD_PASSDONE), (unsigned long long)s_cells);
        atomicAdd(ctr + DD_VISITS, s_visits);
    }
}

// the frontier window moves on: [DD_LO, DD_HI) = what the level before appended
__global__ void k_dd_advance(int32_t *ctr)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int32_t lo = ctr[DD_HI], hi = ctr[DD_TAIL];
        ctr[DD_LO] = lo; ctr[DD_HI] = hi;
        if (hi > lo) ctr[DD_LEVELS] += 1;
    }
}

// ---- the queue of a REVERSE sweep (flowdist.hip, flowacc_rev.hip): both depend on the graph alone, not on the statistic
// cell v is final: every open cell with an edge into v has one open out-edge less.  `cw` = graph word of v, 0 for a lane
// that holds no cell.
__device__ __forceinline__ void dd_release(const DistArgs &A, int32_t v, uint32_t cw)
{
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int32_t u = v + NB_DI[d] * A.m + NB_DJ[d];
        bool ready = false;
        // (a target upstream of v is final already and holds a value, not a count)
        if ((cw & (1u << d)) && dd_is_open(A, u)) ready = atomicSub(dd_count(A, u), 1) == 1;
        dd_push(A, ready, u);
    }
    if (cw & CI_PIT_IN) {
        for (int64_t e = dd_lower_bound(A.pin_dst, A.n_pit, v); e < A.n_pit && A.pin_dst[e] == v; e++) {
            const int32_t u = A.pin_src[e];
            if (dd_is_open(A, u) && atomicSub(dd_count(A, u), 1) == 1) {
                const int64_t slot = atomicAdd(A.ctr + DD_TAIL, 1);
                if (slot < A.qcap) A.queue[slot] = u;
            }
        }
    }
}

// every open cell counts its open out-neighbours (all values are from earlier launches); those with none start the queue
__global__ __launch_bounds__(256) void k_dd_recount(DistArgs A)
{
    for (int i = blockIdx.y; i < A.n; i += gridDim.y)
    for (int j0 = blockIdx.x * blockDim.x; j0 < A.m; j0 += gridDim.x * blockDim.x) {
        const int j = j0 + (int)threadIdx.x;
        bool ready = false;
        int32_t c = 0;
        if (j < A.m) {
            c = i * A.m + j;
            if (dd_is_open(A, c)) {
                const uint32_t cw = A.cinfo[c];
                const int s = ci_section(cw);
                int cnt = 0;
                if ((cw & CI_OUT1) && dd_is_open(A, c + fe1r(s) * A.m + fe1c(s))) cnt++;
                if ((cw & CI_OUT2) && dd_is_open(A, c + fe2r(s) * A.m + fe2c(s))) cnt++;
                if (cw & CI_PIT_OUT)
                    for (int64_t e = dd_lower_bound(A.pit_src, A.n_pit, c); e < A.n_pit && A.pit_src[e] == c; e++)
                        if (dd_is_open(A, A.pit_dst[e])) cnt++;
                *dd_count(A, c) = cnt;
                ready = cnt == 0;
            }
        }
        dd_push(A, ready, c);
    }
}

// cells that never became ready (on or upstream of a drainage cycle): a plain NaN instead of the count
__global__ void k_dd_unresolved(double *D, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x)
        if (reinterpret_cast<const uint32_t *>(D)[2 * c + 1] == DD_OPEN_HI) D[c] = dd_nan();
}

}  // namespace

// grid of the kernels that walk the tile row by row (256 columns per workgroup)
static dim3 dist_row_grid(const pydem_tile *t)
{
    const unsigned gx = (unsigned)cdiv(t->m, 256), gy = 4096 / gx ? 4096 / gx : 1;
    return dim3(gx, gy < (unsigned)t->n ? gy : (unsigned)t->n);
}

// the state both calls share (allocated by the first call of either, freed with the tile) and the argument block over it
static int dist_state(pydem_tile *t, DistArgs &A, int kind, int stat)
{
    const int64_t ntiles = cdiv(t->m, DD_T) * cdiv(t->n, DD_T);
    PYDEM_TRY(tile_alloc(t, &t->dd_out, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->dd_queue, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->dd_ctr, (size_t)(DD_WORDS + 4 * ntiles)));
    if (!t->dd_h_ctr) HIP_TRY(hipHostMalloc((void **)&t->dd_h_ctr, DD_WORDS * sizeof(int32_t), hipHostMallocDefault));
    for (int k = 0; k < 2; k++) if (!t->dd_ev[k]) HIP_TRY(hipEventCreate(&t->dd_ev[k]));
    A.cinfo = t->cinfo; A.prop = t->prop; A.elev = t->elev; A.dX2 = t->dX2; A.dY2 = t->dY2;
    A.D = t->dd_out; A.queue = t->dd_queue; A.mask = t->dd_mask;
    A.pit_src = t->pits.src; A.pit_dst = t->pits.dst; A.pit_w = t->pits.w;
    A.pin_dst = t->pits.in_dst; A.pin_src = t->pits.in_src; A.pin_w = t->pits.in_w;
    A.n_pit = t->pits.n_edges;
    A.n = (int)t->n; A.m = (int)t->m; A.kind = kind; A.stat = stat;
    A.ctr = t->dd_ctr; A.qcap = t->NN;
    return 0;
}

// The schedule of a call, the same for both directions: the counters, the cell pattern (`init`), tile passes while they pay
// (`tiles`), the queue for the rest (`recount`, then one `level` launch per level), NaN for what never became ready, the
// timing and the download.  The four arguments launch the direction's kernels on the tile's stream; default_per_visit: the
// cells a tile visit has to finish on average for another pass to beat the queue (the switch point of the direction).
template <class FInit, class FTiles, class FRecount, class FLevel>
static int dist_schedule(pydem_tile *t, const char *what, int64_t default_per_visit, double *out, double *ms, int64_t *levels,
                         int64_t *n_unresolved, FInit init, FTiles tiles, FRecount recount, FLevel level)
{
    const int tiles_x = (int)cdiv(t->m, DD_T), tiles_y = (int)cdiv(t->n, DD_T);
    const int64_t ntiles = (int64_t)tiles_x * tiles_y;
    int32_t *tile_state = t->dd_ctr + DD_WORDS;
    // PYDEM_DIST_PASSES=<n>: at most n tile passes (0: the queue alone); PYDEM_DIST_MIN_PER_VISIT=<n>: the switch point (0: tile
    // passes for as long as one finishes anything).  For tests and timing: the result does not depend on either.
    static const int max_passes = [] { const char *e = getenv("PYDEM_DIST_PASSES"); const int v = e ? atoi(e) : DD_MAX_PASSES; return v < 0 ? 0 : v; }();
    static const int64_t env_per_visit = [] { const char *e = getenv("PYDEM_DIST_MIN_PER_VISIT"); return e ? (int64_t)atoll(e) : (int64_t)-1; }();
    const int64_t min_per_visit = env_per_visit >= 0 ? env_per_visit : default_per_visit;
    const int glevel = grid_for(cdiv(t->NN, 4), 2048);
    volatile int32_t *h = t->dd_h_ctr;
    auto look = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(t->dd_h_ctr, t->dd_ctr, DD_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        return 0;
    };
    auto word64 = [&](int k) { return (int64_t)(((uint64_t)(uint32_t)h[k + 1] << 32) | (uint32_t)h[k]); };
    HIP_TRY(hipEventRecord(t->dd_ev[0], t->stream));
    HIP_TRY(hipMemsetAsync(t->dd_ctr, 0, (DD_WORDS + 4 * ntiles) * sizeof(int32_t), t->stream));
    init();
    HIP_TRY(hipGetLastError());
    // tile passes while they pay
    int64_t n_levels = 1, done = 0, visits = 0, n_open = -1;
    for (int pass = 1; pass <= max_passes; pass++) {
        tiles(pass, tiles_x, tiles_y, tile_state);
        hipLaunchKernelGGL(k_dd_pass_sum, dim3(grid_for(ntiles, 256)), dim3(256), 0, t->stream, (const int32_t *)(tile_state + 3 * ntiles), (int)ntiles, t->dd_ctr);
        HIP_TRY(hipGetLastError());
        PYDEM_TRY(look());
        n_open = word64(DD_NOPEN);
        const int64_t d = word64(DD_PASSDONE) - done, v = (int64_t)h[DD_VISITS] - visits;
        done += d; visits += v;
        if (d > 0) n_levels++;
        if (done >= n_open || d == 0 || d < min_per_visit * v) break;
    }
    if (n_open < 0) { PYDEM_TRY(look()); n_open = word64(DD_NOPEN); }
    // the queue for the rest
    if (done < n_open) {
        recount();
        hipLaunchKernelGGL(k_dd_advance, dim3(1), dim3(64), 0, t->stream, t->dd_ctr);
        HIP_TRY(hipGetLastError());
        for (;;) {
            for (int k = 0; k < DD_BATCH; k++) {
                level(glevel);
                hipLaunchKernelGGL(k_dd_advance, dim3(1), dim3(64), 0, t->stream, t->dd_ctr);
            }
            HIP_TRY(hipGetLastError());
            PYDEM_TRY(look());
            if (h[DD_HI] == h[DD_LO]) break;         // the last level appended nothing
        }
        n_levels += (int64_t)h[DD_LEVELS];
        done += (int64_t)h[DD_TAIL];
    }
    const int64_t left = n_open - done;
    if (left > 0) {
        hipLaunchKernelGGL(k_dd_unresolved, dim3(grid_for(t->NN, 2048)), dim3(256), 0, t->stream, t->dd_out, t->NN);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(t->dd_ev[1], t->stream));
    HIP_TRY(hipEventSynchronize(t->dd_ev[1]));
    float el = 0.f;
    HIP_TRY(hipEventElapsedTime(&el, t->dd_ev[0], t->dd_ev[1]));
    if (ms) *ms = (double)el;
    if (levels) *levels = n_levels;        // the initial level + tile passes that finished something + levels of the queue
    if (n_unresolved) *n_unresolved = left;
    {
        static const bool dbg = [] { const char *e = getenv("PYDEM_DIST_DEBUG"); return e && atoi(e) > 0; }();
        if (dbg) fprintf(stderr, "%s: %lld open cells, %lld tile visits finished %lld, queue: %d levels, %d cells; %lld unresolved; %.3f ms\n",
                         what, (long long)n_open, (long long)visits, (long long)word64(DD_PASSDONE), (int)h[DD_LEVELS], (int)h[DD_TAIL], (long long)left, (double)el);
    }
    if (out) PYDEM_TRY(tile_plane_copy(t, t->dd_out, out, (size_t)t->NN * 8, true));
    return 0;
}
