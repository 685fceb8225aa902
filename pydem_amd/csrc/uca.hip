// uca.hip -- K3 section/proportion, K4 implicit flow graph, K5 frontier sweep, K6 TWI.
//
// Replaces, for one tile (reference pydem/dem_processing.py unless noted):
//   K3  _calc_uca_section_proportion :1021-1070                      (int8 facet index: bit-exact)
//   K4  _mk_adjacency_matrix :1072-1153 + _mk_connectivity :1155-1267 -- the reference builds an
//       NN x NN scipy CSC matrix (and its CSR twin, :879); here the graph stays implicit: every
//       cell has <= 2 regular out-edges given by (section, proportion) and the keep-filter of
//       :1136-1137, so a cell's regular in-edges are one bit per 8-neighbour (the in-mask of the graph word, uca_graph.h); the few
//       non-adjacent pit->drain edges live in a small side list (PitGraph).
//   K5  _calc_uca_chunk :864-987 + the native loop cyutils._drain_area (pydem/cyfuncs/cyutils.pyx
//       :119-187): topological sweep.  The reference pushes area[i]*w along out-edges and re-scans
//       all N cells four times per round; here each cell PULLS a0 + sum(area[u]*w(u->c)) over its
//       in-edges in a fixed order (no floating-point atomics, so results are run-to-run
//       deterministic).  Default schedule: tile passes (K5b) -- one wavefront per 32x32 tile runs
//       as many level-synchronous rounds as it can on its CU, tiles are re-listed when a finished
//       cell drains into them.  Alternative (PYDEM_SWEEP_MODE=queue): frontier queue rounds with a
//       level-ownership hand-off instead of in-degree atomics.  On a DAG all formulations compute
//       the same fixed point; only the order of the additions differs from the reference's push
//       (<= a few ulp; tolerance 1e-6 relative per BASELINE.json).
//   K6  calc_twi :1647-1677.
// The cross-tile edge fix-up that runs on the same graph afterwards (K7) is uca_edge.hip.
// The pointwise kernels are bounded by HBM; the sweeps by dependent memory latency times the tiles / cells in flight.
#include "uca_graph.h"      // the graph word, SweepArgs, QE and the counter slots: shared with the edge fix-up (uca_edge.hip)
#include <algorithm>
#include <vector>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define PI_D 3.141592653589793

namespace {

// ------------------------------------------------------------------------------- K3 (+ first half of K4)
// section / proportion, and while both are in registers the cell's two regular out-edges (keep-filter of
// :1136-1137): the graph word leaves this kernel with its out flags and facet index; the in-mask follows
// in k_graph_inmask from the neighbours' words
__global__ __launch_bounds__(256) void k_section_proportion(const double *__restrict__ dir,
                                                            const uint8_t *__restrict__ flats,
                                                            const double *__restrict__ sec_theta, int64_t NN, int n, int m,
                                                            const double *__restrict__ elev,
                                                            int8_t *__restrict__ section, double *__restrict__ prop,
                                                            uint32_t *__restrict__ cinfo)
{
    // rows come from blockIdx.y (grid-stride), columns from blockIdx.x: no 64-bit division per cell
    (void)NN;
    for (int i = blockIdx.y; i < n; i += gridDim.y)
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const int64_t c = (int64_t)i * m + j;
        const double theta = sec_theta[i];
        const double d = dir[c];
        int sec0 = (int)(int8_t)(int)floor(d / PI_D * 2.0);                      // :1035
        const double quadrant = d - PI_D / 2.0 * (double)sec0;                   // :1037
        const int mod2 = sec0 & 1;                                               // python % 2
        int sec = sec0 * 2 + ((quadrant > theta) && mod2 == 0) + ((quadrant > (PI_D / 2 - theta)) && mod2 == 1);  // :1040-1043
        sec = (int)(int8_t)sec;
        const bool I1 = sec == 0 || sec == 1 || sec == 4 || sec == 5;           // :1050
        const double cth = PI_D / 2 - theta;
        // the four cases of :1052-1062 -- I1: quadrant / theta or (quadrant - theta) / cth, else: quadrant / cth or (quadrant - cth) / theta --
        // exclude each other: operands selected first, ONE division (a wavefront holds cells of all four cases, and the four
        // predicated fp64 divisions were most of this kernel's instructions); a NaN direction fails both tests and stays NaN
        const double t1 = I1 ? theta : cth, t2 = I1 ? cth : theta;
        const bool lo = quadrant <= t1, hi = quadrant > t1;
        const double num = lo ? quadrant : quadrant - t1, den = lo ? t1 : t2;
        double p = (lo || hi) ? num / den : NAN;
        if (flats[c]) { sec = -1; p = NAN; }                                     // :1064-1065
        if (sec == 8) sec = 0;                                                   // :1067
        const int a = (sec & 1) ? -1 : 1;                                        // adjust[section], negative wraps
        const double pf = (1 + a) / 2.0 - (double)a * p;                         // :1068
        prop[c] = pf;
        section[c] = (int8_t)sec;
        uint32_t gf = 0;
        if (sec >= 0 && sec <= 7) {
            const double z = elev[c];
            const int i1 = i + fe1r(sec), j1 = j + fe1c(sec), i2 = i + fe2r(sec), j2 = j + fe2c(sec);
            if (i1 >= 0 && i1 < n && j1 >= 0 && j1 < m && keep_edge(pf, elev[(int64_t)i1 * m + j1], z)) gf |= CI_OUT1;
            if (i2 >= 0 && i2 < n && j2 >= 0 && j2 < m && keep_edge(1 - pf, elev[(int64_t)i2 * m + j2], z)) gf |= CI_OUT2;   // weights [prop, 1 - prop] :1082
        }
        cinfo[c] = gf | ((uint32_t)(sec & 7) << CI_SEC_SHIFT);
    }
}

// ------------------------------------------------------------------------------- K4
// second half of K4: a neighbour drains into this cell iff its facet points here and that out-edge survived the
// keep-filter -- both are in the neighbour's graph word (4 B, row-coalesced) instead of its section, proportion
// and elevation
__global__ __launch_bounds__(256) void k_graph_inmask(const double *__restrict__ prop, const double *__restrict__ elev,
                                                      int n, int m, uint32_t *__restrict__ cinfo, uint8_t *__restrict__ todo0,
                                                      uint8_t *__restrict__ todo_work, double *__restrict__ corner_sums)
{
    for (int i = blockIdx.y; i < n; i += gridDim.y)
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const int64_t c = (int64_t)i * m + j;
        const uint32_t cw = cinfo[c] & (CI_OUT1 | CI_OUT2 | (7u << CI_SEC_SHIFT));
        uint32_t im = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const int ui = i + NB_DI[d], uj = j + NB_DJ[d];
            if (ui < 0 || ui >= n || uj < 0 || uj >= m) continue;
            const uint32_t wu = cinfo[(int64_t)ui * m + uj];
            const int su = (int)((wu >> CI_SEC_SHIFT) & 7u);
            const bool cardinal = (NB_DI[d] == 0) || (NB_DJ[d] == 0);
            if ((su == NB_S0[d] || su == NB_S1[d]) && (wu & (cardinal ? CI_OUT1 : CI_OUT2))) im |= 1u << d;
        }
        // sources (no in-edges) are round 0
        cinfo[c] = im | cw | ((im ? CI_LEVEL_INF : 0u) << CI_LEVEL_SHIFT);
        // inlet-edge detection (_calc_uca_chunk :909-930); interior cells are never 'todo'
        const bool top = i == 0, bot = i == n - 1, left = j == 0, right = j == m - 1;
        if (top || bot || left || right) {
            const double TOL = 1e-2;
            const double p = prop[c], z = elev[c];
            double outsum = 0.0;
            if (cw & CI_OUT1) outsum += p;
            if (cw & CI_OUT2) outsum += 1 - p;
            const int s = (cw & (CI_OUT1 | CI_OUT2)) ? ci_section(cw) : -1;     // only cells with an out-edge can be inlets
            bool td = false;
            const bool has_out = outsum > TOL;
            // assignment order of the reference: left, right, top, bottom (later overwrite earlier)
            if (left) td = has_out && (s == 6 || s == 7 || s == 0 || s == 1);
            if (right) td = has_out && (s == 2 || s == 3 || s == 4 || s == 5);
            if (top) td = has_out && (s == 4 || s == 5 || s == 6 || s == 7);
            if (bot) td = has_out && (s == 0 || s == 1 || s == 2 || s == 3);
            if ((top || bot) && (left || right)) {
                double insum = 0.0;
                for (int d = 0; d < 8; d++)
                    if (im & (1u << d)) {
                        const int64_t u = (int64_t)(i + NB_DI[d]) * m + (j + NB_DJ[d]);
                        const bool cardinal = (NB_DI[d] == 0) || (NB_DJ[d] == 0);
                        insum += cardinal ? prop[u] : 1 - prop[u];
                    }
                const int q = (top ? 0 : 2) + (left ? 0 : 1);
                corner_sums[q * 3 + 0] = outsum;
                corner_sums[q * 3 + 1] = insum;
                corner_sums[q * 3 + 2] = td ? 1.0 : 0.0;
            }
            if (isnan(z)) td = false;                                            // :935
            todo0[c] = td;
            todo_work[c] = td;
        }
    }
}

// pit edges contribute to in-degrees, flags and the corner sums
// STASH (pydem_uca only, where the area plane is free until the sweep): the walk also leaves {first in-edge, first out-edge} of
// every pit source / drain in the cell's area slot, what k_pit_stash (below) does in a walk of its own over the same lists
template <bool STASH>
__global__ void k_graph_add_pits(const int32_t *__restrict__ src, const int32_t *__restrict__ dst,
                                 const double *__restrict__ w, int64_t ne, int n, int m,
                                 uint32_t *cinfo, double *corner_sums, const int32_t *__restrict__ pin_dst, double *area)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = src[e], d = dst[e];
        if (STASH) {
            int32_t *slots = reinterpret_cast<int32_t *>(area);
            const int32_t pd = pin_dst[e];
            if (e == 0 || pin_dst[e - 1] != pd) slots[2 * (int64_t)pd] = (int32_t)e;
            if (e == 0 || src[e - 1] != s) slots[2 * (int64_t)s + 1] = (int32_t)e;
        }
        atomicOr(&cinfo[s], CI_PIT_OUT);
        atomicOr(&cinfo[d], CI_PIT_IN | (CI_LEVEL_INF << CI_LEVEL_SHIFT));   // a pit drains here: not a source
        const int corners[4] = {0, m - 1, (n - 1) * m, (n - 1) * m + m - 1};
        for (int q = 0; q < 4; q++) {
            if (s == corners[q]) atomicAdd(&corner_sums[q * 3 + 0], w[e]);
            if (d == corners[q]) atomicAdd(&corner_sums[q * 3 + 1], w[e]);
        }
    }
}

// corner pass-through rule (:920-930): todo |= (outsum > TOL) | (insum < TOL)
__global__ void k_corner_todo(const double *__restrict__ corner_sums, const double *__restrict__ elev, int n, int m,
                              uint8_t *todo0, uint8_t *todo_work)
{
    const int q = threadIdx.x;
    if (q >= 4) return;
    const int64_t corners[4] = {0, m - 1, (int64_t)(n - 1) * m, (int64_t)(n - 1) * m + m - 1};
    const int64_t c = corners[q];
    bool td = corner_sums[q * 3 + 2] != 0.0;
    td = td || (corner_sums[q * 3 + 0] > 1e-2) || (corner_sums[q * 3 + 1] < 1e-2);
    if (isnan(elev[c])) td = false;
    todo0[c] = td;
    todo_work[c] = td;
}

// ------------------------------------------------------------------------------- K5
// Frontier bookkeeping without per-edge atomics.  level[c] is the round in which cell c is
// processed (0 for sources, LEVEL_INF while unknown).  When cell u (level r) is final it looks at
// each target t: t is ready for round r+1 iff every upstream cell of t has level <= r, and exactly
// one of t's upstream cells with level == r -- the one with the largest cell id -- appends t to
// the next frontier and stamps level[t] = r+1.  All level-r stamps were written by the previous
// launch, so the test reads only settled values; the in-degree counters (and their ~1.4 device
// atomics per cell) of a textbook Kahn sweep disappear.  The frontier itself is appended through
// an LDS staging buffer: wavefront ballot + popcount prefix, one LDS atomic per wave, and one
// global atomic per ~1.5k cells when the buffer is flushed.
constexpr int STAGE_CAP = 4096;      // LDS staging entries per block (8 B each: 32 KiB)
constexpr int STAGE_FLUSH = STAGE_CAP - 512;    // flush when fewer than 2*256 slots remain


struct Stage {
    QE buf[STAGE_CAP];
    int32_t cnt;
    int32_t base;
};

// wave-aggregated append into the block's LDS staging buffer
__device__ __forceinline__ void stage_push(Stage &S, bool pred, int32_t cell, uint32_t cw)
{
    const unsigned long long bal = __ballot(pred);
    if (bal == 0ull) return;
    const int lane = (int)__lane_id();
    const int leader = __ffsll((long long)bal) - 1;
    int32_t base = 0;
    if (lane == leader) base = atomicAdd(&S.cnt, (int32_t)__popcll(bal));
    base = __shfl(base, leader);
    if (pred) { QE q; q.c = cell; q.cw = cw; S.buf[base + __popcll(bal & ((1ull << lane) - 1ull))] = q; }
}

// block-wide: move the staged cells to the global frontier (call from uniform control flow)
__device__ __forceinline__ void stage_flush(const SweepArgs &A, Stage &S, QE *__restrict__ qn, int32_t *cn, bool force)
{
    __syncthreads();
    const int32_t c = S.cnt;
    if (c > 0 && (force || c > STAGE_FLUSH)) {
        if (threadIdx.x == 0) S.base = atomicAdd(cn, c);
        __syncthreads();
        const int32_t b = S.base;
        if ((int64_t)b + c <= A.qcap) { for (int32_t k = threadIdx.x; k < c; k += blockDim.x) qn[b + k] = S.buf[k]; }
        else if (threadIdx.x == 0) atomicAdd(A.err, 1);
        __syncthreads();
        if (threadIdx.x == 0) S.cnt = 0;
    }
    __syncthreads();
}

// Pit side lists without a search: until a cell is processed its slot of the area array is unused, so
// it carries {first in-edge, first out-edge} of the cell (k_pit_stash); the edges of one cell are
// contiguous in the sorted lists and end where the key changes.  Reading the slot costs one load that
// travels with the gathers instead of the block-table lookup plus key scan (3+ dependent loads).
__device__ __forceinline__ int2 pit_stash(const SweepArgs &A, int32_t c) { return reinterpret_cast<const int2 *>(A.area)[c]; }

__global__ void k_pit_stash(const int32_t *__restrict__ pin_dst, const int32_t *__restrict__ pit_src, int64_t ne, double *area)
{
    int32_t *slots = reinterpret_cast<int32_t *>(area);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        if (e == 0 || pin_dst[e - 1] != pin_dst[e]) slots[2 * (int64_t)pin_dst[e]] = (int32_t)e;
        if (e == 0 || pit_src[e - 1] != pit_src[e]) slots[2 * (int64_t)pit_src[e] + 1] = (int32_t)e;
    }
}

// graph words of the 8 neighbours of t (row ti, column tj); out-of-tile neighbours read t itself (never used)
__device__ __forceinline__ void load_upstream_words(const SweepArgs &A, int32_t t, int ti, int tj, uint32_t w[8])
{
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int ii = ti + NB_DI[d], jj = tj + NB_DJ[d];
        const bool ok = ii >= 0 && ii < A.n && jj >= 0 && jj < A.m;
        w[d] = A.cinfo[ok ? t + NB_DI[d] * A.m + NB_DJ[d] : t];
    }
}

// Frontier bookkeeping without per-edge atomics.  The level field of cinfo[c] is the round in which
// cell c is processed (0 for sources, CI_LEVEL_INF while unknown).  When cell u (level r) is final it
// looks at each target t: t is ready for round r+1 iff every upstream cell of t has level <= r, and
// exactly one of t's upstream cells with level == r -- the one with the largest cell id -- appends t
// to the next frontier and stamps level r+1.  All level-r stamps were written by the previous
// launch, so the test reads only settled values; the in-degree counters (and their ~1.4 device
// atomics per cell) of a textbook Kahn sweep disappear.
// `ct` = graph word of t, `w` = graph words of its neighbours (SPEC: all eight were loaded up front;
// otherwise only those in t's in-mask are fetched here), `in_start` = first pit in-edge of t.
template <bool SPEC>
__device__ __forceinline__ bool owns_target(const SweepArgs &A, int32_t t, int32_t u, uint32_t r, uint32_t ct, const uint32_t w[8],
                                            int32_t in_start)
{
    int32_t owner = -1;
    bool ready = true;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        if (ct & (1u << d)) {
            const int32_t v = t + NB_DI[d] * A.m + NB_DJ[d];
            const uint32_t lv = (v == u) ? r : ci_level(SPEC ? w[d] : A.cinfo[v]);
            ready = ready && (lv <= r);
            if (lv == r) owner = v > owner ? v : owner;
        }
    }
    if (ct & CI_PIT_IN) {
        for (int32_t e = in_start;; e += 4) {
            int32_t d4[4], s4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t idx = e + k < A.n_pit ? e + k : A.n_pit - 1;
                d4[k] = A.pin_dst[idx]; s4[k] = A.pin_src[idx];
            }
            uint32_t l4[4];
            bool v4[4];
            bool more = true;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                more = more && e + k < A.n_pit && d4[k] == t;
                v4[k] = more;
                l4[k] = (more && s4[k] != u) ? ci_level(A.cinfo[s4[k]]) : r;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (v4[k]) {
                    ready = ready && (l4[k] <= r);
                    if (l4[k] == r) owner = s4[k] > owner ? s4[k] : owner;
                }
            }
            if (!more) break;
        }
    }
    return ready && owner == u;
}

// publish a finished cell: area plus the two outgoing contributions (sign carries the todo taint)
__device__ __forceinline__ void publish_cell(const SweepArgs &A, int32_t c, uint32_t cw, double acc, bool td)
{
    A.area[c] = acc;
    double2 o = make_double2(0.0, 0.0);
    if (cw & (CI_OUT1 | CI_OUT2)) {
        const double p = A.prop[c];
        if (cw & CI_OUT1) o.x = acc * p;                                        // area[i] * factor, cyutils.pyx:163
        if (cw & CI_OUT2) o.y = acc * (1 - p);
        if (td) { o.x = -o.x; o.y = -o.y; }
    }
    A.contrib[c] = o;
    if (td) A.todo_work[c] = 1;
}

// sum over the pit in-edges of cell c (sorted by source id), four edges per batch of loads
__device__ __forceinline__ void gather_pit_edges(const SweepArgs &A, int32_t c, int32_t in_start, double &acc, bool &td)
{
    for (int32_t e = in_start;; e += 4) {
        int32_t d4[4], s4[4]; double w4[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t idx = e + k < A.n_pit ? e + k : A.n_pit - 1;
            d4[k] = A.pin_dst[idx]; s4[k] = A.pin_src[idx]; w4[k] = A.pin_w[idx];
        }
        double a4[4]; uint8_t t4[4];
        bool more = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            more = more && e + k < A.n_pit && d4[k] == c;
            a4[k] = more ? A.area[s4[k]] : 0.0;
            t4[k] = more ? A.todo_work[s4[k]] : (uint8_t)0;
        }
        more = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            more = more && e + k < A.n_pit && d4[k] == c;
            if (more) { acc += a4[k] * w4[k]; td = td || (t4[k] != 0); }
        }
        if (!more) break;
    }
}

// rounds >= 1: pull, store, release.  LOWLAT (small frontiers): every load that only needs the queue
// entry -- in-edge contributions, the targets' graph words, the graph words of ALL their neighbours,
// the pit slots -- is issued in one batch, so a regular cell costs two dependent memory round trips
// per round (queue entry, batch).  Large frontiers are bound by the lines they touch, not by latency,
// and fetch only the neighbours in each target's in-mask.
// push2(pred, t, ct): called by all lanes together for the two regular targets; pushp(t, ct): called
// by single lanes for the (rare) pit targets.
template <bool LOWLAT, typename Push2, typename PushP>
__device__ __forceinline__ void process_cell(const SweepArgs &A, bool active, QE q, uint32_t r, Push2 push2, PushP pushp)
{
    const int32_t c = q.c;
    const uint32_t cw = q.cw;
    int32_t t1 = -1, t2 = -1;
    uint32_t c1 = 0, c2 = 0;
    bool r1 = false, r2 = false;
    int32_t out_start = -1;
    if (active) {
        const int m = A.m;
        const int i = c / m, j = c - i * m;
        const int sct = ci_section(cw);
        uint32_t l1[8], l2[8];
        int2 s1 = make_int2(-1, -1), s2 = make_int2(-1, -1), sc = make_int2(-1, -1);
        if (cw & CI_OUT1) {
            const int dr = fe1r(sct), dc = fe1c(sct);
            t1 = c + dr * m + dc; c1 = A.cinfo[t1];
            if (LOWLAT) { load_upstream_words(A, t1, i + dr, j + dc, l1); s1 = pit_stash(A, t1); }
        }
        if (cw & CI_OUT2) {
            const int dr = fe2r(sct), dc = fe2c(sct);
            t2 = c + dr * m + dc; c2 = A.cinfo[t2];
            if (LOWLAT) { load_upstream_words(A, t2, i + dr, j + dc, l2); s2 = pit_stash(A, t2); }
        }
        if (cw & (CI_PIT_IN | CI_PIT_OUT)) sc = pit_stash(A, c);
        double acc = A.a0[i];                                                   // :885, :901
        // only inlet cells on the tile edge start tainted (:909-930); interior bytes are written later
        bool td = (i == 0 || i == A.n - 1 || j == 0 || j == m - 1) && A.todo_work[c] != 0;
        // regular in-edges in ascending source id: NW N NE W E SW S SE; a cardinal neighbour feeds us
        // through its first slot, a diagonal one through its second
#pragma unroll
        for (int d = 0; d < 8; d++) {
            if (cw & (1u << d)) {
                const int32_t u = c + NB_DI[d] * m + NB_DJ[d];
                const bool cardinal = (NB_DI[d] == 0) || (NB_DJ[d] == 0);
                const double x = cardinal ? A.contrib[u].x : A.contrib[u].y;
                acc += fabs(x);                                                 // cyutils.pyx:163
                td = td || (x < 0);                                             // :165 (float taint -> bool)
            }
        }
        if (cw & CI_PIT_IN) gather_pit_edges(A, c, sc.x, acc, td);
        out_start = sc.y;
        publish_cell(A, c, cw, acc, td);
        if (t1 >= 0) {
            if (!LOWLAT && (c1 & CI_PIT_IN)) s1 = pit_stash(A, t1);
            r1 = owns_target<LOWLAT>(A, t1, c, r, c1, l1, s1.x);
        }
        if (t2 >= 0) {
            if (!LOWLAT && (c2 & CI_PIT_IN)) s2 = pit_stash(A, t2);
            r2 = owns_target<LOWLAT>(A, t2, c, r, c2, l2, s2.x);
        }
        if (r1) A.cinfo[t1] = ci_with_level(c1, r + 1);
        if (r2) A.cinfo[t2] = ci_with_level(c2, r + 1);
    }
    push2(r1, t1, c1);
    push2(r2, t2, c2);
    if (active && (cw & CI_PIT_OUT)) {                                           // rare: drained pit
        for (int32_t e = out_start;; e += 4) {
            int32_t s4[4], t4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t idx = e + k < A.n_pit ? e + k : A.n_pit - 1;
                s4[k] = A.pit_src[idx]; t4[k] = A.pit_dst[idx];
            }
            bool more = true;
            for (int k = 0; k < 4 && more; k++) {
                more = e + k < A.n_pit && s4[k] == c;
                if (!more) break;
                const int32_t t = t4[k];
                const uint32_t ct = A.cinfo[t];
                const int2 st = pit_stash(A, t);
                uint32_t lw[8];
                load_upstream_words(A, t, t / A.m, t % A.m, lw);
                if (owns_target<true>(A, t, c, r, ct, lw, st.x)) {
                    A.cinfo[t] = ci_with_level(ct, r + 1);
                    pushp(t, ct);
                }
            }
            if (!more) break;
        }
    }
}

#ifdef PYDEM_SWEEP_QUEUE      // the frontier-queue schedule: a diagnostic build only (python -m pydem_amd.build with PYDEM_HIPCC_FLAGS=-DPYDEM_SWEEP_QUEUE)
// one frontier round; counters rotate over 3 slots: in = r%3, out = (r+1)%3, (r+2)%3 is cleared
template <bool LOWLAT>
__global__ __launch_bounds__(256) void k_sweep_round(SweepArgs A, const QE *__restrict__ qc, QE *__restrict__ qn,
                                                     int32_t *cnt3, int r, int32_t *total)
{
    __shared__ Stage S;
    const int32_t nq = cnt3[r % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) { cnt3[(r + 2) % 3] = 0; if (nq) { atomicAdd(total, nq); atomicAdd(total + 2, 1); } }
    if (nq == 0) return;
    if (threadIdx.x == 0) S.cnt = 0;
    __syncthreads();
    int32_t *cn = &cnt3[(r + 1) % 3];
    for (int32_t base = blockIdx.x * blockDim.x; base < nq; base += gridDim.x * blockDim.x) {
        const int32_t q = base + threadIdx.x;
        const bool active = q < nq;
        QE qe; qe.c = 0; qe.cw = 0;
        if (active) qe = qc[q];
        process_cell<LOWLAT>(A, active, qe, (uint32_t)r,
                             [&](bool pred, int32_t t, uint32_t ct) { stage_push(S, pred, t, ct); },
                             [&](int32_t t, uint32_t ct) {
                                 const int32_t slot = atomicAdd(cn, 1);
                                 if (slot < A.qcap) { QE e; e.c = t; e.cw = ct; qn[slot] = e; }
                                 else atomicAdd(A.err, 1);
                             });
        stage_flush(A, S, qn, cn, false);
    }
    stage_flush(A, S, qn, cn, true);
}

// Small frontiers: ONE workgroup runs round after round without going back to the host.  A kernel
// boundary makes every first access of the next round a trip across the fabric (the per-XCD L2s are
// only coherent at kernel boundaries), ~2 us per dependent load and 4+ of them per round; inside one
// workgroup the frontier, the graph words and the contributions it wrote a round ago come from its
// own CU's caches and __syncthreads() is the only synchronisation.  The last ~600 rounds of a
// 16384^2 tile are rivers of a few hundred cells.  Stops when the frontier is empty or outgrows
// SWEEP_SMALL_CAP; reports the round it stopped at and what it processed.
constexpr int SWEEP_SMALL_CAP = 1024;

__global__ __launch_bounds__(1024) void k_sweep_small(SweepArgs A, QE *q0, QE *q1, int32_t *cnt3, int r_start, int r_max,
                                                      int32_t *total, int32_t *state)
{
    __shared__ int s_next;
    int r = r_start;
    int32_t nq = cnt3[r % 3];
    int32_t done = 0, rounds = 0;
    while (nq > 0 && nq <= SWEEP_SMALL_CAP && r < r_max) {
        if (threadIdx.x == 0) s_next = 0;
        __syncthreads();
        const QE *qc = (r % 2) ? q1 : q0;
        QE *qn = (r % 2) ? q0 : q1;
        for (int32_t base = 0; base < nq; base += blockDim.x) {
            const int32_t q = base + threadIdx.x;
            const bool active = q < nq;
            QE qe; qe.c = 0; qe.cw = 0;
            if (active) qe = qc[q];
            auto push = [&](int32_t t, uint32_t ct) {
                const int32_t slot = atomicAdd(&s_next, 1);
                if (slot < A.qcap) { QE e; e.c = t; e.cw = ct; qn[slot] = e; }
                else atomicAdd(A.err, 1);
            };
            process_cell<true>(A, active, qe, (uint32_t)r, [&](bool pred, int32_t t, uint32_t ct) { if (pred) push(t, ct); }, push);
        }
        __syncthreads();
        done += nq; rounds++;
        nq = s_next;
        r++;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        cnt3[r % 3] = nq; cnt3[(r + 1) % 3] = 0; cnt3[(r + 2) % 3] = 0;
        atomicAdd(total, done); atomicAdd(total + 2, rounds);
        state[0] = r;
    }
}

#endif  // PYDEM_SWEEP_QUEUE

// ------------------------------------------------------------------------------- K5b
// Tile passes.  A queue round moves every flow path by ONE cell per kernel boundary and re-streams
// scattered 64 B lines for every cell it touches.  Here ONE WAVEFRONT owns a 32x32 tile for a pass and
// runs as many level-synchronous rounds as it can without leaving the CU: a cell is final once all
// its upstream cells are final -- those inside the tile become so during the pass, cells of the
// one-cell halo only if an earlier pass finished them.  Only the BOOKKEEPING lives in LDS (one word
// per cell -- graph bits + open-upstream count --, a final-cell bitmap for the setup, the ready ring: 4.9 KB per tile, so 32
// tiles are in flight per CU in the full passes and hide each other's latency); areas and contributions go straight to their global arrays, where
// the same wavefront finds them again in its caches a round later (a workgroup-scope fence orders a
// round's stores before the next round's loads).  A pass is either over all tiles (pass 1) or over
// the tiles LISTED by the previous pass: whenever a finished cell drains into another tile, that
// tile is listed for the next pass.  Flow paths advance by one tile per pass instead of one cell
// per round.  Cells finished in pass p carry level p.  The arithmetic per cell (gather order,
// products) is identical to process_cell().
#ifndef PYDEM_TH
#define PYDEM_TH 32
#endif
constexpr int TT = 32;                  // tile width (cells per row: two rows per wavefront load, a 34-bit row of the final bitmap)
constexpr int TH = PYDEM_TH, HH = TH + 2;  // tile height (32 or 64 rows)
static_assert(TH == 32 || TH == 64, "tile height");
// sp half-word of a cell: bits 14-15 state (0 open, 1 final / outside, 2 finished in this pass), bit 13 "waits for
// a cell another tile must finish", bits 0-12 upstream cells of this tile that are still open
constexpr uint32_t SP_STATE_SHIFT = 14, SP_BLOCKED = 1u << 13;
#ifndef PYDEM_STG_B
#define PYDEM_STG_B 4
#endif
constexpr int TILE_RING = TH == 32 ? 256 : 512;  // ready-list ring (a push that does not fit is dropped: the cell stays open with a zero
                                // count, the tile lists itself and the next pass picks the cell up in its setup)

struct TileW {
    uint32_t cs[TH * TT];           // per cell of the tile: high half = static graph bits, low half = sp (state / blocked / open-upstream
                                    // count); one LDS word per cell: a count-down is a plain 32-bit atomic, setup and rounds read both
                                    // halves at once.  The halo ring only exists as bits of `fin`.
    union {
        unsigned long long fin[HH]; // staging and setup: bit lj of row li (halo coordinates) = the cell was final before this pass
                                    // (or lies outside the grid)
        double a0[TH];              // rounds: cell area of the tile's rows
    };
    uint16_t list[TILE_RING];       // ready cells in the order they became ready
    int tail;                       // list end (monotonic; slot = index % TILE_RING)
    int limit;                      // first list index whose push was dropped (INT_MAX: none): the pass stops there
};                                  // 4888 bytes: eight 4-tile workgroups per CU

__device__ __forceinline__ uint16_t &sp_of(TileW &L, int idx) { return reinterpret_cast<uint16_t *>(L.cs)[2 * idx]; }
__device__ __forceinline__ uint32_t sp_state(const TileW &L, int idx) { return (L.cs[idx] >> SP_STATE_SHIFT) & 3u; }

// count-down of cell idx; returns the old half-word (a count that is decremented is >= 1: no borrow into the graph bits)
__device__ __forceinline__ uint32_t sp_dec(TileW &L, int idx) { return atomicSub(&L.cs[idx], 1u) & 0xFFFFu; }

__device__ __forceinline__ void tile_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// orders LDS traffic of the wavefront only (the rounds have no global stores to wait for)
__device__ __forceinline__ void tile_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

constexpr int TILE_PEND = 48;    // woken tiles a wavefront collects before it appends them to the next pass's list
struct TileNext {            // LISTED passes: tiles that must run again in the next pass
    int32_t *flag;           // per tile: last pass it was listed for
    int32_t *list, *count;
};

// contribution of in-edge d (0..7 = NW N NE W E SW S SE, the order of the in-mask bits) into cell c: one 8-byte load,
// the cardinal neighbours hand over their first share, the diagonal ones their second
__device__ __forceinline__ const double *in_edge_ptr(const SweepArgs &A, int32_t c, int m, int d)
{
    const int q = d + (d >> 2);                   // 0..8 with the centre (4) skipped
    const int di = (q * 11) >> 5;                 // q / 3
    const int32_t u = c + (di - 1) * m + (q - 3 * di - 1);
    return reinterpret_cast<const double *>(A.contrib + u) + (((0x5A >> d) & 1) ? 0 : 1);
}
__device__ __forceinline__ double in_edge(const SweepArgs &A, int32_t c, int m, int d) { return *in_edge_ptr(A, c, m, d); }

// Addresses of a tile visit.  The visits issue half of their cycles (profiles/r04_pmc_sq_hot.csv), and a third of a round's
// vector instructions were 64-bit address arithmetic: cell id (a quarter-rate 32-bit multiply) -> sign extension -> shift ->
// 64-bit add, per access.  The tile is wavefront-uniform, so the five planes get one SCALAR base each -- the address of the
// halo's first cell (i0 - 1, j0 - 1), which for a tile on the grid's edge lies in front of the plane and is only ever
// used with offsets of cells that exist -- and a lane addresses a cell by `h` = halo row * m + halo column (24-bit
// multiply: full rate; stage_sweep refuses tiles of 2^22 columns or more), scaled to a 32-bit unsigned byte offset: the
// loads and stores take the SGPR base + VGPR offset form.
struct TileBase {
    const char *cinfo, *area, *contrib, *prop, *todo;
    int32_t org;             // cell id of the halo's first cell (negative on the first row / column of the grid)
};
__device__ __forceinline__ TileBase tile_base(const SweepArgs &A, int i0, int j0)
{
    TileBase B;
    const int64_t org = (int64_t)(i0 - 1) * A.m + (j0 - 1);
    B.org = (int32_t)org;
    B.cinfo = reinterpret_cast<const char *>(A.cinfo) + org * 4;
    B.area = reinterpret_cast<const char *>(A.area) + org * 8;
    B.contrib = reinterpret_cast<const char *>(A.contrib) + org * 16;
    B.prop = reinterpret_cast<const char *>(A.prop) + org * 8;
    B.todo = reinterpret_cast<const char *>(A.todo_work) + org;
    return B;
}
template <typename T>
__device__ __forceinline__ T ld_off(const char *base, uint32_t off) { return *reinterpret_cast<const T *>(base + (size_t)off); }
template <typename T>
__device__ __forceinline__ void st_off(const char *base, uint32_t off, T v) { *reinterpret_cast<T *>(const_cast<char *>(base) + (size_t)off) = v; }
__device__ __forceinline__ uint32_t halo_cell(int li, int lj, int m) { return __umul24((uint32_t)li, (uint32_t)m) + (uint32_t)lj; }

// byte offsets of the eight in-edges relative to a cell's entry of the contribution plane (one LDS table per workgroup,
// filled at kernel start): neighbour d (0..7 = NW N NE W E SW S SE), the cardinal ones hand over their first share, the
// diagonal ones their second
__device__ __forceinline__ void fill_nbr16(int32_t *nbr16, int m)
{
    if (threadIdx.x < 8) {
        const int d = threadIdx.x, q = d + (d >> 2), di = q / 3, dj = q - 3 * di;
        nbr16[d] = ((di - 1) * m + (dj - 1)) * 16 + (((0x5A >> d) & 1) ? 0 : 8);
    }
}
__device__ __forceinline__ double in_edge_h(const TileBase &B, const int32_t *nbr16, uint32_t h, int d)
{
#ifdef PYDEM_EXP_AREAONLY      // timing experiment (taint is lost: results differ): the share formed from the upstream cell's area and proportion
    const uint32_t off16 = h * 16u + (uint32_t)nbr16[d];
    const uint32_t uo = (off16 >> 4) * 8u;
    const double ua = ld_off<double>(B.area, uo), up = ld_off<double>(B.prop, uo);
    return (off16 & 8u) ? ua * (1 - up) : ua * up;
#else
    return ld_off<double>(B.contrib, h * 16u + (uint32_t)nbr16[d]);        // (the neighbour lies in the halo: the sum is >= 0)
#endif
}

// staging of a tile visit: the graph words of the tile (high half of L.cs, state bit "final before this pass" in the low
// half) and the final bitmap of tile + halo
// (`hw`, when given: the graph words of the halo ring as well -- the symbolic visit K5f looks for its inlets there; ring
// position: top row 0..TT+1, bottom row TT+2.., left column 2(TT+2).., right column 2(TT+2)+TH..)
__device__ __forceinline__ void tile_stage(const SweepArgs &A, const TileBase &B, TileW &L, uint32_t pass, int i0, int j0, int lane,
                                           uint32_t *hw = nullptr)
{
    const int n = A.n, m = A.m;
    const int half = lane >> 5, l32 = lane & 31;
    constexpr int NSET = TH * TT / 64;
    // ---- stage the graph words of tile + halo by rows (two 32-cell rows per wavefront load, the halo ring in three
    // loads), a few loads of a lane in flight at a time: the passes are latency-bound.  The "final before this pass"
    // bits come out of wave ballots, one 64-bit word per row.
    auto stage_word = [&](int gi, int gj) -> uint32_t {                  // 0xFFFFFFFF: outside the grid
        return (gi >= 0 && gi < n && gj >= 0 && gj < m) ? A.cinfo[(int64_t)gi * m + gj] : 0xFFFFFFFFu;
    };
    auto final_before = [&](uint32_t w) -> bool {                        // outside the grid: nothing drains from there
        if (w == 0xFFFFFFFFu) return true;
        const uint32_t lv = ci_level(w);
        return lv >= 1 && lv < pass;
    };
    unsigned long long colL, colR;                                                  // bit r: the halo cell left / right of tile row r is final
    {
        const uint32_t wr = stage_word(half ? i0 + TH : i0 - 1, j0 + l32);          // top / bottom halo row
        uint32_t wk = 0xFFFFFFFFu;
        if (lane < 4) wk = stage_word((lane & 2) ? i0 + TH : i0 - 1, (lane & 1) ? j0 + TT : j0 - 1);   // corners
        if (hw) {
            hw[(half ? TT + 2 : 0) + l32 + 1] = wr;
            if (lane < 4) hw[((lane & 2) ? TT + 2 : 0) + ((lane & 1) ? TT + 1 : 0)] = wk;
        }
        if (TH == 32) {
            const uint32_t wc = stage_word(i0 + l32, half ? j0 + TT : j0 - 1);      // left / right halo column
            if (hw) hw[2 * (TT + 2) + (half ? TH : 0) + l32] = wc;
            const unsigned long long bc = __ballot(final_before(wc));
            colL = bc & 0xFFFFFFFFull; colR = bc >> 32;
        } else {
            const uint32_t wl = stage_word(i0 + lane, j0 - 1), wq = stage_word(i0 + lane, j0 + TT);
            colL = __ballot(final_before(wl)); colR = __ballot(final_before(wq));
        }
        const bool fr = final_before(wr), fk = lane < 4 && final_before(wk);
        const unsigned long long br = __ballot(fr), bk = __ballot(fk);
        if (lane == 0) {
            L.fin[0] = ((br & 0xFFFFFFFFull) << 1) | (bk & 1ull) | (((bk >> 1) & 1ull) << 33);
            L.fin[HH - 1] = ((br >> 32) << 1) | ((bk >> 2) & 1ull) | (((bk >> 3) & 1ull) << 33);
        }
    }
    constexpr int STG_B = PYDEM_STG_B;
#pragma unroll 1
    for (int kb = 0; kb < NSET; kb += STG_B) {
        uint32_t wst[STG_B];
#pragma unroll
        for (int k = 0; k < STG_B; k++) wst[k] = stage_word(i0 + 2 * (kb + k) + half, j0 + l32);
#pragma unroll
        for (int k = 0; k < STG_B; k++) {
            const int r = 2 * (kb + k);                                  // this load: local rows r + 1 (lanes 0-31), r + 2
            const bool f = final_before(wst[k]);
            L.cs[lane + 64 * (kb + k)] = ((wst[k] == 0xFFFFFFFFu ? 0u : (wst[k] & CI_STATIC_MASK)) << 16) | ((f ? 1u : 0u) << SP_STATE_SHIFT);
            const unsigned long long b = __ballot(f);
            if (lane == 0) {
                L.fin[r + 1] = ((b & 0xFFFFFFFFull) << 1) | ((colL >> r) & 1ull) | (((colR >> r) & 1ull) << 33);
                L.fin[r + 2] = ((b >> 32) << 1) | ((colL >> (r + 1)) & 1ull) | (((colR >> (r + 1)) & 1ull) << 33);
            }
        }
    }
}

// WT (the weighted sweep, pydem_uca_weighted): A.a0 holds a seed per CELL instead of the cell area per row, and the shares are
// summed with their signs -- a weight may be zero or negative, so the edge_todo taint cannot ride in the sign and is left out
template <bool LISTED, bool WT = false>
__device__ __forceinline__ void sweep_one_tile(const SweepArgs &A, TileW &L, uint32_t pass, int tiles_x, int tid, int lane,
                                               uint8_t *__restrict__ tile_done, int32_t &n_final, const TileNext &N,
                                               int32_t *pend, int &npend, const int32_t *nbr16)
{
    const int by = tid / tiles_x, bx = tid - by * tiles_x;
    const int i0 = by * TH, j0 = bx * TT, n = A.n, m = A.m;
    const TileBase B = tile_base(A, i0, j0);
    const int half = lane >> 5, l32 = lane & 31;         // interior cell k of a lane: row 2k + half, column l32 of the tile
    // ready-list push; `consumed` = entries already processed (ring occupancy = tail - consumed)
    auto push_ready = [&](int cell, int consumed) {
        const int slot = atomicAdd(&L.tail, 1);
        if (slot - consumed < TILE_RING) L.list[slot % TILE_RING] = (uint16_t)cell;
        else atomicMin(&L.limit, slot);
    };
#ifdef PYDEM_TILE_PROF
    const bool prof = (A.dbg & 4) != 0 && (int)pass >= (A.dbg >> 8);      // PYDEM_TILE_DEBUG = 4 + 256 * first pass to account
#else
    constexpr bool prof = false;       // (the phase timers cost registers: build with -DPYDEM_TILE_PROF to use PYDEM_TILE_DEBUG=4)
#endif
    long long tk0 = 0, tk1 = 0, tk2 = 0, tk3 = 0;
    int nrounds = 0;
    if (prof) tk0 = wall_clock64();
    if (lane == 0) { L.tail = 0; L.limit = INT32_MAX; }
    const double a0_row = (!WT && lane < TH && i0 + lane < n) ? A.a0[i0 + lane] : 0.0;       // lands in LDS once the final bitmap is no longer needed
    constexpr int NSET = TH * TT / 64;
    tile_stage(A, B, L, pass, i0, j0, lane);
    tile_wave_sync();
    if (prof) tk1 = wall_clock64();
    // ---- per-cell setup: how many upstream cells are still open = in-mask bits whose neighbour is not final (three row
    // words of the final bitmap, LDS broadcasts) ...
    uint32_t pitmask = 0;
    int32_t n_open = 0;
#pragma unroll 2
    for (int k = 0; k < NSET; k++) {
        const int li = 2 * k + half + 1, idx = lane + 64 * k;
        const uint32_t w = L.cs[idx];
        if (!((w >> SP_STATE_SHIFT) & 3u)) {                        // open (cells outside the grid were staged as final)
            const unsigned long long f0 = L.fin[li - 1], f1 = L.fin[li], f2 = L.fin[li + 1];
            const uint32_t nf = ((uint32_t)(f0 >> l32) & 7u) | (((uint32_t)(f1 >> l32) & 1u) << 3) |
                                (((uint32_t)(f1 >> (l32 + 2)) & 1u) << 4) | (((uint32_t)(f2 >> l32) & 7u) << 5);
            const uint32_t pend = __popc((w >> 16) & 0xFFu & ~nf);
            sp_of(L, idx) = (uint16_t)pend;                         // the state bits of an open cell are zero: the half-word is the count
            n_open++;
            if (w & (CI_PIT_IN << 16)) pitmask |= 1u << k;
            else if (pend == 0) push_ready(lane + 64 * k, 0);
        }
    }
    // ... then the pit in-edges of the lane's drains: their list offsets in one batch, the edges two loads at a time
    if (pitmask) {
        constexpr int PB = 4;
#pragma unroll 1
        for (int kb = 0; kb < NSET; kb += PB) {
            if (!((pitmask >> kb) & ((1u << PB) - 1u))) continue;
            int32_t e0[PB];
#pragma unroll
            for (int k = 0; k < PB; k++) {
                e0[k] = 0;
                if (pitmask & (1u << (kb + k))) {
                    const int cell = lane + 64 * (kb + k);
                    e0[k] = ld_off<int2>(B.area, halo_cell((cell >> 5) + 1, (cell & 31) + 1, m) * 8u).x;
                }
            }
#pragma unroll
            for (int k = 0; k < PB; k++) {
                if (!(pitmask & (1u << (kb + k)))) continue;
                const int cell = lane + 64 * (kb + k);
                const int32_t c = B.org + (int32_t)halo_cell((cell >> 5) + 1, (cell & 31) + 1, m);
                const int idx = cell;
                uint32_t pend = sp_of(L, idx);
                for (int32_t e = e0[k];; e += 2) {                  // pit -> drain edges are short: most sources sit in this tile
                    const int64_t ia = e < A.n_pit ? e : A.n_pit - 1, ib = e + 1 < A.n_pit ? e + 1 : A.n_pit - 1;
                    const int32_t da = A.pin_dst[ia], db = A.pin_dst[ib], sa = A.pin_src[ia], sb = A.pin_src[ib];
                    const bool va = e < A.n_pit && da == c, vb = va && e + 1 < A.n_pit && db == c;
                    auto blocked = [&](int32_t sc) -> uint32_t {
                        const int si = sc / m - i0, sj = sc % m - j0;
                        if (si >= 0 && si < TH && sj >= 0 && sj < TT)
                            return sp_state(L, si * TT + sj) ? 0u : 1u;          // released on chip when the pit finishes
                        const uint32_t lv = ci_level(A.cinfo[sc]);
                        return (lv >= 1 && lv < pass) ? 0u : SP_BLOCKED;                   // another tile's business: blocked for this pass
                    };
                    uint32_t ba = 0, bb = 0;
                    if (va) ba = blocked(sa);
                    if (vb) bb = blocked(sb);
                    pend = (pend + (ba & 1u) + (bb & 1u)) | ((ba | bb) & SP_BLOCKED);
                    if (!vb) break;
                }
                sp_of(L, idx) = (uint16_t)pend;
                if (pend == 0) push_ready(cell, 0);
            }
        }
    }
    tile_wave_sync();
    if (lane < TH) L.a0[lane] = a0_row;                  // (the final bitmap is dead now)
    tile_wave_sync();
    // ---- rounds: the ready cells [head, tail) are processed, the targets they release are appended
    if (prof) tk2 = wall_clock64();
    int32_t finalized = 0;
    uint32_t wake = 0;                 // bit (dti + 1) * 3 + dtj + 1: a finished cell drains into that neighbour tile
    int head = 0;
    // A lane that finishes a cell and thereby makes one of its targets ready keeps that target for itself ("chain"):
    // the next iteration needs neither the ready list (three dependent LDS operations) nor a load of the contribution it
    // has just stored (a load behind a pending write-through store waits for the store's round trip) -- the share travels
    // in a register.  Along a river this is the whole critical path of a tile visit.  Lanes without a chained cell take
    // the next entries of the ready list.
    int mycell = -1, cd = -1;          // the lane's cell (tile-local id), the in-edge (bit of the in-mask) the chained share arrives by
    double cv = 0.0;                   // the chained share
    for (;;) {
        const int tail = L.tail < L.limit ? L.tail : L.limit;
        const bool need = mycell < 0;
        const unsigned long long nb = __ballot(need);
        const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(nb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nb, 0u));
        const int avail = tail - head, wanted = __popcll(nb);
        if (need && rank < avail) { mycell = L.list[(head + rank) % TILE_RING]; cd = -1; }
        head += wanted < avail ? wanted : avail;
        if (!__ballot(mycell >= 0)) break;
        nrounds++;
        int next = -1, nd = -1;
        double nv = 0.0;
        if (mycell >= 0) {
            const int cell = mycell;
            const int li = (cell >> 5) + 1, lj = (cell & 31) + 1, idx = cell;
            const int gi = i0 + li - 1, gj = j0 + lj - 1;
            const uint32_t h = halo_cell(li, lj, m);                 // the cell in halo coordinates: offsets into the five planes
            const int32_t c = B.org + (int32_t)h;
            const uint32_t cw = L.cs[idx] >> 16;
            // everything that only needs (c, cw): proportion, pit slots, the in-edge contributions (most cells have one
            // or two in-edges: walk the set bits, in ascending order like the reference's pull, four loads in flight)
            double pv = 0.0;
            if (cw & (CI_OUT1 | CI_OUT2)) pv = ld_off<double>(B.prop, h * 8u);
            int2 po = make_int2(0, 0);
            if (cw & (CI_PIT_IN | CI_PIT_OUT)) po = ld_off<int2>(B.area, h * 8u);
            uint32_t mm = cw & 0xFFu;
            double xs[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                xs[q] = 0.0;
                if (mm) {
                    const int d = __ffs(mm) - 1; mm &= mm - 1u;
                    if (d == cd) xs[q] = cv; else xs[q] = in_edge_h(B, nbr16, h, d);
                }
            }
            double a;
            bool td;
            if constexpr (WT) {
                a = A.a0[c];
                td = false;
#pragma unroll
                for (int q = 0; q < 4; q++) a += xs[q];
            } else {
                a = L.a0[li - 1];
                td = (gi == 0 || gi == n - 1 || gj == 0 || gj == m - 1) && ld_off<uint8_t>(B.todo, h) != 0;
#pragma unroll
                for (int q = 0; q < 4; q++) { a += fabs(xs[q]); td = td || (xs[q] < 0); }       // (+0.0 leaves the positive sum as it is)
            }
            while (mm) {                                                                    // five and more in-edges: rare
                const int d = __ffs(mm) - 1; mm &= mm - 1u;
                const double x = (d == cd) ? cv : in_edge_h(B, nbr16, h, d);
                if constexpr (WT) a += x;
                else { a += fabs(x); td = td || (x < 0); }
            }
            if (cw & CI_PIT_IN)
                for (int32_t e = po.x; e < A.n_pit && A.pin_dst[e] == c; e++) {
                    const int32_t sc = A.pin_src[e];
                    a += A.area[sc] * A.pin_w[e];
                    if constexpr (!WT) td = td || (A.todo_work[sc] != 0);
                }
            double2 o = make_double2(0.0, 0.0);
            if (cw & CI_OUT1) o.x = a * pv;
            if (cw & CI_OUT2) o.y = a * (1 - pv);
            if (td) { o.x = -o.x; o.y = -o.y; }
            st_off<double>(B.area, h * 8u, a);
#ifndef PYDEM_EXP_NOCONTRIB      // timing experiment: the tile visits without their 16-byte contribution stores
            st_off<double2>(B.contrib, h * 16u, o);
#endif
            if (LISTED) st_off<uint32_t>(B.cinfo, h * 4u, ci_with_level(cw, pass));    // finished in this pass (other tiles treat levels < their pass as final)
            if (td) st_off<uint8_t>(B.todo, h, (uint8_t)1);
            sp_of(L, idx) = (uint16_t)(2u << SP_STATE_SHIFT);
            finalized++;
            // release the targets inside the tile; targets in other tiles may be ready now: their tiles run in the
            // next pass (listing a tile whose cell still waits for somebody else costs one idle staging; whoever
            // finishes last lists it again)
            auto release = [&](int ti, int tj, double share, bool chainable) {      // tile-local coordinates 1..TT when inside
                if (ti >= 1 && ti <= TH && tj >= 1 && tj <= TT) {
                    const int tcell = (ti - 1) * TT + (tj - 1);
                    if (sp_dec(L, tcell) == 1u) {
                        if (chainable && next < 0) {
                            const int q = (li - ti + 1) * 3 + (lj - tj + 1);          // where this cell sits in the target's 3x3 window
                            next = tcell; nd = q - (q > 4 ? 1 : 0); nv = share;
                        } else push_ready(tcell, head);
                    }
                } else if (LISTED) {
                    // (out-edges only exist towards cells of the grid.)  The eight neighbour tiles are woken once, after
                    // the rounds: two dependent returning atomics per cell would sit on every round's critical path
                    const int dti = ti < 1 ? -1 : (ti > TH ? 1 : 0), dtj = tj < 1 ? -1 : (tj > TT ? 1 : 0);
                    if (ti >= 1 - TH && ti <= 2 * TH && tj >= 1 - TT && tj <= 2 * TT) wake |= 1u << ((dti + 1) * 3 + dtj + 1);
                    else {                                            // a pit draining further away than the next tile
                        const int tt = ((i0 + ti - 1) / TH) * tiles_x + (j0 + tj - 1) / TT;
                        if (atomicExch(&N.flag[tt], (int32_t)pass + 1) != (int32_t)pass + 1) N.list[atomicAdd(N.count, 1)] = tt;
                    }
                }
            };
            const int sct = ci_section(cw);
            if (cw & CI_OUT1) release(li + fe1r(sct), lj + fe1c(sct), o.x, true);
            if (cw & CI_OUT2) release(li + fe2r(sct), lj + fe2c(sct), o.y, true);
            if (cw & CI_PIT_OUT)
                for (int32_t e = po.y; e < A.n_pit && A.pit_src[e] == c; e++) {
                    const int32_t dc = A.pit_dst[e];
                    const int ti = dc / m - i0 + 1, tj = dc % m - j0 + 1;
                    // a drain inside the tile that an earlier pass already finished cannot exist (it waits for this pit)
                    release(ti, tj, 0.0, false);
                }
        }
        mycell = next; cd = nd; cv = nv;
        tile_wave_sync();
    }
    // ---- the tile is done when every cell that was open at setup has been finished.  A pass that revisits a tile
    // finishes few cells and stamps their level as it goes; the first pass finishes most of the tile and stamps in rows
    if (prof) tk3 = wall_clock64();
    if (!LISTED)
        for (int k = 0; k < NSET; k++) {
            const int li = 2 * k + half + 1, idx = lane + 64 * k;
            const uint32_t w = L.cs[idx];
            if (((w >> SP_STATE_SHIFT) & 3u) == 2u) A.cinfo[(int64_t)(i0 + li - 1) * m + j0 + l32] = ci_with_level(w >> 16, pass);
        }
    for (int off = 32; off > 0; off >>= 1) { finalized += __shfl_down(finalized, off); n_open += __shfl_down(n_open, off); }
    if (LISTED) {
        // the tiles this visit wakes (lanes 0-8: the neighbours a finished cell drains into; lane 9: the tile itself when
        // its ready ring overflowed) go to the wavefront's pending list; the kernel appends the pending lists to the
        // global one with one add per wavefront / workgroup (tile_list_flush): the list counter is a single address too
        for (int off = 32; off > 0; off >>= 1) wake |= __shfl_xor(wake, off);
        bool win = false;
        int tt = 0;
        if (lane < 9 && ((wake >> lane) & 1u)) { tt = tid + (lane / 3 - 1) * tiles_x + (lane % 3 - 1); win = true; }
        if (lane == 9 && L.limit != INT32_MAX) { tt = tid; win = true; }
        if (win) win = atomicExch(&N.flag[tt], (int32_t)pass + 1) != (int32_t)pass + 1;
        const unsigned long long bw = __ballot(win);
        if (win) pend[npend + __popcll(bw & ((1ull << lane) - 1ull))] = tt;
        npend += __popcll(bw);
    }
    if (lane == 0) {
        n_final += finalized;          // (lane 0's running count: the kernel adds it to the global counter once, see there)
        if (finalized == n_open) tile_done[tid] = 1;
        A.tile_open[tid] = n_open - finalized;
        if (prof) {      // cycles per phase, summed over tiles (PYDEM_TILE_DEBUG=4)
            const long long tk4 = wall_clock64();
            unsigned long long *acc = reinterpret_cast<unsigned long long *>(A.err + (CS_TILE_PROF - CS_QUEUE_ERR));   // see stage_sweep
            atomicAdd(acc + 0, (unsigned long long)(tk1 - tk0)); atomicAdd(acc + 1, (unsigned long long)(tk2 - tk1));
            atomicAdd(acc + 2, (unsigned long long)(tk3 - tk2)); atomicAdd(acc + 3, (unsigned long long)(tk4 - tk3));
            atomicAdd(acc + 4, (unsigned long long)nrounds); atomicAdd(acc + 5, 1ull);
            if (finalized == 0) atomicAdd(acc + 6, 1ull);
        }
    }
    tile_wave_sync();
}

#include "uca_sym.inl"

// every tile that is not done yet (LISTED: also lists the tiles of the next pass).  Persistent wavefronts, XCD-contiguous
// bands of tiles: workgroup b runs on XCD b % 8 and its wavefronts take the next tile of that XCD's band from the band's
// counter -- a visit lasts 20 .. 100 rounds, and with four fixed tiles per workgroup the LDS of a workgroup (an eighth of
// the CU's) sat behind its slowest visit (PYDEM_SWEEP_STATIC build: the round-3 mapping, for A/B runs)
#ifndef PYDEM_SWEEP_STEAL
#define PYDEM_SWEEP_STEAL 1          // bands a workgroup works on: its own XCD (8 = the others afterwards: measured 31.1 vs 29.3 ms of sweep -- slower)
#endif
#ifndef PYDEM_FULL_WPB
#define PYDEM_FULL_WPB 4            // wavefronts per workgroup of the two full passes
#endif
constexpr int FWPB = PYDEM_FULL_WPB;
template <bool LISTED, bool WT = false>
__global__ __launch_bounds__(64 * FWPB, 32 / FWPB) void k_sweep_tiles(SweepArgs A, uint32_t pass, int tiles_x, int tiles_total,
                                                     uint8_t *__restrict__ tile_done, int32_t *n_final, TileNext N, int32_t *work8)
{
    __shared__ TileW L[FWPB];
    __shared__ int32_t s_pend[FWPB][TILE_PEND];
    __shared__ int32_t s_nbr16[8];
    fill_nbr16(s_nbr16, A.m);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int32_t fin = 0;
    int npend = 0;
    auto flush = [&]() {
        tile_wave_sync();
        int32_t base = 0;
        if (lane == 0) base = atomicAdd(N.count, npend);
        base = __shfl(base, 0);
        if (lane < npend) N.list[base + lane] = s_pend[wave][lane];
        npend = 0;
        tile_wave_sync();
    };
#ifdef PYDEM_SWEEP_STATIC
    (void)work8;
    const int per4 = (gridDim.x >> 3) * 4;
    for (int tid = (blockIdx.x & 7) * per4 + (blockIdx.x >> 3) * 4 + wave, once = 0; once < 1; once++) {
        if (tid < tiles_total && !tile_done[tid])
            sweep_one_tile<LISTED, WT>(A, L[wave], pass, tiles_x, tid, lane, tile_done, fin, N, s_pend[wave], npend, s_nbr16);
    }
#else
    const int per = (tiles_total + 7) >> 3;
    // own band first, then the other XCDs' bands (their tails: a band of rough terrain takes longer than its neighbours)
    for (int st = 0; st < PYDEM_SWEEP_STEAL; st++) {
        const int xcd = (int)((blockIdx.x + st) & 7);
        for (;;) {
            int32_t q = 0;
            if (lane == 0) q = atomicAdd(&work8[xcd], 1);
            q = __builtin_amdgcn_readfirstlane(__shfl(q, 0));
            const int tid = xcd * per + q;
            if (q >= per || tid >= tiles_total) break;
            if (tile_done[tid]) continue;
            sweep_one_tile<LISTED, WT>(A, L[wave], pass, tiles_x, tid, lane, tile_done, fin, N, s_pend[wave], npend, s_nbr16);
            if (LISTED && npend > TILE_PEND - 10) flush();      // (a visit adds at most ten)
        }
    }
#endif
    if (LISTED && npend) flush();
    // the counter of finished cells is a single address: one add per wavefront
    if (lane == 0 && fin) atomicAdd(n_final, fin);
}

// later passes: only the listed tiles (those a finished cell of the previous pass drains into); lists the next ones.  The
// wavefronts take the list entries from a counter (work3[pass % 3]; the counter of the next pass is cleared here).
#ifndef PYDEM_LISTED_OCC
#define PYDEM_LISTED_OCC 6
#endif
#ifndef PYDEM_LISTED_WPB
#define PYDEM_LISTED_WPB 2          // wavefronts (= tiles in flight) per workgroup of the listed passes (same-box A/B: 4: 30.36, 1: 29.83, 2: 29.68 ms of sweep)
#endif
constexpr int LWPB = PYDEM_LISTED_WPB;
template <bool WT = false>
__global__ __launch_bounds__(64 * LWPB, PYDEM_LISTED_OCC) void k_sweep_tiles_listed(SweepArgs A, uint32_t pass, int tiles_x, const int32_t *__restrict__ list_in,
                                                            const int32_t *n_in, uint8_t *__restrict__ tile_done, int32_t *n_final,
                                                            TileNext N, int32_t *clear_count, int32_t *work3, SymArgs Y)
{
    __shared__ TileW L[LWPB];
    __shared__ SymLight SL[LWPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t nt = *n_in;
#ifdef PYDEM_LISTED_DYNAMIC
    if (blockIdx.x == 0 && threadIdx.x < 8) work3[((pass + 1) % 3) * 8 + threadIdx.x] = 0;         // the next pass's work counters
#endif
    if (blockIdx.x == 0 && threadIdx.x == 0) *clear_count = 0;                                     // the list of the pass after the next one
    // (the tile id is the same for the whole wavefront: as a scalar it keeps the tile's coordinates and every address
    // derived from them out of the vector registers)
    __shared__ int32_t s_pend[LWPB][TILE_PEND];
    __shared__ int32_t s_nbr16[8];
    fill_nbr16(s_nbr16, A.m);
    __syncthreads();
    int32_t fin = 0;               // finished cells of all tiles of this wavefront: one add at the end
    int npend = 0;                 // tiles woken by this wavefront's visits that are not on the global list yet
    auto flush = [&]() {
        tile_wave_sync();
        int32_t base = 0;
        if (lane == 0) base = atomicAdd(N.count, npend);
        base = __shfl(base, 0);
        if (lane < npend) N.list[base + lane] = s_pend[wave][lane];
        npend = 0;
        tile_wave_sync();
    };
#ifndef PYDEM_LISTED_DYNAMIC
    // (taking the list entries from counters like the full passes do was measured and is slower here: 2.74 / 2.18 / 1.68 ms
    // against 2.41 / 1.79 / 1.26 ms for passes 4-6 -- -DPYDEM_LISTED_DYNAMIC keeps the variant)
    (void)work3;
    for (int32_t k = __builtin_amdgcn_readfirstlane(blockIdx.x * LWPB + wave); k < nt; k += gridDim.x * LWPB) {
#else
    // eight counters (one per XCD's workgroups, each over an eighth of the list): a single one would see a grab per visit
    // from every wavefront of the chip -- 100 k returning atomics on one address per pass, ~10 ns each
    const int xcd = blockIdx.x & 7;
    const int32_t per = (nt + 7) >> 3;
    int32_t *wk = &work3[(pass % 3) * 8 + xcd];
    for (;;) {
        int32_t k = 0;
        if (lane == 0) k = atomicAdd(wk, 1);
        k = __builtin_amdgcn_readfirstlane(__shfl(k, 0));
        (void)per;
        k = k * 8 + xcd;                   // interleaved: the list is in wake order, contiguous eighths would be regions of unequal work
        if (k >= nt) break;
#endif
        const int tid = __builtin_amdgcn_readfirstlane(list_in[k]);
        const uint32_t blk = Y.tile_sym ? __builtin_amdgcn_readfirstlane(Y.tile_sym[tid]) : SYM_NONE;
        if (blk != SYM_NONE) sym_light_visit<WT>(A, Y, SL[wave], pass, tiles_x, tid, lane, blk, fin, N, s_pend[wave], npend);     // (a tile that went symbolic, K5f)
        else sweep_one_tile<true, WT>(A, L[wave], pass, tiles_x, tid, lane, tile_done, fin, N, s_pend[wave], npend, s_nbr16);
        if (npend > TILE_PEND - 10) flush();            // (a visit adds at most ten)
    }
    if (npend) flush();
    if (lane == 0 && fin) atomicAdd(n_final, fin);
}

// ------------------------------------------------------------------------------- K5d
// Dense level prologue (PYDEM_SWEEP_DENSE=k, measured alternative -- see DESIGN.md section 4 "Round 4"): k full-grid
// streaming kernels ahead of the tile passes.  Level p finishes every open cell whose sources all finished in a level
// < p: one lane per cell, no lists, no atomics besides the count, the same gather order as the tile visits (NW ... SE,
// then the pit in-edges by source), so the values are bit-identical to theirs.  A stamp of THIS level reads as "open"
// (levels < p count), so concurrent stamps never let a cell read a value written in the same launch.
// (WT: seed per cell, signed shares, no taint -- see sweep_one_tile)
constexpr int DENSE_BAND = 64;
template <bool WT = false>
__global__ __launch_bounds__(256) void k_sweep_dense_level(SweepArgs A, uint32_t p, int32_t *n_final)
{
    const int n = A.n, m = A.m;
    int32_t fin = 0;
    // a workgroup walks a band of DENSE_BAND consecutive rows of its 256 columns: the neighbour rows it reads were touched by
    // itself a row earlier (L1 / the XCD's L2), and the count of finished cells costs one atomic per band and column block
    // (one per row and block kept the counter's L2 channel busy for 12 ms per level)
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i_end = min(n, (int)(blockIdx.y + 1) * DENSE_BAND);
    if (j < m)
    for (int i = blockIdx.y * DENSE_BAND; i < i_end; i++) {
        const int32_t c = i * m + j;
        const uint32_t w = A.cinfo[c];
        const uint32_t lv = ci_level(w);
        if (lv >= 1 && lv != CI_LEVEL_INF) continue;                     // finished in an earlier level
        const uint32_t cw = w & CI_STATIC_MASK;
        bool ready = true;
#pragma unroll
        for (int d = 0; d < 8; d++)
            if (cw & (1u << d)) {
                const uint32_t lu = ci_level(A.cinfo[c + NB_DI[d] * m + NB_DJ[d]]);
                ready = ready && lu >= 1 && lu < p;
            }
        if (!ready) continue;
        int2 po = make_int2(0, 0);
        if (cw & CI_PIT_IN) {
            po = pit_stash(A, c);
            for (int32_t e = po.x; e < A.n_pit && A.pin_dst[e] == c; e++) {
                const uint32_t lu = ci_level(A.cinfo[A.pin_src[e]]);
                ready = ready && lu >= 1 && lu < p;
            }
            if (!ready) continue;
        }
        double a = WT ? A.a0[c] : A.a0[i];
        bool td = !WT && (i == 0 || i == n - 1 || j == 0 || j == m - 1) && A.todo_work[c] != 0;
#pragma unroll
        for (int d = 0; d < 8; d++)
            if (cw & (1u << d)) {
                const double x = in_edge(A, c, m, d);
                if constexpr (WT) a += x;
                else { a += fabs(x); td = td || (x < 0); }
            }
        if (cw & CI_PIT_IN)
            for (int32_t e = po.x; e < A.n_pit && A.pin_dst[e] == c; e++) {
                const int32_t sc = A.pin_src[e];
                a += A.area[sc] * A.pin_w[e];
                if constexpr (!WT) td = td || (A.todo_work[sc] != 0);
            }
        double2 o = make_double2(0.0, 0.0);
        if (cw & (CI_OUT1 | CI_OUT2)) {
            const double pv = A.prop[c];
            if (cw & CI_OUT1) o.x = a * pv;
            if (cw & CI_OUT2) o.y = a * (1 - pv);
            if (td) { o.x = -o.x; o.y = -o.y; }
        }
        A.area[c] = a;
        A.contrib[c] = o;
        A.cinfo[c] = ci_with_level(cw, p);
        if (td) A.todo_work[c] = 1;
        fin++;
    }
    for (int off = 32; off > 0; off >>= 1) fin += __shfl_down(fin, off);
    __shared__ int32_t s_fin;
    if (threadIdx.x == 0) s_fin = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && fin) atomicAdd(&s_fin, fin);
    __syncthreads();
    if (threadIdx.x == 0 && s_fin) atomicAdd(n_final, s_fin);
}

// ------------------------------------------------------------------------------- K5e
// Resident visits for the river passes.  After a dozen passes the listed tiles have a few dozen open cells each, and a
// pass lasts as long as its longest dependency chain: rounds per visit x time per round.  The generic round goes
// through global memory for every cell (proportion, in-edge shares, results, a fence that waits for the stores); here
// the open cells of the tile get SLOTS in LDS -- (K, p) = constant part of the area (cell area + shares of the upstream
// cells that are final already) and proportion, fetched for all open cells at once before the rounds --, the rounds
// only touch LDS, and the results leave the CU once after the last round.  A tile with more open cells than slots
// takes the generic visit (sweep_one_tile).  The sum of a cell's in-edges is taken over the final ones first and the
// ones finished in this visit second, both ascending (the generic visit: ascending over all of them).
constexpr int RCAP = 256;
constexpr uint32_t RS_TAINT = 1u << 19, RS_FIN = 1u << 20;      // slot word: bits 0-10 cell, 11-18 in-edges from cells open at setup
constexpr int RS_OPEN_SHIFT = 11, RS_FINAL_SHIFT = 21;          //            bits 21-28 in-edges from cells final at setup
constexpr uint32_t RS_CELL = (1u << RS_OPEN_SHIFT) - 1u, RS_CELL_OPEN = (1u << 19) - 1u;

struct TileR {
    TileW W;                    // staging, final bitmap, count-downs as in the generic visit; W.list = ready SLOTS (each enters once)
    uint16_t map[TH * TT];      // cell -> slot (only read for cells that were open at setup)
    double Kd[RCAP];            // constant part while the cell is open, its area once it is finished
    double Pd[RCAP];            // proportion
    uint32_t sm[RCAP];          // slot word
};

// tile-local id of the neighbour in-edge d (0..7 = NW N NE W E SW S SE) comes from
__device__ __forceinline__ int nb_local(int cell, int d)
{
    const int q = d + (d >> 2);
    const int di = (q * 11) >> 5;
    return cell + (di - 1) * TT + (q - 3 * di - 1);
}

template <bool WT = false>
__device__ __forceinline__ void sweep_tile_resident(const SweepArgs &A, TileR &R, uint32_t pass, int tiles_x, int tid, int lane,
                                                    uint8_t *__restrict__ tile_done, int32_t &n_final, const TileNext &N,
                                                    int32_t *pend, int &npend)
{
    TileW &L = R.W;
    const int by = tid / tiles_x, bx = tid - by * tiles_x;
    const int i0 = by * TH, j0 = bx * TT, n = A.n, m = A.m;
    const int half = lane >> 5, l32 = lane & 31;
    constexpr int NSET = TH * TT / 64;
    if (lane == 0) L.tail = 0;
    const double a0_row = (!WT && lane < TH && i0 + lane < n) ? A.a0[i0 + lane] : 0.0;
    tile_stage(A, tile_base(A, i0, j0), L, pass, i0, j0, lane);
    tile_wave_sync();
    // ---- setup: open-upstream counts (as in the generic visit) and a slot per open cell
    uint32_t pitmask = 0;
    int nslot = 0;
#pragma unroll 2
    for (int k = 0; k < NSET; k++) {
        const int li = 2 * k + half + 1, idx = lane + 64 * k;
        const uint32_t w = L.cs[idx];
        const bool open = !((w >> SP_STATE_SHIFT) & 3u);
        const unsigned long long bo = __ballot(open);
        if (open) {
            const unsigned long long f0 = L.fin[li - 1], f1 = L.fin[li], f2 = L.fin[li + 1];
            const uint32_t nf = ((uint32_t)(f0 >> l32) & 7u) | (((uint32_t)(f1 >> l32) & 1u) << 3) |
                                (((uint32_t)(f1 >> (l32 + 2)) & 1u) << 4) | (((uint32_t)(f2 >> l32) & 7u) << 5);
            const uint32_t im = (w >> 16) & 0xFFu;
            const uint32_t cnt = __popc(im & ~nf);
            sp_of(L, idx) = (uint16_t)cnt;
            const int s = nslot + __popcll(bo & ((1ull << lane) - 1ull));
            R.map[idx] = (uint16_t)s;
            R.sm[s] = (uint32_t)idx | ((im & ~nf) << RS_OPEN_SHIFT) | ((im & nf) << RS_FINAL_SHIFT);
            if (w & (CI_PIT_IN << 16)) pitmask |= 1u << k;
            else if (cnt == 0) L.list[atomicAdd(&L.tail, 1)] = (uint16_t)s;
        }
        nslot += __popcll(bo);
    }
    // pit in-edges of the lane's drains: sources open in this tile are released on chip, sources another tile has not
    // finished block the drain for this pass
    if (pitmask) {
#pragma unroll 1
        for (int k = 0; k < NSET; k++) {
            if (!(pitmask & (1u << k))) continue;
            const int cell = lane + 64 * k;
            const int32_t c = (i0 + (cell >> 5)) * m + j0 + (cell & 31);
            uint32_t cnt = sp_of(L, cell);
            for (int32_t e = pit_stash(A, c).x; e < A.n_pit && A.pin_dst[e] == c; e++) {
                const int32_t sc = A.pin_src[e];
                const int si = sc / m - i0, sj = sc % m - j0;
                if (si >= 0 && si < TH && sj >= 0 && sj < TT) cnt += sp_state(L, si * TT + sj) ? 0u : 1u;
                else { const uint32_t lv = ci_level(A.cinfo[sc]); if (!(lv >= 1 && lv < pass)) cnt |= SP_BLOCKED; }
            }
            sp_of(L, cell) = (uint16_t)cnt;
            if (cnt == 0) L.list[atomicAdd(&L.tail, 1)] = R.map[cell];
        }
    }
    tile_wave_sync();
    if (lane < TH) L.a0[lane] = a0_row;                  // (the final bitmap is dead now)
    tile_wave_sync();
    // ---- the constant part of every open cell: all its loads in flight together
    for (int s = lane; s < nslot; s += 64) {
        uint32_t smv = R.sm[s];
        const int cell = smv & RS_CELL;
        const int gi = i0 + (cell >> 5), gj = j0 + (cell & 31);
        const int32_t c = gi * m + gj;
        const uint32_t cw = L.cs[cell] >> 16;
        double pv = 0.0;
        if (cw & (CI_OUT1 | CI_OUT2)) pv = A.prop[c];
        bool td = !WT && (gi == 0 || gi == n - 1 || gj == 0 || gj == m - 1) && A.todo_work[c] != 0;
        uint32_t mm = (smv >> RS_FINAL_SHIFT) & 0xFFu;
        double xs[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            xs[q] = 0.0;
            if (mm) { const int d = __ffs(mm) - 1; mm &= mm - 1u; xs[q] = in_edge(A, c, m, d); }
        }
        double K;
        if constexpr (WT) {
            K = A.a0[c];
#pragma unroll
            for (int q = 0; q < 4; q++) K += xs[q];
            while (mm) { const int d = __ffs(mm) - 1; mm &= mm - 1u; K += in_edge(A, c, m, d); }
        } else {
            K = L.a0[cell >> 5];
#pragma unroll
            for (int q = 0; q < 4; q++) { K += fabs(xs[q]); td = td || (xs[q] < 0); }
            while (mm) { const int d = __ffs(mm) - 1; mm &= mm - 1u; const double x = in_edge(A, c, m, d); K += fabs(x); td = td || (x < 0); }
        }
        R.Kd[s] = K; R.Pd[s] = pv;
        R.sm[s] = (smv & RS_CELL_OPEN) | (td ? RS_TAINT : 0u);
    }
    tile_lds_sync();
    // ---- rounds on LDS
    uint32_t wake = 0;
    int head = 0;
    for (;;) {
        const int tail = L.tail;
        if (head >= tail) break;
        const int idx = head + lane;
        if (idx < tail) {
            // (a lane that went on at once with a target its cell released -- no list, no barrier -- was measured: slower,
            // the other branch of a braided river waits in the list meanwhile)
            const int s = L.list[idx];
            const uint32_t smv = R.sm[s];
            const int cell = smv & RS_CELL, li = cell >> 5, lj = cell & 31;
            const uint32_t cw = L.cs[cell] >> 16;
            double a = R.Kd[s];
            bool td = (smv & RS_TAINT) != 0u;
            uint32_t mm = (smv >> RS_OPEN_SHIFT) & 0xFFu;       // sources of this tile that were open at setup: finished in this visit
            while (mm) {
                const int d = __ffs(mm) - 1; mm &= mm - 1u;
                const int ss = R.map[nb_local(cell, d)];
                const double as = R.Kd[ss], ps = R.Pd[ss];
                a += ((0x5A >> d) & 1) ? as * ps : as * (1 - ps);
                td = td || (R.sm[ss] & RS_TAINT);
            }
            const int32_t c = (i0 + li) * m + j0 + lj;
            int2 po = make_int2(0, 0);
            if (cw & (CI_PIT_IN | CI_PIT_OUT)) po = pit_stash(A, c);
            if (cw & CI_PIT_IN)
                for (int32_t e = po.x; e < A.n_pit && A.pin_dst[e] == c; e++) {
                    const int32_t sc = A.pin_src[e];
                    const int si = sc / m - i0, sj = sc % m - j0;
                    bool here = false;
                    if (si >= 0 && si < TH && sj >= 0 && sj < TT) here = sp_state(L, si * TT + sj) == 2u;      // finished in this visit
                    if (here) { const int ss = R.map[si * TT + sj]; a += R.Kd[ss] * A.pin_w[e]; td = td || (R.sm[ss] & RS_TAINT); }
                    else { a += A.area[sc] * A.pin_w[e]; if constexpr (!WT) td = td || (A.todo_work[sc] != 0); }
                }
            R.Kd[s] = a;
            R.sm[s] = (smv & RS_CELL) | (td ? RS_TAINT : 0u) | RS_FIN;
            sp_of(L, cell) = (uint16_t)(2u << SP_STATE_SHIFT);
            auto release = [&](int ti, int tj) {            // tile-local coordinates 0..TT-1 when inside
                if (ti >= 0 && ti < TH && tj >= 0 && tj < TT) {
                    const int tcell = ti * TT + tj;
                    if (sp_dec(L, tcell) == 1u) L.list[atomicAdd(&L.tail, 1)] = R.map[tcell];
                } else {
                    const int dti = ti < 0 ? -1 : (ti >= TH ? 1 : 0), dtj = tj < 0 ? -1 : (tj >= TT ? 1 : 0);
                    if (ti >= -TH && ti < 2 * TH && tj >= -TT && tj < 2 * TT) wake |= 1u << ((dti + 1) * 3 + dtj + 1);
                    else {
                        const int tt = ((i0 + ti) / TH) * tiles_x + (j0 + tj) / TT;
                        if (atomicExch(&N.flag[tt], (int32_t)pass + 1) != (int32_t)pass + 1) N.list[atomicAdd(N.count, 1)] = tt;
                    }
                }
            };
            const int sct = ci_section(cw);
            if (cw & CI_OUT1) release(li + fe1r(sct), lj + fe1c(sct));
            if (cw & CI_OUT2) release(li + fe2r(sct), lj + fe2c(sct));
            if (cw & CI_PIT_OUT)
                for (int32_t e = po.y; e < A.n_pit && A.pit_src[e] == c; e++) {
                    const int32_t dc = A.pit_dst[e];
                    release(dc / m - i0, dc % m - j0);
                }
        }
        head = tail < head + 64 ? tail : head + 64;
        tile_lds_sync();
    }
    // ---- results of the finished cells
    int nfin = 0;
    for (int s = lane; s < nslot; s += 64) {
        const uint32_t smv = R.sm[s];
        if (!(smv & RS_FIN)) continue;
        const int cell = smv & RS_CELL;
        const int32_t c = (i0 + (cell >> 5)) * m + j0 + (cell & 31);
        const uint32_t cw = L.cs[cell] >> 16;
        const double a = R.Kd[s], pv = R.Pd[s];
        double2 o = make_double2(0.0, 0.0);
        if (cw & CI_OUT1) o.x = a * pv;
        if (cw & CI_OUT2) o.y = a * (1 - pv);
        if (smv & RS_TAINT) { o.x = -o.x; o.y = -o.y; A.todo_work[c] = 1; }
        A.area[c] = a;
        A.contrib[c] = o;
        A.cinfo[c] = ci_with_level(cw, pass);
        nfin++;
    }
    for (int off = 32; off > 0; off >>= 1) { nfin += __shfl_down(nfin, off); wake |= __shfl_xor(wake, off); }
    bool win = false;
    int tt = 0;
    if (lane < 9 && ((wake >> lane) & 1u)) { tt = tid + (lane / 3 - 1) * tiles_x + (lane % 3 - 1); win = true; }
    if (win) win = atomicExch(&N.flag[tt], (int32_t)pass + 1) != (int32_t)pass + 1;
    const unsigned long long bw = __ballot(win);
    if (win) pend[npend + __popcll(bw & ((1ull << lane) - 1ull))] = tt;
    npend += __popcll(bw);
    if (lane == 0) {
        n_final += nfin;
        A.tile_open[tid] = nslot - nfin;
        if (nfin == nslot) tile_done[tid] = 1;
    }
    tile_wave_sync();
}

// listed passes with few tiles: one wavefront (= one workgroup) per tile, resident visit when the tile's open cells fit
template <bool WT = false>
__global__ __launch_bounds__(64) void k_sweep_tiles_resident(SweepArgs A, uint32_t pass, int tiles_x, const int32_t *__restrict__ list_in,
                                                             const int32_t *n_in, uint8_t *__restrict__ tile_done, int32_t *n_final,
                                                             TileNext N, int32_t *clear_count, SymArgs Y)
{
    __shared__ TileR R;
    __shared__ SymLight SL;
    __shared__ int32_t s_pend[TILE_PEND];
    __shared__ int32_t s_nbr16[8];
    fill_nbr16(s_nbr16, A.m);
    __syncthreads();
    const int lane = threadIdx.x;
    const int32_t nt = *n_in;
    if (blockIdx.x == 0 && lane == 0) *clear_count = 0;
    int32_t fin = 0;
    int npend = 0;
    auto flush = [&]() {
        tile_wave_sync();
        int32_t base = 0;
        if (lane == 0) base = atomicAdd(N.count, npend);
        base = __shfl(base, 0);
        if (lane < npend) N.list[base + lane] = s_pend[lane];
        npend = 0;
        tile_wave_sync();
    };
    for (int32_t k = blockIdx.x; k < nt; k += gridDim.x) {
        const int tid = __builtin_amdgcn_readfirstlane(list_in[k]);
        const uint32_t blk = Y.tile_sym ? __builtin_amdgcn_readfirstlane(Y.tile_sym[tid]) : SYM_NONE;
        if (blk != SYM_NONE) sym_light_visit<WT>(A, Y, SL, pass, tiles_x, tid, lane, blk, fin, N, s_pend, npend);
        else if (__builtin_amdgcn_readfirstlane(A.tile_open[tid]) <= RCAP)
            sweep_tile_resident<WT>(A, R, pass, tiles_x, tid, lane, tile_done, fin, N, s_pend, npend);
        else
            sweep_one_tile<true, WT>(A, R.W, pass, tiles_x, tid, lane, tile_done, fin, N, s_pend, npend, s_nbr16);
        if (npend > TILE_PEND - 10) flush();
    }
    if (npend) flush();
    if (lane == 0 && fin) atomicAdd(n_final, fin);
}

// ------------------------------------------------------------------------------- K5a
// The first pass over a tile is special: nothing is final yet, so a cell can only be finished if its whole upstream
// closure lies inside the tile (and involves no pit edge).  Most cells are like that (~2/3 of a fractal tile), and for
// them nothing but the area has to leave the CU before the visit ends: one WORKGROUP of four wavefronts owns the tile,
// every thread OWNS 4 cells (row 8k + t / 32, column t % 32), and per cell LDS holds one word (graph bits + count-down of the open upstream
// cells) and one 16-byte slot that carries the cell's proportion until the cell is finished and its two contributions
// afterwards (20 KB per tile: eight tiles per CU).  A round: every thread reads the words of its own open cells,
// finishes those whose count reached zero -- in-edge gather from LDS in the same ascending order
// as process_cell(), arithmetic identical -- and counts its in-tile targets down with non-returning LDS atomics (the
// owner sees the zero in the next round).  At the end the rows of the tile are written once, coalesced: contribution
// 16 B + graph word 4 B per finished cell; the generic pass stored them in dependency order and paid ~47 B of write
// traffic per finished cell for 28 (profiles/README.md).  Cells with pit edges, cells fed from another tile and
// everything downstream of them are left to pass 2.  (WT: the seed of a cell comes from global memory when the cell is finished,
// signed shares, no taint -- see sweep_one_tile)
constexpr uint32_t FC_COUNT = 0xFu, FC_BLOCKED = 1u << 8, FC_DONE = 1u << 9, FC_TODO = 1u << 10;   // low half of the cell word

struct TileFirst {
    double2 slot[TT * TT];      // .x = proportion while the cell is open; (share 1, share 2) once it is finished
    uint32_t cs[TT * TT];       // high half: static graph bits, low half: FC_*
    double a0[TT];
};

// workgroup barrier that orders LDS traffic only: the global stores of a round (areas, fire-and-forget) are not waited for
__device__ __forceinline__ void lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <bool WT = false>
__global__ __launch_bounds__(256) void k_sweep_first(SweepArgs A, int tiles_x, int tiles_total, uint8_t *__restrict__ tile_done,
                                                     int32_t *n_final)
{
    __shared__ TileFirst L;
    __shared__ int32_t s_fin[2], s_any[2];
    const int t = threadIdx.x;
    const int per = gridDim.x >> 3;                 // workgroup b runs on XCD b % 8: one contiguous band of tiles per XCD
    const int tid = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (tid >= tiles_total) return;
    const int by = tid / tiles_x, bx = tid - by * tiles_x;
    const int i0 = by * TT, j0 = bx * TT, n = A.n, m = A.m;
    const int r0 = t >> 5, l32 = t & 31;            // the thread's cell k: row 8k + r0, column l32 (idx = t + 256 k)
    const int gj = j0 + l32;
    constexpr int NSET = TT * TT / 256;
    uint32_t ingrid = 0;                             // bit k: the thread's cell k exists
    if (t < 2) { s_fin[t] = 0; s_any[t] = 0; }
    {
        // ---- stage: graph words and proportions of the thread's cells, all loads in flight at once
        uint32_t cw[NSET];
        double pv[NSET];
#pragma unroll
        for (int k = 0; k < NSET; k++) {
            const int gi = i0 + 8 * k + r0;
            const bool ok = gi < n && gj < m;
            const int64_t c = (int64_t)gi * m + gj;
            cw[k] = ok ? A.cinfo[c] : 0xFFFFFFFFu;
            pv[k] = ok ? A.prop[c] : 0.0;
        }
        if (t < TT) L.a0[t] = (!WT && i0 + t < n) ? A.a0[i0 + t] : 0.0;
        const uint32_t out_col = (l32 == 0 ? 0x29u : 0u) | (l32 == TT - 1 ? 0x94u : 0u);      // in-edges that would come from another tile
        const bool edge_col = gj == 0 || gj == m - 1;
#pragma unroll
        for (int k = 0; k < NSET; k++) {
            const int r = 8 * k + r0, gi = i0 + r;
            const uint32_t w = cw[k];
            uint32_t word = FC_BLOCKED;
            if (w != 0xFFFFFFFFu) {
                ingrid |= 1u << k;
                const uint32_t outside = out_col | (r == 0 ? 0x07u : 0u) | (r == TT - 1 ? 0xE0u : 0u);
                const bool blocked = ((w & 0xFFu & outside) != 0u) || (w & (CI_PIT_IN | CI_PIT_OUT));
                word = ((w & CI_STATIC_MASK) << 16) | __popc(w & 0xFFu) | (blocked ? FC_BLOCKED : 0u);
                if (!WT && !blocked && (edge_col || gi == 0 || gi == n - 1) && A.todo_work[(int64_t)gi * m + gj] != 0) word |= FC_TODO;   // inlet cells of the tile's edge
            }
            L.cs[t + 256 * k] = word;
            L.slot[t + 256 * k].x = pv[k];
        }
    }
    lds_sync();
    int ph = 0;
    // ---- rounds.  A thread that counts a target down to zero goes on with that target itself ("chain": a river is
    // walked by one thread within one round instead of one cell per round); whatever else becomes ready waits for
    // its owner's next look
    for (;;) {
        uint32_t ready = 0;
#pragma unroll
        for (int k = 0; k < NSET; k++)
            if ((L.cs[t + 256 * k] & (FC_COUNT | FC_BLOCKED | FC_DONE)) == 0u) ready |= 1u << k;
        if (ready) s_any[ph] = 1;
        lds_sync();                                    // (also: every thread has read its words before anybody counts down)
        const bool go = s_any[ph] != 0;
        if (t == 0) s_any[ph ^ 1] = 0;
        ph ^= 1;
        if (!go) break;
        while (ready) {
            const int k = __ffs(ready) - 1; ready &= ready - 1u;
            int cur = t + 256 * k;
            do {
                const int r = cur >> 5, cl = cur & 31;
                const uint32_t word = L.cs[cur], w = word >> 16;
                const double pv = L.slot[cur].x;
                double a = WT ? A.a0[(int64_t)(i0 + r) * m + j0 + cl] : L.a0[r];
                bool td = (word & FC_TODO) != 0u;
                uint32_t mm = w & 0xFFu;
                while (mm) {                                        // ascending neighbour order, like the reference's pull
                    const int d = __ffs(mm) - 1; mm &= mm - 1u;
                    const int q = d + (d >> 2), di = (q * 11) >> 5;            // q = 0..8 with the centre skipped, di = q / 3
                    const double2 u = L.slot[cur + (di - 1) * TT + (q - 3 * di - 1)];
                    const double x = ((0x5A >> d) & 1) ? u.x : u.y;             // cardinal neighbours hand over their first share
                    if constexpr (WT) a += x;
                    else { a += fabs(x); td = td || (x < 0); }
                }
                double2 o = make_double2(0.0, 0.0);
                if (w & CI_OUT1) o.x = a * pv;
                if (w & CI_OUT2) o.y = a * (1 - pv);
                if (td) { o.x = -o.x; o.y = -o.y; }
                L.slot[cur] = o;
                L.cs[cur] = word | FC_DONE | (td ? FC_TODO : 0u);
                A.area[(int64_t)(i0 + r) * m + j0 + cl] = a;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");      // the shares are in place before a count can reach zero
                const int sct = ci_section(w);
                int next = -1;
                if (w & CI_OUT1) {
                    const int tr = r + fe1r(sct), tc = cl + fe1c(sct);
                    if (tr >= 0 && tr < TT && tc >= 0 && tc < TT &&
                        (atomicSub(&L.cs[tr * TT + tc], 1u) & (FC_COUNT | FC_BLOCKED)) == 1u) next = tr * TT + tc;
                }
                if (w & CI_OUT2) {
                    const int tr = r + fe2r(sct), tc = cl + fe2c(sct);
                    if (tr >= 0 && tr < TT && tc >= 0 && tc < TT &&
                        (atomicSub(&L.cs[tr * TT + tc], 1u) & (FC_COUNT | FC_BLOCKED)) == 1u && next < 0) next = tr * TT + tc;
                }
                cur = next;
            } while (cur >= 0);
        }
        lds_sync();
    }
    // ---- write the finished cells, row by row
    uint32_t done = 0;
#pragma unroll
    for (int k = 0; k < NSET; k++) {
        const uint32_t word = L.cs[t + 256 * k];
        if (!(word & FC_DONE)) continue;
        done |= 1u << k;
        const int64_t c = (int64_t)(i0 + 8 * k + r0) * m + gj;
        A.contrib[c] = L.slot[t + 256 * k];
        A.cinfo[c] = ci_with_level(word >> 16, 1u);
        if (word & FC_TODO) A.todo_work[c] = 1;
    }
    const int32_t finalized = __popc(done), n_cells = __popc(ingrid);
    if (finalized) atomicAdd(&s_fin[0], finalized);
    if (n_cells) atomicAdd(&s_fin[1], n_cells);
    __syncthreads();
    if (t == 0) {
        if (s_fin[0]) atomicAdd(n_final, s_fin[0]);
        if (s_fin[0] == s_fin[1]) tile_done[tid] = 1;
    }
}

#ifdef PYDEM_SWEEP_QUEUE
// switch from queue rounds to listed tile passes: the tiles that hold the current frontier
__global__ void k_tiles_of_frontier(const QE *__restrict__ q, const int32_t *nq, int m, int tiles_x, int32_t stamp, TileNext N)
{
    const int32_t n = *nq;
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const int32_t c = q[k].c;
        const int tt = (c / m / TH) * tiles_x + (c % m) / TT;
        if (atomicExch(&N.flag[tt], stamp) != stamp) N.list[atomicAdd(N.count, 1)] = tt;
    }
}

// after the tile passes: cells that are not final but whose upstream cells all are form the first
// queue frontier (level `r`)
__global__ __launch_bounds__(256) void k_sweep_rebuild_frontier(SweepArgs A, uint32_t r, QE *__restrict__ qn, int32_t *cn)
{
    __shared__ Stage S;
    if (threadIdx.x == 0) S.cnt = 0;
    __syncthreads();
    const int64_t NN = (int64_t)A.n * A.m;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < NN; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = base + threadIdx.x;
        bool push = false;
        uint32_t cw = 0;
        if (c < NN) {
            cw = A.cinfo[c];
            const uint32_t lv = ci_level(cw);
            if (lv == 0 || lv == CI_LEVEL_INF) {
                bool ready = true;
#pragma unroll
                for (int d = 0; d < 8; d++)
                    if (cw & (1u << d)) {
                        const uint32_t lu = ci_level(A.cinfo[c + NB_DI[d] * A.m + NB_DJ[d]]);
                        ready = ready && (lu >= 1 && lu < r);
                    }
                if (ready && (cw & CI_PIT_IN))
                    for (int32_t e = pit_stash(A, (int32_t)c).x; e < A.n_pit && A.pin_dst[e] == (int32_t)c; e++) {
                        const uint32_t lu = ci_level(A.cinfo[A.pin_src[e]]);
                        ready = ready && (lu >= 1 && lu < r);
                    }
                if (ready) { A.cinfo[c] = ci_with_level(cw, r); push = true; }
            }
        }
        stage_push(S, push, (int32_t)c, cw);
        stage_flush(A, S, qn, cn, false);
    }
    stage_flush(A, S, qn, cn, true);
}

#endif  // PYDEM_SWEEP_QUEUE

__global__ void k_row_area(const double *__restrict__ dX2, const double *__restrict__ dY2, int n, double *a0)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a0[i] = dX2[i] * dY2[i];                                          // :885
}

// ------------------------------------------------------------------------------- K5w
// Weighted sweep (pydem_uca_weighted): the same schedule from a per-cell seed.  _calc_uca_chunk starts its sweep from
// area = dX2 * dY2 per row (dem_processing.py:885, :901) and cyutils.pyx:163 is linear in it, so a weighted accumulation
// is that sweep started from w * dX2 * dY2 (or w).  The seed is formed once, in place in the weight plane: w[c] * a0[i]
// is what the plain sweep's a0[i] is for w = 1, so the two agree bit for bit there.
__global__ void k_weight_seed(const double *__restrict__ dX2, const double *__restrict__ dY2, int n, int m, double *__restrict__ w)
{
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const double a0 = dX2[i] * dY2[i];                                        // :885 (k_row_area)
        for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) w[(int64_t)i * m + j] *= a0;
    }
}

// the level field of every graph word as the graph stage leaves it (sources 0, every other cell "not yet known"): a
// sweep consumes the stamps, an edge round keeps its counts there
__global__ void k_sweep_rearm(uint32_t *__restrict__ cinfo, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t w = cinfo[c] & CI_STATIC_MASK;
        cinfo[c] = w | (((w & (0xFFu | CI_PIT_IN)) ? CI_LEVEL_INF : 0u) << CI_LEVEL_SHIFT);
    }
}

// :972 only (no edge masks: the weighted call leaves edge_todo / edge_done alone)
__global__ void k_uca_weighted_finalize(double *__restrict__ uca_w, const uint8_t *__restrict__ flats, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x)
        if (flats[c]) uca_w[c] = NAN;
}

// ------------------------------------------------------------------------------- K5c
// Circular drainage (rare: e.g. the overlap-1 patch of a tile's edge aspects can close a two-cell loop).  When the tile
// passes stall, the cells on and below the loop are unfinished; the reference then re-seeds its push sweep from the
// unfinished cells within 1 % of the highest unfinished elevation (dem_processing.py:951-964) and its Cython loop
// (cyutils.pyx:119-187) keeps going round by round -- pushing IN PLACE in ascending cell order, queueing a cell again
// whenever all its sources are done, skipping pushes into finished cells on the tile edge.  Those rules are order
// dependent, so the handful of unfinished cells is replayed here exactly like that by ONE thread (the oracle's
// oracle_uca_chunk / oracle_drain_area are the line-by-line model); everything else of the tile is already final.
struct ReseedCell { int32_t c; int32_t pin_first; int32_t pout_first; int32_t pad; };

// not finished by any pass: sources start with level 0, every other cell with "not yet known"
__device__ __forceinline__ bool ci_unfinished(uint32_t w) { const uint32_t lv = ci_level(w); return lv == 0 || lv == CI_LEVEL_INF; }

// area / taint an unfinished cell has received so far: the shares of its FINISHED upstream cells (graph word level >= 1)
// (WT: seed per cell, signed shares, no taint -- see sweep_one_tile)
template <bool WT = false>
__device__ void gather_finished(const SweepArgs &A, int32_t c, uint32_t cw, int32_t pin_first, double &a, bool &td)
{
    const int m = A.m, gi = c / m, gj = c - gi * m;
    a = WT ? A.a0[c] : A.a0[gi];
    td = !WT && (gi == 0 || gi == A.n - 1 || gj == 0 || gj == m - 1) && A.todo_work[c] != 0;
    for (int d = 0; d < 8; d++)
        if (cw & (1u << d)) {
            const int32_t u = c + NB_DI[d] * m + NB_DJ[d];
            if (ci_unfinished(A.cinfo[u])) continue;
            const bool cardinal = (NB_DI[d] == 0) || (NB_DJ[d] == 0);
            const double x = cardinal ? A.contrib[u].x : A.contrib[u].y;
            if constexpr (WT) a += x;
            else { a += fabs(x); td = td || (x < 0); }
        }
    if (cw & CI_PIT_IN)
        for (int32_t e = pin_first; e < A.n_pit && A.pin_dst[e] == c; e++) {
            const int32_t sc = A.pin_src[e];
            if (ci_unfinished(A.cinfo[sc])) continue;
            a += A.area[sc] * A.pin_w[e];
            if constexpr (!WT) td = td || (A.todo_work[sc] != 0);
        }
}

// the unfinished cells, in any order (the host sorts the few of them); their pit-list offsets are saved because the area
// slot that holds them is about to carry the area
__global__ __launch_bounds__(256) void k_reseed_collect(SweepArgs A, ReseedCell *__restrict__ list, int32_t *count, int32_t cap,
                                                        const double *__restrict__ elev, int32_t *nan_flag)
{
    const int64_t NN = (int64_t)A.n * A.m;
    for (int64_t c64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c64 < NN; c64 += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = (int32_t)c64;
        if (elev[c] != elev[c]) *nan_flag = 1;              // numpy's max over the tile propagates NaN (:963): then nothing is re-seeded
        const uint32_t w = A.cinfo[c];
        if (!ci_unfinished(w)) continue;
        int2 po = make_int2(0, 0);
        if (w & (CI_PIT_IN | CI_PIT_OUT)) po = pit_stash(A, c);
        const int32_t slot = atomicAdd(count, 1);
        if (slot < cap) { list[slot].c = c; list[slot].pin_first = po.x; list[slot].pout_first = po.y; list[slot].pad = 0; }
    }
}

__device__ __forceinline__ int reseed_find(const ReseedCell *U, int32_t nU, int32_t c)
{
    int lo = 0, hi = nU - 1;
    while (lo <= hi) { const int mid = (lo + hi) >> 1; if (U[mid].c == c) return mid; if (U[mid].c < c) lo = mid + 1; else hi = mid - 1; }
    return -1;
}

// ONE thread.  st[k]: bit 0 done, bit 1 in the current frontier, bit 2 in the previous frontier; tdf[k]: taint
template <bool WT = false>
__global__ void k_reseed_replay(SweepArgs A, const ReseedCell *__restrict__ U, int32_t nU, const double *__restrict__ elev,
                                const double *__restrict__ pit_w, uint8_t *__restrict__ st, uint8_t *__restrict__ tdf,
                                int tile_has_nan, int maxcount, uint32_t pass, int32_t *n_final, int32_t *n_done_out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int n = A.n, m = A.m;
    auto on_edge = [&](int32_t c) { const int i = c / m, j = c - i * m; return i == 0 || i == n - 1 || j == 0 || j == m - 1; };
    auto is_done = [&](int32_t c) -> bool {            // finished before the stall, or in the replay
        if (!ci_unfinished(A.cinfo[c])) return true;
        const int k = reseed_find(U, nU, c);
        return k >= 0 && (st[k] & 1u);
    };
    // what the unfinished cells have received so far
    for (int k = 0; k < nU; k++) {
        double a; bool td;
        gather_finished<WT>(A, U[k].c, A.cinfo[U[k].c] & CI_STATIC_MASK, U[k].pin_first, a, td);
        A.area[U[k].c] = a; tdf[k] = td; st[k] = 0;
    }
    int32_t n_done = 0, done_prev = -1;
    for (int count = 2; n_done < nU && count < maxcount && n_done != done_prev; count++) {     // :951-952 (the first drain was the tile passes)
        done_prev = n_done;
        // ---- the new frontier: ids[((data * ~done - max_elev) / max_elev > -0.01)] (:962-964); finished cells count as 0
        double mx = 0.0;
        for (int k = 0; k < nU; k++) if (!(st[k] & 1u) && elev[U[k].c] > mx) mx = elev[U[k].c];
        if (tile_has_nan) mx = NAN;
        for (int k = 0; k < nU; k++) {
            const double v = (st[k] & 1u) ? 0.0 : elev[U[k].c];
            st[k] = (uint8_t)((st[k] & 1u) | (((v - mx) / mx > -0.01) ? 2u : 0u));
        }
        // ---- cyutils._drain_area (:119-187)
        for (int64_t guard = 0; guard < 8 * (int64_t)nU + 64; guard++) {
            for (int k = 0; k < nU; k++) if (st[k] & 2u) { if (!(st[k] & 1u)) n_done++; st[k] |= 1u; }     // :138-140
            for (int k = 0; k < nU; k++) st[k] = (uint8_t)((st[k] & 1u) | ((st[k] & 2u) ? 4u : 0u));         // swap, zero the new frontier
            for (int k = 0; k < nU; k++) {
                if (!(st[k] & 4u)) continue;
                const int32_t i = U[k].c;
                const uint32_t cw = A.cinfo[i] & CI_STATIC_MASK;
                // the column of i: targets in ascending cell order (scipy sorts the indices of a CSC column)
                int32_t tg[2]; double fc[2]; int nt = 0;
                if (cw & (CI_OUT1 | CI_OUT2)) {
                    const int sct = ci_section(cw);
                    const double pv = A.prop[i];
                    if (cw & CI_OUT1) { tg[nt] = i + fe1r(sct) * m + fe1c(sct); fc[nt] = pv; nt++; }
                    if (cw & CI_OUT2) { tg[nt] = i + fe2r(sct) * m + fe2c(sct); fc[nt] = 1 - pv; nt++; }
                    if (nt == 2 && tg[1] < tg[0]) { const int32_t tt = tg[0]; tg[0] = tg[1]; tg[1] = tt; const double ff = fc[0]; fc[0] = fc[1]; fc[1] = ff; }
                }
                int32_t e = (cw & CI_PIT_OUT) ? U[k].pout_first : 0;
                for (int q = 0;; q++) {
                    int32_t row; double factor;
                    if (cw & CI_PIT_OUT) { if (!(e < A.n_pit && A.pit_src[e] == i)) break; row = A.pit_dst[e]; factor = pit_w[e]; e++; }
                    else { if (q >= nt) break; row = tg[q]; factor = fc[q]; }
                    const int kr = reseed_find(U, nU, row);
                    if (kr < 0) continue;                                   // (cannot happen: everything below an unfinished cell is unfinished)
                    if ((st[kr] & 1u) && on_edge(row)) continue;            // :159-161
                    A.area[row] += A.area[i] * factor;                      // :163
                    if (tdf[k]) tdf[kr] = 1;                                // edge_todo[row] += edge_todo[i] * factor (positive factors)
                    bool wait = false;                                      // :173-179
                    const uint32_t cwr = A.cinfo[row] & CI_STATIC_MASK;
                    for (int d = 0; d < 8 && !wait; d++)
                        if ((cwr & (1u << d)) && !is_done(row + NB_DI[d] * m + NB_DJ[d])) wait = true;
                    if (!wait && (cwr & CI_PIT_IN))
                        for (int32_t e2 = U[kr].pin_first; e2 < A.n_pit && A.pin_dst[e2] == row; e2++)
                            if (!is_done(A.pin_src[e2])) { wait = true; break; }
                    if (!wait) st[kr] |= 2u;
                }
            }
            bool changed = false;                                           // :187
            for (int k = 0; k < nU; k++) if (((st[k] >> 1) & 1u) != ((st[k] >> 2) & 1u)) changed = true;
            if (!changed) break;
        }
        for (int k = 0; k < nU; k++) st[k] &= 1u;                           // ids[:] = False (:962)
    }
    // finished cells join the others (level stamp, taint); the rest keep what they have received, like the reference
    for (int k = 0; k < nU; k++) {
        const int32_t c = U[k].c;
        if (tdf[k]) A.todo_work[c] = 1;
        if (st[k] & 1u) A.cinfo[c] = ci_with_level(A.cinfo[c], pass);
    }
    atomicAdd(n_final, n_done);
    *n_done_out = n_done;
}

// Host replay (more unfinished cells than the one-thread replay above is meant for): what the host needs of an unfinished
// cell -- its static graph word, elevation, proportion, pit-list offsets and what it has received from its finished
// upstream cells -- gathered in parallel; the results come back through k_reseed_scatter.
struct ReseedHost { int32_t c; uint32_t cw; int32_t pin_first, pout_first; double area, elev, prop; int32_t td, pad; };
template <bool WT = false>
__global__ __launch_bounds__(256) void k_reseed_gather(SweepArgs A, const ReseedCell *__restrict__ U, int32_t nU, const double *__restrict__ elev,
                                                       ReseedHost *__restrict__ out)
{
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nU; k += gridDim.x * blockDim.x) {
        ReseedHost h;
        h.c = U[k].c; h.cw = A.cinfo[h.c] & CI_STATIC_MASK; h.pin_first = U[k].pin_first; h.pout_first = U[k].pout_first;
        double a; bool td;
        gather_finished<WT>(A, h.c, h.cw, h.pin_first, a, td);
        h.area = a; h.td = td; h.pad = 0; h.elev = elev[h.c]; h.prop = (h.cw & (CI_OUT1 | CI_OUT2)) ? A.prop[h.c] : 0.0;
        out[k] = h;
    }
}
struct ReseedBack { int32_t c; int32_t flags; double area; };      // flags: bit 0 finished by the replay, bit 1 taint
__global__ __launch_bounds__(256) void k_reseed_scatter(SweepArgs A, const ReseedBack *__restrict__ B, int32_t nU, uint32_t pass)
{
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nU; k += gridDim.x * blockDim.x) {
        const int32_t c = B[k].c;
        A.area[c] = B[k].area;
        if (B[k].flags & 2) A.todo_work[c] = 1;
        if (B[k].flags & 1) A.cinfo[c] = ci_with_level(A.cinfo[c], pass);
    }
}

// finalisation of _calc_uca_chunk (:966-980): NaN on flats, edge_done = ~edge_todo etc.
// (16 cells per thread: the byte masks travel as 16-byte words; uca and elev are only touched where the masks ask for
// them -- flats, cells still on `todo` -- unless the saturation limit needs every value: 3 instead of 19 bytes per cell)
__device__ __forceinline__ bool finalize_cell(double *__restrict__ uca, const double *__restrict__ elev, int64_t c, uint32_t f, uint32_t td,
                                              int apply_limit, double limit)
{
    if (f) uca[c] = NAN;                                                         // :972
    bool dn = !td;                                                               // :974
    if (td && isnan(elev[c])) dn = true;                                         // :975
    if (apply_limit && !f && uca[c] > limit) dn = true;                          // :977-980 (NaN > limit is false)
    return dn;
}

__global__ __launch_bounds__(256) void k_uca_finalize(double *__restrict__ uca, const uint8_t *__restrict__ flats,
                                                      const uint8_t *__restrict__ todo_work, const double *__restrict__ elev,
                                                      uint8_t *__restrict__ edge_done, int64_t NN, int apply_limit, double limit)
{
    const int64_t nvec = NN >> 4, stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t v = t0; v < nvec; v += stride) {
        const uint4 f4 = reinterpret_cast<const uint4 *>(flats)[v], t4 = reinterpret_cast<const uint4 *>(todo_work)[v];
        const uint32_t fw[4] = {f4.x, f4.y, f4.z, f4.w}, tw[4] = {t4.x, t4.y, t4.z, t4.w};
        uint32_t dw[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t d = 0;
#pragma unroll
            for (int b = 0; b < 4; b++)
                d |= (finalize_cell(uca, elev, v * 16 + q * 4 + b, (fw[q] >> (8 * b)) & 0xFFu, (tw[q] >> (8 * b)) & 0xFFu, apply_limit, limit) ? 1u : 0u) << (8 * b);
            dw[q] = d;
        }
        reinterpret_cast<uint4 *>(edge_done)[v] = make_uint4(dw[0], dw[1], dw[2], dw[3]);
    }
    for (int64_t c = (nvec << 4) + t0; c < NN; c += stride)
        edge_done[c] = finalize_cell(uca, elev, c, flats[c], todo_work[c], apply_limit, limit);
}

// ------------------------------------------------------------------------------- K6
__global__ __launch_bounds__(256) void k_twi(const double *__restrict__ uca, const double *__restrict__ mag,
                                             double *__restrict__ twi, int64_t NN, double min_slope, int lim_uca,
                                             double uca_cap, int lim_twi, double twi_cap)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        double t = uca[c];
        if (lim_uca && t > uca_cap) t = uca_cap;                                 // :1663-1665
        t = log(t / (mag[c] + min_slope));                                       // :1667
        if (lim_twi && t > twi_cap) t = twi_cap;                                 // :1669-1672
        twi[c] = t;
    }
}

}  // namespace

int stage_section_graph(pydem_tile *t, const pydem_options *opt)
{
    const int n = (int)t->n, m = (int)t->m;
    t->graph_opt = *opt;
    t->edge_clean = false;
    t->einc_ready = false;
    PYDEM_TRY(tile_alloc(t, &t->todo_work, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->cinfo, (size_t)t->NN));          // the cinfo words
    const dim3 grid2((unsigned)(cdiv(m, 256) < 64 ? cdiv(m, 256) : 64), (unsigned)(n < 16384 ? n : 16384));
    t->tm.n_pit_edges = 0; t->tm.n_pits_undrained = 0; t->tm.pits_ms = 0;
    t->pits.n_edges = 0; t->pits.n_raw = 0;
    if (t->flats_state == 2) t->flats_state = 0;      // (state 2 is stated on the pit list that goes here; the pit search itself keeps
                                                      // state 1: it writes a mean of non-negative slopes and flats = 0 at the same cells)
    // The section / out-flag kernel and the in-mask kernel are streaming kernels that share nothing with the pit search
    // (bound by instruction issue, little memory traffic) except the flats mask: the reference derives section and
    // proportion from the mask as it is BEFORE the pits are patched (:1021-1070 runs ahead of _mk_adjacency_matrix).  A
    // snapshot of the mask (the todo_work bytes are idle until the in-mask kernel clears them) lets both kernels run on
    // the side stream while the main stream searches the pits and patches flats / mag.
    double *corner_sums = (double *)(t->counters + CS_WORK);                     // 12 doubles inside the counter block
    HIP_TRY(hipEventRecord(t->ev_fork, t->stream));
    HIP_TRY(hipStreamWaitEvent(t->stream2, t->ev_fork, 0));
    HIP_TRY(hipMemcpyAsync(t->todo_work, t->flats, (size_t)t->NN, hipMemcpyDeviceToDevice, t->stream2));
    HIP_TRY(hipEventRecord(t->ev_snap, t->stream2));
    HIP_TRY(hipStreamWaitEvent(t->stream, t->ev_snap, 0));                       // the pit search may patch flats from here on
    hipLaunchKernelGGL(k_section_proportion, grid2, dim3(256), 0, t->stream2, t->dir, (const uint8_t *)t->todo_work, t->sec_theta,
                       t->NN, n, m, t->elev, t->section, t->prop, t->cinfo);
    HIP_TRY(hipMemsetAsync(t->counters + CS_WORK, 0, CS_WORK_WORDS * sizeof(int32_t), t->stream2));
    HIP_TRY(hipMemsetAsync(t->edge_todo, 0, (size_t)t->NN, t->stream2));
    HIP_TRY(hipMemsetAsync(t->todo_work, 0, (size_t)t->NN, t->stream2));
    hipLaunchKernelGGL(k_graph_inmask, grid2, dim3(256), 0, t->stream2, t->prop, t->elev, n, m,
                       t->cinfo, t->edge_todo, t->todo_work, corner_sums);
    HIP_TRY(hipEventRecord(t->ev_join, t->stream2));
    static int graph_serial = -1;      // PYDEM_GRAPH_SERIAL=1 (measurements): the graph kernels before the pit search instead of beside it
    if (graph_serial < 0) { const char *e = getenv("PYDEM_GRAPH_SERIAL"); graph_serial = e ? atoi(e) : 0; }
    if (graph_serial) HIP_TRY(hipStreamWaitEvent(t->stream, t->ev_join, 0));
    HIP_TRY(hipEventRecord(t->ev[0], t->stream));
    if (opt->drain_pits) PYDEM_TRY(stage_pits(t, opt));
    HIP_TRY(hipEventRecord(t->ev[2], t->stream));
    HIP_TRY(hipStreamWaitEvent(t->stream, t->ev_join, 0));
    const bool stash = t->pit_stash_live && t->uca != nullptr;     // (pydem_uca asked for it: tile.hip)
    t->pit_stash_live = false;
    if (t->pits.n_edges > 0) {
        if (stash) {
            hipLaunchKernelGGL(k_graph_add_pits<true>, dim3(grid_for(t->pits.n_edges, 1024)), dim3(256), 0, t->stream, t->pits.src,
                               t->pits.dst, t->pits.w, t->pits.n_edges, n, m, t->cinfo, corner_sums, (const int32_t *)t->pits.in_dst, t->uca);
            t->pit_stash_live = true;
        } else {
            hipLaunchKernelGGL(k_graph_add_pits<false>, dim3(grid_for(t->pits.n_edges, 1024)), dim3(256), 0, t->stream, t->pits.src,
                               t->pits.dst, t->pits.w, t->pits.n_edges, n, m, t->cinfo, corner_sums, (const int32_t *)nullptr, (double *)nullptr);
        }
    }
    hipLaunchKernelGGL(k_corner_todo, dim3(1), dim3(64), 0, t->stream, corner_sums, t->elev, n, m, t->edge_todo, t->todo_work);
    HIP_TRY(hipEventRecord(t->ev[3], t->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventSynchronize(t->ev[3]));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, t->ev[0], t->ev[2]));      // the pit search, with both graph kernels beside it
    HIP_TRY(hipEventElapsedTime(&b, t->ev[2], t->ev[3]));      // what is left of them after it + pit flags + corners
    (void)a;
    t->tm.graph_ms = b;
    return 0;
}


// The re-seed loop of the reference (dem_processing.py:951-964 around cyutils._drain_area, cyutils.pyx:119-187) over the
// unfinished cells on the HOST: the same rules as k_reseed_replay, line by line, with the frontiers kept as sorted lists
// instead of flag scans (a round costs its frontier, not the whole list).  H is sorted by cell.  Pit lists: out-edges
// (src-sorted: pit_src / pit_dst / pit_w), in-edges (dst-sorted: pin_dst / pin_src).
static int64_t reseed_replay_host(std::vector<ReseedHost> &H, std::vector<uint8_t> &done, int n, int m, int maxcount, bool tile_has_nan,
                                  const std::vector<int32_t> &pit_src, const std::vector<int32_t> &pit_dst, const std::vector<double> &pit_w,
                                  const std::vector<int32_t> &pin_dst, const std::vector<int32_t> &pin_src)
{
    const int32_t nU = (int32_t)H.size();
    const int64_t n_pit = (int64_t)pit_src.size();
    static const int DI[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, DJ[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
    auto find = [&](int32_t c) -> int32_t {
        int32_t lo = 0, hi = nU - 1;
        while (lo <= hi) { const int32_t mid = (lo + hi) >> 1; if (H[(size_t)mid].c == c) return mid; if (H[(size_t)mid].c < c) lo = mid + 1; else hi = mid - 1; }
        return -1;
    };
    auto on_edge = [&](int32_t c) { const int i = c / m, j = c - i * m; return i == 0 || i == n - 1 || j == 0 || j == m - 1; };
    auto is_done = [&](int32_t c) -> bool { const int32_t k = find(c); return k < 0 || done[(size_t)k]; };   // not listed = finished by the passes
    done.assign((size_t)nU, 0);
    std::vector<uint8_t> in_cur((size_t)nU, 0);
    std::vector<int32_t> cur, prev;
    int64_t n_done = 0, done_prev = -1;
    for (int count = 2; n_done < nU && count < maxcount && n_done != done_prev; count++) {          // :951-952
        done_prev = n_done;
        double mx = 0.0;                                                                            // :962-964
        for (int32_t k = 0; k < nU; k++) if (!done[(size_t)k] && H[(size_t)k].elev > mx) mx = H[(size_t)k].elev;
        if (tile_has_nan) mx = NAN;
        cur.clear();
        for (int32_t k = 0; k < nU; k++) {
            const double v = done[(size_t)k] ? 0.0 : H[(size_t)k].elev;
            if ((v - mx) / mx > -0.01) cur.push_back(k);
        }
        for (int64_t guard = 0; guard < 8 * (int64_t)nU + 64; guard++) {
            for (int32_t k : cur) { if (!done[(size_t)k]) n_done++; done[(size_t)k] = 1; }          // cyutils.pyx:138-140
            prev.swap(cur); cur.clear();
            for (int32_t k : prev) {                                                                // ascending cell order
                const ReseedHost &S = H[(size_t)k];
                const int32_t i = S.c;
                int32_t tg[2]; double fc[2]; int nt = 0;
                if (S.cw & (CI_OUT1 | CI_OUT2)) {
                    const int sct = (int)((S.cw >> CI_SEC_SHIFT) & 7u);
                    if (S.cw & CI_OUT1) { tg[nt] = i + fe1r(sct) * m + fe1c(sct); fc[nt] = S.prop; nt++; }
                    if (S.cw & CI_OUT2) { tg[nt] = i + fe2r(sct) * m + fe2c(sct); fc[nt] = 1 - S.prop; nt++; }
                    if (nt == 2 && tg[1] < tg[0]) { std::swap(tg[0], tg[1]); std::swap(fc[0], fc[1]); }
                }
                int64_t e = (S.cw & CI_PIT_OUT) ? S.pout_first : 0;
                for (int q = 0;; q++) {
                    int32_t row; double factor;
                    if (S.cw & CI_PIT_OUT) { if (!(e < n_pit && pit_src[(size_t)e] == i)) break; row = pit_dst[(size_t)e]; factor = pit_w[(size_t)e]; e++; }
                    else { if (q >= nt) break; row = tg[q]; factor = fc[q]; }
                    const int32_t kr = find(row);
                    if (kr < 0) continue;
                    if (done[(size_t)kr] && on_edge(row)) continue;                                  // :159-161
                    H[(size_t)kr].area += S.area * factor;                                          // :163
                    if (S.td) H[(size_t)kr].td = 1;
                    bool wait = false;                                                              // :173-179
                    const uint32_t cwr = H[(size_t)kr].cw;
                    for (int d = 0; d < 8 && !wait; d++)
                        if ((cwr & (1u << d)) && !is_done(row + DI[d] * m + DJ[d])) wait = true;
                    if (!wait && (cwr & CI_PIT_IN))
                        for (int64_t e2 = H[(size_t)kr].pin_first; e2 < n_pit && pin_dst[(size_t)e2] == row; e2++)
                            if (!is_done(pin_src[(size_t)e2])) { wait = true; break; }
                    if (!wait && !in_cur[(size_t)kr]) { in_cur[(size_t)kr] = 1; cur.push_back(kr); }
                }
            }
            std::sort(cur.begin(), cur.end());
            for (int32_t k : cur) in_cur[(size_t)k] = 0;
            if (cur == prev) break;                                                                 // :187 (the frontier did not change)
        }
        cur.clear();
    }
    return n_done;
}

// The sweep schedule.  WT = false: pydem_uca's sweep into t->uca (fill_sweep_args).  WT = true: the weighted sweep of
// pydem_uca_weighted -- A.a0 = the per-cell seeds, A.area = t->uca_w, the same schedule (dense / LDS first-pass diagnostics
// and the queue schedule are not offered), NaN on flats only, no edge masks.
template <bool WT>
static int sweep_schedule(pydem_tile *t, const pydem_options *opt, double *seed)
{
    const int n = (int)t->n, m = (int)t->m;
    // (the tile visits address a tile + halo by 32-bit byte offsets from a scalar base: 34 rows of 16-byte entries)
    if (m >= (1 << 22)) { pydem_set_error("uca: tiles wider than 4 194 303 columns are not supported (this one has %d)", m); return -2; }
    PYDEM_TRY(tile_alloc(t, &t->queue[0], (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->queue[1], (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->row_area, (size_t)t->n));
    PYDEM_TRY(tile_alloc(t, &t->contrib, (size_t)t->NN * 2));
    t->circular_cells = 0;
    int32_t *total = t->counters + CS_PROCESSED;
#ifdef PYDEM_SWEEP_QUEUE
    int32_t *cnt3 = t->counters + CS_FRONTIER;
    int32_t *nsrc = t->counters + CS_SOURCES;
    int64_t done_prev = 0;
#endif
    HIP_TRY(hipEventRecord(t->ev[0], t->stream));
    HIP_TRY(hipMemsetAsync(t->counters, 0, CS_WINDOW * sizeof(int32_t), t->stream));
    if (!WT) hipLaunchKernelGGL(k_row_area, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, t->stream, t->dX2, t->dY2, n, t->row_area);
    SweepArgs A;
    fill_sweep_args(t, A);
    if (WT) { A.a0 = seed; A.area = t->uca_w; }
    const bool stashed = !WT && t->pit_stash_live;      // (the graph stage of this pydem_uca has done it in its walk over the pit edges)
    if (!WT) t->pit_stash_live = false;
    if (A.n_pit > 0 && !stashed)   // the unused area slots of pit sources / drains carry their edge-list offsets until they are processed
        hipLaunchKernelGGL(k_pit_stash, dim3(grid_for(A.n_pit, 2048)), dim3(256), 0, t->stream, A.pin_dst, A.pit_src, A.n_pit, A.area);
    // ---- tile-local passes until they stop paying, then the queue rounds take over
    const int tiles_x = (int)cdiv(m, TT), tiles_total = tiles_x * (int)cdiv(n, TH);
    // scratch: tile_done bytes | per-tile "listed for pass" stamps | two tile lists | open cells per tile
    const size_t tiles_pad = ((size_t)tiles_total + 255) & ~(size_t)255;
    const size_t scratch_need = tiles_pad * (1 + 4 + 4 + 4 + 4 + 4) + 64 * sizeof(int32_t);     // ... | block offsets of the symbolic tiles | K5f counters
    PYDEM_TRY(tile_reserve(t, &t->scratch, &t->scratch_bytes, scratch_need, scratch_need, false));
    uint8_t *tile_done = (uint8_t *)t->scratch;
    int32_t *tile_flag = (int32_t *)(tile_done + tiles_pad);
    int32_t *tile_list[2] = {tile_flag + tiles_pad, tile_flag + 2 * tiles_pad};
    int32_t *cntT = t->counters + CS_TILE_LIST;
    A.tile_open = tile_flag + 3 * tiles_pad;
    // K5f (two-level solve, uca_sym.inl): at the first look of the host that finds at most PYDEM_SWEEP_SYM tiles listed (0: never) ONE
    // symbolic visit per unfinished tile replaces the repeated numeric visits of the later passes.  The pool of coefficients lives in the
    // two queue buffers (idle in this schedule; the re-seed replay takes them over after k_sym_finish).
    static int64_t sym_switch = -1;
    if (sym_switch < 0) { const char *e = getenv("PYDEM_SWEEP_SYM"); sym_switch = e ? atoll(e) : 4096; if (sym_switch < 0) sym_switch = 0; }
    SymArgs Y;
    memset(&Y, 0, sizeof(Y));
    int32_t *symc = tile_flag + 4 * tiles_pad + tiles_pad;      // 64 counters: [0..15] pool regions, [16..23] / [24..31] work counters of the two launches, [32..] statistics
    const bool sym_on = sym_switch > 0 && TH == 32 && t->NN / 2 < ((int64_t)1 << 31);
    if (sym_on) {
        Y.pool0 = (double *)t->queue[0]; Y.pool1 = (double *)t->queue[1];
        Y.nreg = t->NN >= ((int64_t)1 << 22) ? 16 : 2;
        Y.reg_cap = (uint32_t)((t->NN / 2) / (Y.nreg / 2));
        Y.ctr = symc; Y.tile_sym = (uint32_t *)(tile_flag + 4 * tiles_pad); Y.stat = symc + 32;
        HIP_TRY(hipMemsetAsync(Y.tile_sym, 0xff, tiles_pad * 4, t->stream));
        HIP_TRY(hipMemsetAsync(symc, 0, 64 * sizeof(int32_t), t->stream));
    }
    HIP_TRY(hipMemsetAsync(tile_done, 0, tiles_pad * 5, t->stream));      // done bytes + stamps
    HIP_TRY(hipMemsetAsync(A.tile_open, 0x7f, tiles_pad * 4, t->stream));
    HIP_TRY(hipMemsetAsync(cntT, 0, 4 * sizeof(int32_t), t->stream));
    if (A.dbg & 4) HIP_TRY(hipMemsetAsync(t->counters + CS_TILE_PROF, 0, CS_TILE_PROF_WORDS * sizeof(int32_t), t->stream));
    int64_t launches = 0;
    uint32_t pass = 0;
    int32_t *work16 = t->counters + CS_WORK, *work3 = t->counters + CS_WORK;      // band counters of the two full passes / rotating counters of the listed ones
    HIP_TRY(hipMemsetAsync(work16, 0, 16 * sizeof(int32_t), t->stream));
    static int lds_pad = -1;        // occupancy experiments only: extra dynamic LDS per workgroup (PYDEM_TILE_LDS_PAD)
    if (lds_pad < 0) { const char *e = getenv("PYDEM_TILE_LDS_PAD"); lds_pad = e ? atoi(e) : 0; }
    // listed tile passes from pass p on (the list of pass p is in tile_list[p % 2] / cntT[p % 3]); returns the next pass number
    static int res_switch = -1;     // listed tiles at or below which the passes use resident visits (K5e)
    if (res_switch < 0) { const char *e = getenv("PYDEM_SWEEP_RESIDENT"); res_switch = e ? atoi(e) : 4096; }
    int64_t listed_left = 0;        // tiles listed for the pass run_listed returned (> 0 only when it stopped at `stop_at`)
    auto run_listed = [&](int p, int64_t ntiles, int64_t stop_at) -> int {
        TileNext N;
        N.flag = tile_flag;
        listed_left = ntiles;
        while (ntiles > stop_at) {
            static int dbg_each = -1;                        // PYDEM_SWEEP_DEBUG=2: a look (and a line) after every pass
            if (dbg_each < 0) { const char *e = getenv("PYDEM_SWEEP_DEBUG"); dbg_each = (e && atoi(e) >= 2) ? 1 : 0; }
            const int batch = dbg_each ? 1 : ntiles < 2048 ? 16 : 8;    // passes between two looks at the list size (a look idles the GPU for ~30 us; the grid only shrinks below 8192 listed tiles)
#ifndef PYDEM_LISTED_DYNAMIC
            const int grid = (int)(ntiles < 8192 ? (ntiles > 64 ? ntiles : 64) : 8192) * (4 / LWPB);
#else
            const int64_t want = cdiv(ntiles, 4);            // persistent wavefronts: no more workgroups than the chip holds at once
            const int grid = (int)(want < 256 * PYDEM_LISTED_OCC ? (want > 16 ? want : 16) : 256 * PYDEM_LISTED_OCC);
#endif
            const bool resident = ntiles <= res_switch;
            for (int b = 0; b < batch; b++, p++) {
                N.list = tile_list[(p + 1) % 2]; N.count = &cntT[(p + 1) % 3];
                if (resident)
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_tiles_resident<WT>), dim3((unsigned)(ntiles > 256 ? ntiles : 256)), dim3(64), 0, t->stream, A, (uint32_t)p, tiles_x,
                                       (const int32_t *)tile_list[p % 2], (const int32_t *)&cntT[p % 3], tile_done, total, N,
                                       &cntT[(p + 2) % 3], Y);
                else
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_tiles_listed<WT>), dim3(grid), dim3(64 * LWPB), (size_t)lds_pad, t->stream, A, (uint32_t)p, tiles_x,
                                       (const int32_t *)tile_list[p % 2], (const int32_t *)&cntT[p % 3], tile_done, total, N,
                                       &cntT[(p + 2) % 3], work3, Y);
                launches++;
            }
            if (hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream) != hipSuccess) return -1;
            if (hipStreamSynchronize(t->stream) != hipSuccess) return -1;
            ntiles = t->h_counters[CS_TILE_LIST + p % 3];
            listed_left = ntiles;
            if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "listed tile pass %d: %lld tiles listed next, processed %d (%d %s passes)\n", p, (long long)ntiles, t->h_counters[CS_PROCESSED], batch, resident ? "resident" : "generic");
            if (p > (int)CI_LEVEL_INF - 256) return -2;
        }
        return p;
    };
    // ---- circular drainage: replay of the reference's re-seed loop over the unfinished cells (K5c), after either schedule
    auto replay_unfinished = [&](uint32_t pass) -> int {
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        if ((int64_t)t->h_counters[CS_PROCESSED] >= t->NN) return 0;
        {
            // (the counter says how many cells the schedule processed; what is unfinished is decided by the level stamps:
            // the queue schedule does not count every cell it settles)
            ReseedCell *U = (ReseedCell *)t->queue[0];                       // scratch: the queue buffers are idle by now
            const int64_t cap64 = std::min<int64_t>(t->NN * 4 / (int64_t)sizeof(ReseedCell), (int64_t)1 << 22);
            uint8_t *stf = (uint8_t *)t->queue[1];                           // state bytes, then taint bytes
            int32_t *rc = t->counters + CS_RESEED;                           // [0] collected, [1] NaN flag, [2] finished by the replay
            HIP_TRY(hipMemsetAsync(rc, 0, 3 * sizeof(int32_t), t->stream));
            hipLaunchKernelGGL(k_reseed_collect, dim3(grid_for(t->NN, 4096)), dim3(256), 0, t->stream, A, U, rc, (int32_t)cap64,
                               (const double *)t->elev, rc + 1);
            HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipStreamSynchronize(t->stream));
            const int64_t unfinished = (int64_t)t->h_counters[CS_RESEED];
            if (unfinished == 0) {
                // every cell carries a level stamp although the schedule did not process all of them: seen with the queue
                // schedule on tiles with circular drainage (a queued cell of a loop is never processed).  Not silently.
                pydem_set_error("sweep: %lld cells were scheduled but never processed (PYDEM_SWEEP_MODE=queue does not support this tile's "
                                "circular drainage; use the default schedule)", (long long)(t->NN - (int64_t)t->h_counters[CS_PROCESSED]));
                return -5;
            }
            t->circular_cells = unfinished;
            static int64_t host_above = -1;        // PYDEM_RESEED_HOST_ABOVE (tests): unfinished cells above which the host replays
            if (host_above < 0) { const char *e = getenv("PYDEM_RESEED_HOST_ABOVE"); host_above = e ? atoll(e) : ((int64_t)1 << 22); }
            if (unfinished > cap64 || unfinished > host_above) {
                // more cells than the one-thread replay is meant for (a loop at the head of a long river): the reference finishes
                // such a tile, slowly (:951-964) -- so does the host here, with a note on stderr
                fprintf(stderr, "pydem: circular drainage with %lld unfinished cells: the re-seed loop runs on the host\n", (long long)unfinished);
                if (unfinished > INT32_MAX / 2) { pydem_set_error("circular drainage: %lld unfinished cells", (long long)unfinished); return -5; }
                const int32_t nU = (int32_t)unfinished;
                DevTemp d_tmp;
                PYDEM_TRY(d_tmp.alloc((size_t)nU * (sizeof(ReseedCell) + sizeof(ReseedHost))));
                ReseedCell *U2 = d_tmp.as<ReseedCell>();
                ReseedHost *dH = (ReseedHost *)(d_tmp.as<char>() + (size_t)nU * sizeof(ReseedCell));
                HIP_TRY(hipMemsetAsync(rc, 0, 3 * sizeof(int32_t), t->stream));
                hipLaunchKernelGGL(k_reseed_collect, dim3(grid_for(t->NN, 4096)), dim3(256), 0, t->stream, A, U2, rc, nU, (const double *)t->elev, rc + 1);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reseed_gather<WT>), dim3(grid_for(nU, 1024)), dim3(256), 0, t->stream, A, (const ReseedCell *)U2, nU, (const double *)t->elev, dH);
                std::vector<ReseedHost> H((size_t)nU);
                HIP_TRY(hipMemcpyAsync(H.data(), dH, (size_t)nU * sizeof(ReseedHost), hipMemcpyDeviceToHost, t->stream));
                HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
                HIP_TRY(hipStreamSynchronize(t->stream));
                const bool has_nan = t->h_counters[CS_RESEED + 1] != 0;
                std::sort(H.begin(), H.end(), [](const ReseedHost &a, const ReseedHost &b) { return a.c < b.c; });
                const size_t np = (size_t)A.n_pit;
                std::vector<int32_t> h_ps(np), h_pd(np), h_is(np), h_id(np); std::vector<double> h_pw(np);
                if (np) {
                    HIP_TRY(hipMemcpy(h_ps.data(), A.pit_src, np * 4, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(h_pd.data(), A.pit_dst, np * 4, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(h_pw.data(), t->pits.w, np * 8, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(h_id.data(), A.pin_dst, np * 4, hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(h_is.data(), A.pin_src, np * 4, hipMemcpyDeviceToHost));
                }
                std::vector<uint8_t> dn;
                const int64_t n_done = reseed_replay_host(H, dn, n, m, (int)opt->circular_ref_maxcount, has_nan, h_ps, h_pd, h_pw, h_id, h_is);
                std::vector<ReseedBack> back((size_t)nU);
                for (int32_t k = 0; k < nU; k++) { back[(size_t)k].c = H[(size_t)k].c; back[(size_t)k].area = H[(size_t)k].area; back[(size_t)k].flags = (dn[(size_t)k] ? 1 : 0) | (H[(size_t)k].td ? 2 : 0); }
                static_assert(sizeof(ReseedBack) <= sizeof(ReseedHost), "the gather buffer is reused for the results");
                HIP_TRY(hipMemcpy(dH, back.data(), (size_t)nU * sizeof(ReseedBack), hipMemcpyHostToDevice));
                hipLaunchKernelGGL(k_reseed_scatter, dim3(grid_for(nU, 1024)), dim3(256), 0, t->stream, A, (const ReseedBack *)dH, nU, pass);
                HIP_TRY(hipStreamSynchronize(t->stream));
                t->h_counters[CS_PROCESSED] += (int32_t)n_done;
                HIP_TRY(hipMemcpy(t->counters + CS_PROCESSED, t->h_counters + CS_PROCESSED, sizeof(int32_t), hipMemcpyHostToDevice));
                if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "circular drainage: %lld unfinished cells, %lld finished by the re-seed replay on the host\n", (long long)unfinished, (long long)n_done);
                return 0;
            }
            std::vector<ReseedCell> hu((size_t)unfinished);
            HIP_TRY(hipMemcpyAsync(hu.data(), U, hu.size() * sizeof(ReseedCell), hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipStreamSynchronize(t->stream));
            std::sort(hu.begin(), hu.end(), [](const ReseedCell &a, const ReseedCell &b) { return a.c < b.c; });
            HIP_TRY(hipMemcpyAsync(U, hu.data(), hu.size() * sizeof(ReseedCell), hipMemcpyHostToDevice, t->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reseed_replay<WT>), dim3(1), dim3(64), 0, t->stream, A, (const ReseedCell *)U, (int32_t)unfinished,
                               (const double *)t->elev, (const double *)t->pits.w, stf, stf + unfinished, t->h_counters[CS_RESEED + 1],
                               (int)opt->circular_ref_maxcount, pass, total, rc + 2);
            launches += 2;
            HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipStreamSynchronize(t->stream));
            if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "circular drainage: %lld unfinished cells, %d finished by the re-seed replay\n", (long long)unfinished, t->h_counters[CS_RESEED + 2]);
        }
        return 0;
    };
    // 0: tile passes only (the product schedule), 1: tile pass + queue rounds + listed tail.  The queue schedule refuses
    // some valid inputs (circular drainage it cannot finish, frontiers above NN/2 entries): it only exists in builds with
    // -DPYDEM_SWEEP_QUEUE, a product build ignores PYDEM_SWEEP_MODE
#ifdef PYDEM_SWEEP_QUEUE
    static int sweep_mode = -1;
    if (sweep_mode < 0) { const char *e = getenv("PYDEM_SWEEP_MODE"); sweep_mode = (e && !strcmp(e, "queue")) ? 1 : 0; }
    if (WT && sweep_mode == 1) { pydem_set_error("pydem_uca_weighted: PYDEM_SWEEP_MODE=queue is not supported (the weighted sweep runs the tile passes)"); return -6; }
#else
    constexpr int sweep_mode = 0;
#endif
#ifdef PYDEM_SWEEP_STATIC
    const unsigned full_grid = (unsigned)(((tiles_total + 31) / 32) * 8);
#else
    const unsigned full_grid = (unsigned)std::min<int64_t>(((tiles_total + 31) / 32) * 8, 256 * (32 / FWPB));    // persistent: 32 wavefronts per CU
#endif

    if (sweep_mode == 0) {
        // pass 1 over every tile, pass 2 over every tile that is not done (it also lists the tiles of pass 3),
        // then only the listed tiles until no tile is listed any more
        // PYDEM_SWEEP_FIRST=lds: pass 1 by the LDS-resident kernel (K5a).  Measured at 16384^2: 9.9 ms against 7.8 ms of the
        // generic kernel (eight 20-KB tiles per CU instead of 32 bookkeeping-only ones: the dependency depth of a tile times
        // the LDS latency per cell is not hidden any more), and pass 2 inherits the cells with pit edges -- not the default
        static int first_kind = -1;
        if (first_kind < 0) { const char *e = getenv("PYDEM_SWEEP_FIRST"); first_kind = (e && !strcmp(e, "lds")) ? 1 : 0; }
        // PYDEM_SWEEP_DENSE=k: k dense level kernels (K5d) first; the tile passes then start at pass k + 1.  Measured, not
        // the default (profiles/r04_sweep_passes_dense*.txt)
        static int dense_levels = -1;
        if (dense_levels < 0) { const char *e = getenv("PYDEM_SWEEP_DENSE"); dense_levels = e ? atoi(e) : 0; if (dense_levels < 0) dense_levels = 0; }
        for (int lv = 1; lv <= dense_levels; lv++) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_dense_level<WT>), dim3((unsigned)cdiv(m, 256), (unsigned)cdiv(n, DENSE_BAND)), dim3(256), 0, t->stream,
                               A, (uint32_t)lv, total);
            launches++;
        }
        const uint32_t pb = (uint32_t)dense_levels;       // passes so far
        if (first_kind == 1 && TH == 32 && pb == 0)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_first<WT>), dim3((unsigned)(((tiles_total + 7) / 8) * 8)), dim3(256), 0, t->stream, A, tiles_x, tiles_total, tile_done, total);
        else {
            TileNext N0; N0.flag = nullptr; N0.list = nullptr; N0.count = nullptr;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_tiles<false, WT>), dim3(full_grid), dim3(64 * FWPB), (size_t)lds_pad, t->stream, A, pb + 1u, tiles_x, tiles_total, tile_done, total, N0, work16);
        }
        TileNext N; N.flag = tile_flag; N.list = tile_list[(pb + 3) % 2]; N.count = &cntT[(pb + 3) % 3];
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_tiles<true, WT>), dim3(full_grid), dim3(64 * FWPB), (size_t)lds_pad, t->stream, A, pb + 2u, tiles_x, tiles_total, tile_done, total, N, work16 + 8);
        HIP_TRY(hipMemsetAsync(work3, 0, CS_WORK_WORDS * sizeof(int32_t), t->stream));       // (the listed passes reuse the band counters' words: 3 x 8, rotating)
        launches += 2;
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "tile passes %u-%u: %d cells of %lld, %d tiles listed\n", pb + 1, pb + 2, t->h_counters[CS_PROCESSED], (long long)t->NN, t->h_counters[CS_TILE_LIST + (pb + 3) % 3]);
        int p_end = run_listed((int)pb + 3, t->h_counters[CS_TILE_LIST + (pb + 3) % 3], sym_on ? sym_switch : 0);
        if (sym_on && p_end > 0 && listed_left > 0) {
            // pass p_end = the symbolic visit of every tile that is not done (K5f (a)): a superset of the tiles listed for it
            const uint32_t ps = (uint32_t)p_end;
            TileNext N3; N3.flag = tile_flag; N3.list = tile_list[(ps + 1) % 2]; N3.count = &cntT[(ps + 1) % 3];
            HIP_TRY(hipMemsetAsync(&cntT[(ps + 2) % 3], 0, sizeof(int32_t), t->stream));      // (a numeric pass clears the count of the list after the next one)
            int32_t *cand = tile_list[ps % 2];      // (the list of this pass is not used: the candidates take its place)
            hipLaunchKernelGGL(k_sym_candidates, dim3((unsigned)cdiv(tiles_total, 256)), dim3(256), 0, t->stream, (const uint8_t *)tile_done, (const int32_t *)A.tile_open,
                               tiles_total, 256, cand, symc + 16);
            // the three size classes side by side (each kernel lasts as long as its longest visits: 0.7 + 0.4 + 0.4 ms one after the other)
            HIP_TRY(hipEventRecord(t->ev_fork, t->stream));
            HIP_TRY(hipStreamWaitEvent(t->stream2, t->ev_fork, 0));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_sym<256, WT>), dim3(256 * 32), dim3(64), 0, t->stream, A, Y, ps, tiles_x, tiles_total, tile_done, total, N3, (const int32_t *)cand, (const int32_t *)(symc + 16), 0, 0);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sweep_sym<1024, WT>), dim3(256 * 16), dim3(64), 0, t->stream2, A, Y, ps, tiles_x, tiles_total, tile_done, total, N3, (const int32_t *)cand, (const int32_t *)(symc + 17), 1, 256);
            HIP_TRY(hipEventRecord(t->ev_join, t->stream2));
            HIP_TRY(hipStreamWaitEvent(t->stream, t->ev_join, 0));
            launches += 4;
            HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipStreamSynchronize(t->stream));
            if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "symbolic pass %u: %d cells of %lld, %d tiles listed\n", ps, t->h_counters[CS_PROCESSED], (long long)t->NN, t->h_counters[CS_TILE_LIST + (ps + 1) % 3]);
            p_end = run_listed((int)ps + 1, t->h_counters[CS_TILE_LIST + (ps + 1) % 3], 0);
        }
        if (p_end == -1) { pydem_set_error("HIP error in the listed tile passes"); return -4; }
        if (p_end == -2) { pydem_set_error("flow paths longer than %u passes are not supported", CI_LEVEL_INF); return -5; }
        pass = (uint32_t)p_end;
        t->tm.sweep_tile_passes = (int64_t)pass;
        if (sym_on) {
            // K5f (c): the cells that still carry a symbolic header
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sym_finish<WT>), dim3((unsigned)std::min<int64_t>(tiles_total, 256 * 16)), dim3(64), 0, t->stream, A, Y, pass, tiles_x, tiles_total, total);
            launches++;
            if (getenv("PYDEM_SWEEP_DEBUG")) {
                int32_t hs[64];
                HIP_TRY(hipMemcpyAsync(hs, symc, sizeof(hs), hipMemcpyDeviceToHost, t->stream));
                HIP_TRY(hipStreamSynchronize(t->stream));
                int64_t used = 0;
                for (int r = 0; r < Y.nreg; r++) used += hs[r];
                fprintf(stderr, "two-level solve: %d symbolic tiles (%d fell back to numeric visits), %d outlets, %d symbolic cells, pool %lld of %lld doubles\n",
                        hs[32], hs[33], hs[34], hs[35], (long long)used, (long long)Y.reg_cap * Y.nreg);
#ifdef PYDEM_SYM_PROF
                {
                    const unsigned long long *acc = (const unsigned long long *)(hs + 40);
                    const double v = acc[8] ? (double)acc[8] : 1.0;
                    fprintf(stderr, "symbolic visits: %llu, %.1f open cells, %.1f rounds, %.1f pool entries each; us per visit: stage %.1f, inlets %.1f, set-up %.1f, constants %.1f, "
                            "rounds %.1f (%.2f us per round), end %.1f\n", acc[8], acc[9] / v, acc[6] / v, acc[7] / v, acc[0] / v / 100, acc[1] / v / 100, acc[2] / v / 100,
                            acc[3] / v / 100, acc[4] / v / 100, acc[6] ? acc[4] / 100.0 / (double)acc[6] : 0.0, acc[5] / v / 100);
                }
#endif
            }
        }
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        PYDEM_TRY(replay_unfinished(pass));
        if (A.dbg & 4) {
            const unsigned long long *acc = (const unsigned long long *)(t->h_counters + CS_TILE_PROF);
            fprintf(stderr, "tile phases (10 ns ticks summed over %llu tile runs, %llu of them finished nothing): stage %llu, setup %llu, rounds %llu (%llu rounds), stamp %llu\n",
                    acc[5], acc[6], acc[0], acc[1], acc[2], acc[4], acc[3]);
        }
    }
#ifdef PYDEM_SWEEP_QUEUE
    if (sweep_mode == 1) {
    // every pass re-stages all tiles that still have an open cell (rivers cross most tiles), so after the
    // first pass (which finishes ~3/4 of the grid) the queue rounds are cheaper than another pass
    static int max_passes = -1;
    if (max_passes < 0) { const char *e = getenv("PYDEM_TILE_PASSES"); max_passes = e ? atoi(e) : 1; if (max_passes < 1) max_passes = 1; }
    for (;;) {
        pass++;
        { TileNext N0; N0.flag = nullptr; N0.list = nullptr; N0.count = nullptr;
          HIP_TRY(hipMemsetAsync(work16, 0, 16 * sizeof(int32_t), t->stream));
          hipLaunchKernelGGL(k_sweep_tiles<false>, dim3(full_grid), dim3(256), 0, t->stream, A, pass, tiles_x, tiles_total, tile_done, total, N0, work16); }
        launches++;
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        const int64_t done_now = t->h_counters[CS_PROCESSED];
        const int64_t gained = done_now - done_prev;
        if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "tile pass %u: +%lld cells (%.2f%%), total %.2f%%\n", pass, (long long)gained, 100.0 * gained / t->NN, 100.0 * done_now / t->NN);
        done_prev = done_now;
        // a pass costs about one streaming read of the unfinished tiles; stop when it finishes < 1.5 % of the grid
        if (done_now >= t->NN || gained * 64 < t->NN || (int)pass >= max_passes) break;
    }
    t->tm.sweep_tile_passes = (int64_t)pass;
    int r = (int)pass + 1;
    int64_t last = 0;
    if (done_prev < t->NN) {
        hipLaunchKernelGGL(k_sweep_rebuild_frontier, dim3(grid_for(t->NN, 4096)), dim3(256), 0, t->stream, A, (uint32_t)r,
                           (QE *)t->queue[r % 2], &cnt3[r % 3]);
        launches++;
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        last = t->h_counters[CS_FRONTIER + r % 3];
        if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "after rebuild: frontier %lld, processed %d of %lld\n", (long long)last, t->h_counters[CS_PROCESSED], (long long)t->NN);
    }
    (void)nsrc;
    static int small_cap = -1, tile_switch = -1;
    if (small_cap < 0) { const char *e = getenv("PYDEM_SWEEP_SMALL"); small_cap = e ? atoi(e) : SWEEP_SMALL_CAP; }
    if (tile_switch < 0) { const char *e = getenv("PYDEM_SWEEP_TILE_SWITCH"); tile_switch = e ? atoi(e) : 20000; }
    while (last > 0) {
        if (last <= tile_switch) {
            // ---- the rivers: listed tile passes.  A queue round moves every river by ONE cell per kernel
            // boundary; a listed pass moves it through a whole tile (the on-chip rounds) for the same boundary.
            int p = r;
            TileNext N;
            N.flag = tile_flag; N.list = tile_list[p % 2]; N.count = &cntT[p % 3];
            hipLaunchKernelGGL(k_tiles_of_frontier, dim3(grid_for(last, 256)), dim3(256), 0, t->stream, (const QE *)t->queue[r % 2],
                               (const int32_t *)&cnt3[r % 3], m, tiles_x, (int32_t)p, N);
            launches++;
            int64_t ntiles = last;      // upper bound for the first batch
            while (ntiles > 0) {
                const int batch = 8;
                const int grid = (int)(ntiles * 2 < 2048 ? (ntiles * 2 > 64 ? ntiles * 2 : 64) : 2048);
                for (int b = 0; b < batch; b++, p++) {
                    N.list = tile_list[(p + 1) % 2]; N.count = &cntT[(p + 1) % 3];
                    hipLaunchKernelGGL(k_sweep_tiles_listed, dim3(grid), dim3(64 * LWPB), 0, t->stream, A, (uint32_t)p, tiles_x,
                                       (const int32_t *)tile_list[p % 2], (const int32_t *)&cntT[p % 3], tile_done, total, N,
                                       &cntT[(p + 2) % 3], work3, Y);
                    launches++;
                }
                HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_END * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
                HIP_TRY(hipStreamSynchronize(t->stream));
                ntiles = t->h_counters[CS_TILE_LIST + p % 3];
                if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "listed tile pass %d: %lld tiles listed next, processed %d\n", p, (long long)ntiles, t->h_counters[CS_PROCESSED]);
                if (p > (int)CI_LEVEL_INF - 256) { pydem_set_error("flow paths longer than %u passes are not supported", CI_LEVEL_INF); return -5; }
            }
            t->tm.sweep_tile_passes += p - r;
            r = p;
            last = 0;
            break;
        }
        if (last <= small_cap && last <= SWEEP_SMALL_CAP) {
            // one workgroup, many rounds (until the frontier is empty or grows past SWEEP_SMALL_CAP)
            hipLaunchKernelGGL(k_sweep_small, dim3(1), dim3(1024), 0, t->stream, A, (QE *)t->queue[0], (QE *)t->queue[1], cnt3, r,
                               (int)CI_LEVEL_INF - 256, total, t->counters + CS_SWEEP_STATE);
            launches++;
            HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipStreamSynchronize(t->stream));
            const int r_new = t->h_counters[CS_SWEEP_STATE];
            if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "single-workgroup rounds %d..%d, frontier now %d\n", r, r_new, t->h_counters[CS_FRONTIER + r_new % 3]);
            if (r_new == r) { pydem_set_error("sweep made no progress at round %d", r); return -5; }
            r = r_new;
            last = t->h_counters[CS_FRONTIER + r % 3];
            if (r >= (int)CI_LEVEL_INF - 256) { pydem_set_error("flow paths longer than %u rounds are not supported", CI_LEVEL_INF); return -5; }
            continue;
        }
        const int batch = last > 262144 ? 2 : (last > 4096 ? 8 : 64);
        const int grid = grid_for(last, 2048);
        const bool lowlat = last <= 262144;       // latency-bound rounds: speculative batched loads
        for (int b = 0; b < batch; b++, r++) {
            if (lowlat)
                hipLaunchKernelGGL(k_sweep_round<true>, dim3(grid), dim3(256), 0, t->stream, A, (const QE *)t->queue[r % 2],
                                   (QE *)t->queue[(r + 1) % 2], cnt3, r, total);
            else
                hipLaunchKernelGGL(k_sweep_round<false>, dim3(grid), dim3(256), 0, t->stream, A, (const QE *)t->queue[r % 2],
                                   (QE *)t->queue[(r + 1) % 2], cnt3, r, total);
            launches++;
        }
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        last = t->h_counters[CS_FRONTIER + r % 3];
        if (getenv("PYDEM_SWEEP_DEBUG")) fprintf(stderr, "round %d: frontier %lld, processed %d\n", r, (long long)last, t->h_counters[CS_PROCESSED]);
        if (r > (int)CI_LEVEL_INF - 256) { pydem_set_error("flow paths longer than %u rounds are not supported", CI_LEVEL_INF); return -5; }
    }
        PYDEM_TRY(replay_unfinished((uint32_t)r));
    }   // sweep_mode == 1
#endif  // PYDEM_SWEEP_QUEUE
    if (t->h_counters[CS_QUEUE_ERR] > 0) { pydem_set_error("sweep frontier exceeded the queue capacity (%lld entries)", (long long)A.qcap); return -5; }
    const int64_t processed = (int64_t)t->h_counters[CS_PROCESSED];     // tile passes + queue rounds ([4], [10]: tile-pass statistics)
    t->tm.n_unresolved = t->NN - processed;
    t->tm.sweep_kernel_launches = launches;
    if (WT) {
        hipLaunchKernelGGL(k_uca_weighted_finalize, dim3(grid_for(t->NN, 8192)), dim3(256), 0, t->stream, t->uca_w, (const uint8_t *)t->flats, t->NN);
    } else {
        double min_area = INFINITY;
        for (int64_t i = 0; i < t->n; i++) { const double a = t->h_dX2[(size_t)i] * t->h_dY2[(size_t)i]; if (a < min_area) min_area = a; }
        hipLaunchKernelGGL(k_uca_finalize, dim3(grid_for(t->NN, 8192)), dim3(256), 0, t->stream, t->uca, t->flats, t->todo_work,
                           t->elev, t->edge_done, t->NN, opt->apply_uca_limit_edges, opt->uca_saturation_limit * 2 * min_area);
    }
    HIP_TRY(hipEventRecord(t->ev[1], t->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventSynchronize(t->ev[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, t->ev[0], t->ev[1]));
    t->tm.sweep_ms = ms;
    t->tm.sweep_rounds = t->h_counters[CS_ROUNDS];
    return 0;
}

int stage_sweep(pydem_tile *t, const pydem_options *opt) { return sweep_schedule<false>(t, opt, nullptr); }

// pydem_uca_weighted on the tile's flow graph: the seed in place in the weight plane, the level stamps re-armed, the weighted
// schedule.  The sweep's work state -- level stamps, contribution records, queue buffers, scratch -- is shared with the plain
// path; every timing and counter of the plain path is put back, and the next edge round rebuilds its state (edge_clean).
int stage_uca_weighted(pydem_tile *t, const pydem_options *opt, int scale_by_cell_area)
{
    const int n = (int)t->n, m = (int)t->m;
    HIP_TRY(hipEventRecord(t->ev[2], t->stream));
    t->edge_clean = false;              // the level fields and the contribution records carried the classic rounds' state
    if (scale_by_cell_area) {
        const dim3 grid2((unsigned)(cdiv(m, 256) < 64 ? cdiv(m, 256) : 64), (unsigned)(n < 16384 ? n : 16384));
        hipLaunchKernelGGL(k_weight_seed, grid2, dim3(256), 0, t->stream, (const double *)t->dX2, (const double *)t->dY2, n, m, t->weight);
    }
    hipLaunchKernelGGL(k_sweep_rearm, dim3(grid_for(t->NN, 8192)), dim3(256), 0, t->stream, t->cinfo, t->NN);
    HIP_TRY(hipGetLastError());
    const pydem_timings keep = t->tm;
    const int64_t keep_circular = t->circular_cells;
    const int rc = sweep_schedule<true>(t, opt, t->weight);
    float ms = 0;
    if (rc == 0) HIP_TRY(hipEventElapsedTime(&ms, t->ev[2], t->ev[1]));      // seed + re-arm + schedule (ev[1]: end of the schedule, synchronised)
    t->tm = keep;
    t->circular_cells = keep_circular;
    if (rc == 0) t->tm.uca_weighted_ms = ms;
    return rc;
}

int stage_twi(pydem_tile *t, const pydem_options *opt)
{
    HIP_TRY(hipEventRecord(t->ev[0], t->stream));
    const double uca_cap = opt->uca_saturation_limit * opt->twi_min_area;
    const double twi_cap = log(opt->uca_saturation_limit * opt->twi_min_area / opt->twi_min_slope);
    hipLaunchKernelGGL(k_twi, dim3(grid_for(t->NN, 8192)), dim3(256), 0, t->stream, t->uca, t->mag, t->twi, t->NN,
                       opt->twi_min_slope, opt->apply_twi_limits_on_uca, uca_cap, opt->apply_twi_limits, twi_cap);
    HIP_TRY(hipEventRecord(t->ev[1], t->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventSynchronize(t->ev[1]));
    float a = 0;
    HIP_TRY(hipEventElapsedTime(&a, t->ev[0], t->ev[1]));
    t->tm.twi_ms = a;
    return 0;
}

