// flowacc_fwd.hip -- K11: forward accumulation with a per-cell rule on the tile's D-infinity flow graph (TauDEM's DinfDecayAccum
// and DinfTransLimAccum; no counterpart in the reference; semantics: include/pydem_hip.h, pydem_fwd_accum): a load that is
// multiplied on its way out of every cell and capped on its way into every cell, swept from the divides to the outlets like the
// upslope distance of flowdist_up.hip.
//
//     acc = 0; acc += w_e * (mult[u_e] * V[u_e]);  I[c] = acc;  tot = load[c] + acc;  V[c] = min(tot, cap[c])
//
// over the in-edges e = u_e -> c in the order of dd_for_in_edges (without mult: w_e * V[u_e]; without cap: V = tot; a NaN stays
// NaN through the cap).  A cell is open until every cell with an edge into it is final; then ONE lane finishes it by pulling
// their final values: no floating-point atomics, and a value does not depend on the schedule that produced it.  The sweep's own
// parts are the recursion, the value of a cell nothing flows into and the rounds of a tile visit; everything else -- state,
// encoding, counters, switches, the visit frame, the init and level kernels, the in-edge walk, the start set and the queue of a
// forward sweep (UpClassify, k_du_recount, du_release), the host's schedule -- is the engine's (flowdist.h).  The load is the
// seed plane of pydem_rev_accum; mult, cap and the inflow are three more planes of the call's own.
//
//   the init kernel (FwdClassify): UpClassify's rule -- NaN where the elevation is NaN and, under edge_nan, on the tile's border
//   and beside a NaN elevation -- with min(load, cap) instead of 0 where nothing flows in.
//
//   tile passes (k_fa_tiles<MULT>): a visit stages value (8 B), proportion (8 B) and the round flag (2 B) of tile + halo, and
//   mult (8 B) in the instantiation for a call that has one; load and cap of the thread's four cells stay in registers, a
//   finished value lives in the cell's LDS slot until the store.  A cell's work is a multiply-add per in-edge and one min, from
//   LDS alone: no edge cost, no hypot, no division.  A cell with pit in-edges is opened only when all its pits are final from
//   an earlier pass; its lane then reads their values from global memory in the round that finishes it (k_du_tiles' rule).
//   What the compiler reports (-Rpass-analysis=kernel-resource-usage, gfx950):
//       k_fa_tiles<false>   VGPRs  98, no scratch, LDS 21,072 B, 4 waves per SIMD
//       k_fa_tiles<true>    VGPRs 100, no scratch, LDS 30,320 B, 4 waves per SIMD
//       k_fa_inflow         VGPRs  25, no scratch, no LDS,       8 waves per SIMD
//       (k_du_tiles: 158 VGPRs, 30,864 B, 3 waves per SIMD)
//
//   the queue (k_du_recount, k_flow_level with du_release): plain Kahn; a level finishes its cells from the planes (FwdFinish).
//
//   the inflow (k_fa_inflow): one pass over the rows AFTER the sweep, launched only when the caller asks for I: every cell pulls
//   again from the final result plane, in the same order with the same operations, which gives the bits of the acc that
//   produced its V.  The sweep itself keeps one value per cell.
#include "flowdist.h"

namespace {

// The switch point of the tile passes, by the rule of flowdist_up.hip: a visit stages 20 B per cell of block + halo (value,
// proportion, stamp) against the 12 B of the reverse sweep whose 16 cells per visit was measured: 16 * 20 / 12 = 27; with mult,
// 28 B: 37.  Timed on the 16384^2 bench tile at each of 0, 8, 16, 27 and 37 (profiles/fwd_accum_cost.txt; without mult / with
// mult / under a capacity with the inflow pass, ms): 232.6 / 237.7 / 246.2, 168.9 / 172.7 / 182.4, 149.2 / 153.3 / 163.0,
// 142.7 / 146.4 / 156.9, 136.0 / 139.5 / 149.5 -- the later the passes stop the better in every form of the call, so one
// value, the best of the five, serves both instantiations.  The results are the same bits at every value.
constexpr int64_t FA_MIN_PER_VISIT = 37;

// the planes of the call (device): mult and cap may be null
struct FwdPlanes { const double *load, *mult, *cap; };

// (every NaN is stored canonical: no arithmetic here may produce DD_OPEN_HI)
__device__ __forceinline__ double fa_value(double tot, double cap) { return tot != tot ? dd_nan() : (cap < tot ? cap : tot); }
__device__ __forceinline__ double fa_cap(const FwdPlanes &P, int32_t c) { return P.cap ? P.cap[c] : INFINITY; }

// the inflow of cell c whose in-neighbours are all final, from the planes
__device__ __forceinline__ double fa_pull(const DistArgs &A, const double *__restrict__ mult, int32_t c, uint32_t cw)
{
    double acc = 0.0;
    auto add = [&](int32_t u, double w) { const double v = A.D[u]; acc += w * (mult ? mult[u] * v : v); };
    dd_for_in_edges(A, c, cw,
        [&](int d, int32_t u) { const double p = A.prop[u]; add(u, du_cardinal(d) ? p : 1 - p); },
        [&](int64_t e) { add(A.pin_src[e], A.pin_w[e]); });
    return acc;
}

// the value of an open cell whose in-neighbours are all final (the level kernel's Finish)
struct FwdFinish {
    FwdPlanes P;
    __device__ __forceinline__ double operator()(const DistArgs &A, int32_t v, uint32_t cw) const
    {
        return fa_value(P.load[v] + fa_pull(A, P.mult, v, cw), fa_cap(P, v));
    }
};

// UpClassify's start set; a cell nothing flows into carries its own load under its cap
struct FwdClassify {
    int edge_nan;
    FwdPlanes P;
    __device__ __forceinline__ bool operator()(const DistArgs &A, int32_t c, int i, int j, uint32_t cw, double &value) const
    {
        const bool open = UpClassify{edge_nan}(A, c, i, j, cw, value);
        if (!open && value == value) value = fa_value(P.load[c], fa_cap(P, c));
        return open;
    }
};

// ---- tile passes (the frame and its rules: flowdist.h; which cells wait for what: k_du_tiles)
template <bool MULT>
__global__ __launch_bounds__(256) void k_fa_tiles(DistArgs A, FwdPlanes P, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state)
{
    __shared__ double Dl[DD_H * DD_H], Pl[DD_H * DD_H], Ml[MULT ? DD_H * DD_H : 1];
    __shared__ uint16_t Fl[DD_H * DD_H];
    __shared__ int32_t s_done, s_open;
    const TileVisit V = dd_visit_begin(tile_state, pass, tiles_x, tiles_y);
    if (!V.run) return;
    const int i0 = V.i0, j0 = V.j0;
    double p = 0.0, mu = 0.0;                           // proportion and mult of the slot being staged (0 off the grid)
    dd_stage(A, pass, V, Dl, Fl, s_done, s_open,
             [&](int32_t c) { p = A.prop[c]; if (MULT) mu = P.mult[c]; },
             [&](int t) { Pl[t] = p; if (MULT) Ml[t] = mu; p = mu = 0.0; });
    const int32_t *stamp = A.queue;
    int idx[4];
    uint32_t word[4], rem[4];
    double ld[4], cp[4];
    bool open[4];
    int n_open = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const CellSlot sl = dd_slot(k, V);
        idx[k] = sl.idx;
        open[k] = false; word[k] = 0; rem[k] = 0; ld[k] = 0.0; cp[k] = INFINITY;
        if (!dd_slot_open(A, sl, Fl)) continue;
        const int32_t c = dd_slot_cell(A, sl);
        n_open++;
        const uint32_t cw = A.cinfo[c] & (0xFFu | CI_PIT_IN);
        if (cw & CI_PIT_IN) {                           // a drain waits until its pits are final from an earlier pass
            bool settled = true;
            for (PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c); b.more(); b.e++) settled = settled && stamp[A.pin_src[b.e]] < pass;
            if (!settled) continue;
        }
        ld[k] = P.load[c]; cp[k] = fa_cap(P, c);
        word[k] = cw; rem[k] = cw & 0xFFu; open[k] = true;
    }
    // the rounds (their invariant: flowdist.h): a cell is ready when all its regular in-neighbours are final.  A lane remembers
    // which in-neighbours it has seen final and asks only for the others; the evaluation runs on selected operands (DD_SEL).  A
    // finished value goes to the cell's LDS slot only (nobody reads it before a later round); it is read back for the store.
    unsigned finished = 0;
    for (unsigned r = 1;; r++) {
        unsigned fresh = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!open[k]) continue;
            uint32_t w = rem[k];
#pragma unroll
            for (int d = 0; d < 8; d++)
                if ((w & (1u << d)) && Fl[idx[k] + NB_DI[d] * DD_H + NB_DJ[d]] < r) w &= ~(1u << d);
            rem[k] = w;
            if (w == 0) { fresh |= 1u << k; open[k] = false; }
        }
        unsigned todo = fresh;
        while (todo) {
            const int k = __ffs((int)todo) - 1;
            todo &= todo - 1;
            const int ix = DD_SEL(idx, k);
            const int li = ix / DD_H;
            const int32_t c = (i0 + li) * A.m + j0 + ix - li * DD_H;
            double acc = 0.0;
            dd_for_in_edges(A, c, DD_SEL(word, k),
                [&](int d, int32_t) {
                    const int s = ix + NB_DI[d] * DD_H + NB_DJ[d];
                    const double q = Pl[s], v = Dl[s];
                    acc += (du_cardinal(d) ? q : 1 - q) * (MULT ? Ml[s] * v : v);
                },
                [&](int64_t e) {
                    const int32_t u = A.pin_src[e];
                    const double v = A.D[u];
                    acc += A.pin_w[e] * (MULT ? P.mult[u] * v : v);
                });
            Dl[ix] = fa_value(DD_SEL(ld, k) + acc, DD_SEL(cp, k));
            Fl[ix] = (uint16_t)r;
        }
        finished |= fresh;
        if (!__syncthreads_or(fresh != 0)) break;
    }
    dd_visit_end(A, pass, V, s_done, s_open, n_open, finished, [&](int, const CellSlot &sl) { return dd_slot_cell(A, sl); },
                 [&](int, const CellSlot &sl) { return Dl[sl.idx]; });
}

// ---- the inflow, after the sweep: NaN where the start set is NaN, 0 where nothing flows in, the pull from the final values
// elsewhere (a cell that never became ready has an in-neighbour that did not either: NaN)
__global__ __launch_bounds__(256) void k_fa_inflow(DistArgs A, const double *__restrict__ mult, int edge_nan, double *__restrict__ I)
{
    for (int i = blockIdx.y; i < A.n; i += gridDim.y)
    for (int j0 = blockIdx.x * blockDim.x; j0 < A.m; j0 += gridDim.x * blockDim.x) {
        const int j = j0 + (int)threadIdx.x;
        if (j >= A.m) continue;
        const int32_t c = i * A.m + j;
        const uint32_t cw = A.cinfo[c];
        double r = 0.0;
        if (UpClassify{edge_nan}(A, c, i, j, cw, r)) {
            r = fa_pull(A, mult, c, cw);
            if (r != r) r = dd_nan();
        }
        I[c] = r;
    }
}

}  // namespace

extern "C" int pydem_fwd_accum(pydem_tile *t, const double *load, const double *mult, const double *cap, int edge_nan, double *out,
                               double *out_inflow, double *ms, int64_t *levels, int64_t *n_unresolved)
{
    PYDEM_TRY(dist_check_tile(t, "pydem_fwd_accum"));
    if (!load) { pydem_set_error("pydem_fwd_accum: no load"); return -2; }
    if (cap)
        for (int64_t k = 0; k < t->NN; k++)
            if (cap[k] != cap[k]) { pydem_set_error("pydem_fwd_accum: cap is NaN at cell %lld", (long long)k); return -2; }
    PYDEM_TRY(dist_check_graph(t, "pydem_fwd_accum"));
    PYDEM_TRY(dist_upload(t, &t->ra_seed, load));
    if (mult) PYDEM_TRY(dist_upload(t, &t->fa_mult, mult));
    if (cap) PYDEM_TRY(dist_upload(t, &t->fa_cap, cap));
    if (out_inflow) PYDEM_TRY(tile_alloc(t, &t->fa_inflow, (size_t)t->NN));
    DistArgs A;
    PYDEM_TRY(dist_state(t, A, 0, 0));
    const FwdPlanes P = {t->ra_seed, mult ? (const double *)t->fa_mult : (const double *)nullptr,
                         cap ? (const double *)t->fa_cap : (const double *)nullptr};
    double sweep_ms = 0.0;
    PYDEM_TRY(dist_sweep<du_release>(t, "fwd_accum", FA_MIN_PER_VISIT, A, FwdClassify{edge_nan, P}, FwdFinish{P}, k_du_recount,
        [&](dim3 grid, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state) {
            if (P.mult) hipLaunchKernelGGL(k_fa_tiles<true>, grid, dim3(256), 0, t->stream, A, P, pass, tiles_x, tiles_y, tile_state);
            else hipLaunchKernelGGL(k_fa_tiles<false>, grid, dim3(256), 0, t->stream, A, P, pass, tiles_x, tiles_y, tile_state);
        }, out, &sweep_ms, levels, n_unresolved));
    if (out_inflow) {                                   // (its time is part of the call's)
        HIP_TRY(hipEventRecord(t->dd_ev[0], t->stream));
        hipLaunchKernelGGL(k_fa_inflow, dist_row_grid(t), dim3(256), 0, t->stream, A, P.mult, edge_nan, t->fa_inflow);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(t->dd_ev[1], t->stream));
        HIP_TRY(hipEventSynchronize(t->dd_ev[1]));
        float el = 0.f;
        HIP_TRY(hipEventElapsedTime(&el, t->dd_ev[0], t->dd_ev[1]));
        sweep_ms += (double)el;
        PYDEM_TRY(tile_plane_copy(t, t->fa_inflow, out_inflow, (size_t)t->NN * 8, true));
    }
    if (ms) *ms = sweep_ms;
    return 0;
}
