// flowacc_tree.hip -- K13: accumulation along the receiver tree of the tile's D-infinity flow graph (the single-flow-direction
// accumulation on the steepest D-infinity receiver, and, cut at the link boundaries, the per-reach catchment totals of TauDEM's
// StreamNet table; no counterpart in the reference; semantics: include/pydem_hip.h, pydem_tree_accum).  The receivers of
// streamnet.hip pick one tree out of the graph; a cell takes the values of its tree in-neighbours and its own load,
//
//     sum:  acc = 0; acc += V[u] in ascending source order; V[c] = load[c] + acc        max / min:  the same fold from load[c]
//
// and under `cut` a tree edge u -> c out of a stream cell u is taken only where c continues u's link (c is a stream cell with
// exactly one stream inflow), so the value at a link's tail is the reduction over that link's own catchment: a keyed reduction
// of every cell into K groups without a floating-point atomic -- ONE lane finishes a cell from final values, in a fixed operand
// order, and a value does not depend on the schedule that produced it.  The sweep's own parts are the value rule and the rounds
// of a tile visit; state, encoding, counters, switches, the visit frame, the init and level kernels, the in-edge walk, the start
// set and the queue of a forward sweep (UpClassify, k_du_recount, du_release) and the host's schedule are the engine's
// (flowdist.h), the receiver pass and its planes are streamnet.h's.  Readiness is the engine's: a cell waits for ALL its graph
// in-neighbours, only the value rule looks at receivers.  The load is the seed plane of pydem_rev_accum.
//
//   the codes (k_ta_codes): one pass over the rows after the receiver pass.  One byte per cell: the receiver code in the low
//   four bits (0..7 the neighbour direction, 8 a pit edge, 15 none) and bit 4 = the cell is in the stream set (never without
//   `cut`, never on a NaN elevation).  A tree in-neighbour from direction d is "low bits == 7 - d", a stream inflow "byte ==
//   16 | (7 - d)": the tile kernel decides everything about a regular in-edge from one staged byte.
//
//   the init kernel (TaClassify): UpClassify's rule -- NaN where the elevation is NaN and, under edge_nan, on the tile's border
//   and beside a NaN elevation -- with the load instead of 0 where nothing flows in.
//
//   tile passes (k_ta_tiles<OP>): a visit stages value (8 B), round flag (2 B) and code byte (1 B) of tile + halo; the load of the
//   thread's four cells stays in registers, a finished value lives in the cell's LDS slot until the store.  The evaluation
//   (ta_eval) counts the stream inflows of a stream cell from the staged bytes, decides the cut and folds the taken in-neighbours
//   in the order of dd_for_in_edges; a pit source is taken when its receiver edge is a pit edge to the cell, once per source.  A
//   cell with pit in-edges is opened only when all its pits are final from an earlier pass; its lane then reads them from global
//   memory in the round that finishes it (k_du_tiles' rule).
//
//   the queue (k_du_recount, k_flow_level with du_release): plain Kahn; a level finishes its cells from the planes (TaFinish<OP>,
//   the same ta_eval).
//
//   the gather (k_ta_gather): after the sweep, the values at a list of cells -- the link tails -- so that a reach table costs K
//   doubles, not a plane.  The list and the values use the int32 plane and the seed plane, both free once the sweep has ended.
//
// What the compiler reports (-Rpass-analysis=kernel-resource-usage, gfx950):
//       k_ta_tiles<0> (sum)  VGPRs  90, no scratch, LDS 12,992 B, 5 waves per SIMD
//       k_ta_tiles<1> (max)  VGPRs  89, no scratch, LDS 12,992 B, 5 waves per SIMD
//       k_ta_tiles<2> (min)  VGPRs  89, no scratch, LDS 12,992 B, 5 waves per SIMD
//       k_ta_codes           VGPRs   8, no scratch, no LDS,       8 waves per SIMD
//       k_ta_gather          VGPRs   8, no scratch, no LDS,       8 waves per SIMD
//       (k_flow_level<TaFinish<0 / 1 / 2>>: 26 / 24 / 24 VGPRs, k_flow_init<TaClassify>: 42, none with scratch; k_sn_fwd_tiles:
//       54 VGPRs, 12,992 B, 8 waves; k_fa_tiles<false>: 98 VGPRs, 21,072 B, 4 waves.  The registers over k_sn_fwd_tiles are the
//       four loads and the second walk over the in-edges; LDS would allow 12 workgroups per CU, the registers allow 5.)
#include "streamnet.h"

namespace {

// The switch point of the tile passes, by the rule of flowdist_up.hip: a visit stages 11 B per cell of block + halo (value, round
// flag, code) against the 12 B of the reverse sweep whose 16 cells per visit was measured: 16 * 11 / 12 = 15.  Timed on the 16384^2
// bench tile, streams at the top 1 % of uca, at 0, 4, 8, 16, 27 and 37 (profiles/tree_accum_cost.txt; cut / whole tree, under
// edge_nan, ms of the call with its two row passes): 208.8 / 204.3, 211.9 / 206.6, 165.4 / 159.8, 150.6 / 145.1, 145.4 / 139.8,
// 140.2 / 134.6 -- as for k_fa_tiles, whose open set and visit rule these are, the earlier the passes hand over to the queue the
// better, and the rule's 15 would cost 7 %: the best of the six, the siblings' 37, is kept.  The result bits are the same at every
// value (the checksums of the profile; tests/test_gpu_tree_accum.py::test_schedules).
constexpr int64_t TA_MIN_PER_VISIT = 37;

constexpr uint8_t TA_S = 16, TA_CODE = 15;              // the code byte: bit 4 = in the stream set, low bits = the receiver code

// the planes of the call (device)
struct TaPlanes { const double *load; const int32_t *recv; const uint8_t *sc; };

__global__ __launch_bounds__(256) void k_ta_codes(DistArgs A, const uint8_t *__restrict__ code, const double *__restrict__ uca,
                                                  double threshold, int cut, uint8_t *__restrict__ sc)
{
    for (int i = blockIdx.y; i < A.n; i += gridDim.y)
    for (int j0 = blockIdx.x * blockDim.x; j0 < A.m; j0 += gridDim.x * blockDim.x) {
        const int j = j0 + (int)threadIdx.x;
        if (j >= A.m) continue;
        const int32_t c = i * A.m + j;
        bool tg = false;
        if (cut) {
            const double z = A.elev[c];
            tg = z == z && (uca ? uca[c] >= threshold : A.mask[c] != 0);     // (NaN is never a stream)
        }
        sc[c] = (uint8_t)((code[c] & TA_CODE) | (tg ? TA_S : 0));
    }
}

// (every NaN is stored canonical: no arithmetic here may produce DD_OPEN_HI)
__device__ __forceinline__ double ta_canon(double v) { return v != v ? dd_nan() : v; }

// the fold of one cell: sum from 0 with the load added last, max / min from the load
template <int OP>
struct TaAcc {
    double a;
    bool nan;
    __device__ __forceinline__ explicit TaAcc(double load) : a(OP == 0 ? 0.0 : load), nan(load != load) {}
    __device__ __forceinline__ void add(double v)
    {
        if (OP == 0) a += v;
        else { nan = nan || v != v; a = (OP == 1 ? v > a : v < a) ? v : a; }
    }
    __device__ __forceinline__ double result(double load) const { return OP == 0 ? ta_canon(load + a) : (nan ? dd_nan() : a); }
};

// The value of cell c (graph word cw, code byte `me`, load `load`) whose graph in-neighbours are all final.  code(d) / val(d):
// code byte and value of the regular in-neighbour d (from LDS in a tile visit, from the planes in a level); pit sources are read
// from the planes.  A source with two pit entries to c counts once (the list is sorted by (dst, src): `last` is the source
// of the entry before; a regular edge from another source between them does not separate them).
template <int OP, class Code, class Val>
__device__ __forceinline__ double ta_eval(const DistArgs &A, const TaPlanes &P, int32_t c, uint32_t cw, uint8_t me, double load,
                                          Code code, Val val)
{
    bool cont = false;                                  // c continues the link of its one stream inflow
    if (me & TA_S) {
        int n_in = 0;
#pragma unroll
        for (int d = 0; d < 8; d++)
            if ((cw & (1u << d)) && code(d) == (TA_S | (7 - d))) n_in++;
        if (cw & CI_PIT_IN) {
            int32_t last = -1;
            for (PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c); b.more(); b.e++) {
                const int32_t u = A.pin_src[b.e];
                if (u != last && P.sc[u] == (TA_S | SN_PIT) && P.recv[u] == c) n_in++;
                last = u;
            }
        }
        cont = n_in == 1;
    }
    TaAcc<OP> acc(load);
    int32_t last = -1;
    dd_for_in_edges(A, c, cw,
        [&](int d, int32_t) {
            const uint8_t b = code(d);
            if ((b & TA_CODE) == 7 - d && (cont || !(b & TA_S))) acc.add(val(d));
        },
        [&](int64_t e) {
            const int32_t u = A.pin_src[e];
            if (u != last) {
                const uint8_t b = P.sc[u];
                if ((b & TA_CODE) == SN_PIT && P.recv[u] == c && (cont || !(b & TA_S))) acc.add(A.D[u]);
            }
            last = u;
        });
    return acc.result(load);
}

// the value of an open cell whose in-neighbours are all final, from the planes (the level kernel's Finish)
template <int OP>
struct TaFinish {
    TaPlanes P;
    __device__ __forceinline__ double operator()(const DistArgs &A, int32_t c, uint32_t cw) const
    {
        return ta_eval<OP>(A, P, c, cw, P.sc[c], P.load[c],
                           [&](int d) { return P.sc[c + NB_DI[d] * A.m + NB_DJ[d]]; },
                           [&](int d) { return A.D[c + NB_DI[d] * A.m + NB_DJ[d]]; });
    }
};

// UpClassify's start set; a cell nothing flows into carries its own load
struct TaClassify {
    int edge_nan;
    const double *load;
    __device__ __forceinline__ bool operator()(const DistArgs &A, int32_t c, int i, int j, uint32_t cw, double &value) const
    {
        const bool open = UpClassify{edge_nan}(A, c, i, j, cw, value);
        if (!open && value == value) value = ta_canon(load[c]);
        return open;
    }
};

// ---- tile passes (the frame and its rules: flowdist.h; which cells wait for what, and the rounds: k_sn_fwd_tiles)
template <int OP>
__global__ __launch_bounds__(256) void k_ta_tiles(DistArgs A, TaPlanes P, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state)
{
    __shared__ double Dl[DD_H * DD_H];
    __shared__ uint16_t Fl[DD_H * DD_H];
    __shared__ uint8_t Cl[DD_H * DD_H];
    __shared__ int32_t s_done, s_open;
    const TileVisit V = dd_visit_begin(tile_state, pass, tiles_x, tiles_y);
    if (!V.run) return;
    const int i0 = V.i0, j0 = V.j0;
    uint8_t cb = TA_CODE;                               // code byte of the slot being staged (no receiver, no stream off the grid)
    dd_stage(A, pass, V, Dl, Fl, s_done, s_open,
             [&](int32_t c) { cb = P.sc[c]; },
             [&](int t) { Cl[t] = cb; cb = TA_CODE; });
    const int32_t *stamp = A.queue;
    int idx[4];
    uint32_t word[4], rem[4];
    double ld[4];
    bool open[4];
    int n_open = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const CellSlot sl = dd_slot(k, V);
        idx[k] = sl.idx;
        open[k] = false; word[k] = 0; rem[k] = 0; ld[k] = 0.0;
        if (!dd_slot_open(A, sl, Fl)) continue;
        const int32_t c = dd_slot_cell(A, sl);
        n_open++;
        const uint32_t cw = A.cinfo[c] & (0xFFu | CI_PIT_IN);
        if (cw & CI_PIT_IN) {                           // a drain waits until its pits are final from an earlier pass
            bool settled = true;
            for (PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c); b.more(); b.e++) settled = settled && stamp[A.pin_src[b.e]] < pass;
            if (!settled) continue;
        }
        ld[k] = P.load[c];
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
            Dl[ix] = ta_eval<OP>(A, P, c, DD_SEL(word, k), Cl[ix], DD_SEL(ld, k),
                                 [&](int d) { return Cl[ix + NB_DI[d] * DD_H + NB_DJ[d]]; },
                                 [&](int d) { return Dl[ix + NB_DI[d] * DD_H + NB_DJ[d]]; });
            Fl[ix] = (uint16_t)r;
        }
        finished |= fresh;
        if (!__syncthreads_or(fresh != 0)) break;
    }
    dd_visit_end(A, pass, V, s_done, s_open, n_open, finished, [&](int, const CellSlot &sl) { return dd_slot_cell(A, sl); },
                 [&](int, const CellSlot &sl) { return Dl[sl.idx]; });
}

// ---- the values at a list of cells (every entry was checked against [0, n m) on the host)
__global__ __launch_bounds__(256) void k_ta_gather(const double *__restrict__ D, const int32_t *__restrict__ at, int64_t n_at,
                                                   double *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_at; k += (int64_t)gridDim.x * blockDim.x) out[k] = D[at[k]];
}

template <int OP>
int ta_sweep(pydem_tile *t, const DistArgs &A, const TaPlanes &P, int edge_nan, double *out, double *ms, int64_t *levels, int64_t *n_unresolved)
{
    return dist_sweep<du_release>(t, "tree_accum", TA_MIN_PER_VISIT, A, TaClassify{edge_nan, P.load}, TaFinish<OP>{P}, k_du_recount,
        [&](dim3 grid, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state) {
            hipLaunchKernelGGL(k_ta_tiles<OP>, grid, dim3(256), 0, t->stream, A, P, pass, tiles_x, tiles_y, tile_state);
        }, out, ms, levels, n_unresolved);
}

}  // namespace

extern "C" int pydem_tree_accum(pydem_tile *t, int op, const double *load, int cut, const uint8_t *streams, double uca_threshold,
                                int edge_nan, double *out, const int32_t *at, int64_t n_at, double *at_out, double *ms,
                                int64_t *levels, int64_t *n_unresolved)
{
    PYDEM_TRY(dist_check_tile(t, "pydem_tree_accum"));
    if (op < 0 || op > 2) { pydem_set_error("pydem_tree_accum: op must be 0 (sum), 1 (max) or 2 (min) (got %d)", op); return -2; }
    if (!load) { pydem_set_error("pydem_tree_accum: no load"); return -2; }
    if (cut) PYDEM_TRY(sn_check_threshold("pydem_tree_accum", streams, uca_threshold));
    if (!at || !at_out || n_at < 0) n_at = 0;
    for (int64_t k = 0; k < n_at; k++)
        if (at[k] < 0 || (int64_t)at[k] >= t->NN) {
            pydem_set_error("pydem_tree_accum: at[%lld] = %d is outside the tile's %lld cells", (long long)k, (int)at[k], (long long)t->NN);
            return -2;
        }
    PYDEM_TRY(dist_check_graph(t, "pydem_tree_accum"));
    if (cut) PYDEM_TRY(sn_stream_set(t, "pydem_tree_accum", streams));
    PYDEM_TRY(dist_upload(t, &t->ra_seed, load));
    PYDEM_TRY(tile_alloc(t, &t->sn_recv, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->sn_code, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->ta_sc, (size_t)t->NN));
    DistArgs A;
    PYDEM_TRY(dist_state(t, A, 0, 0));
    const TaPlanes P = {t->ra_seed, t->sn_recv, t->ta_sc};
    double pre_ms = 0.0, sweep_ms = 0.0;
    {                                                   // (the two passes over the rows are part of the call's time)
        HIP_TRY(hipEventRecord(t->dd_ev[0], t->stream));
        PYDEM_TRY(sn_receivers(t, A));
        hipLaunchKernelGGL(k_ta_codes, dist_row_grid(t), dim3(256), 0, t->stream, A, (const uint8_t *)t->sn_code,
                           cut && !streams ? (const double *)t->uca : (const double *)nullptr, uca_threshold, cut ? 1 : 0, t->ta_sc);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(t->dd_ev[1], t->stream));
        HIP_TRY(hipEventSynchronize(t->dd_ev[1]));
        float el = 0.f;
        HIP_TRY(hipEventElapsedTime(&el, t->dd_ev[0], t->dd_ev[1]));
        pre_ms = (double)el;
    }
    if (op == 0) PYDEM_TRY(ta_sweep<0>(t, A, P, edge_nan, out, &sweep_ms, levels, n_unresolved));
    else if (op == 1) PYDEM_TRY(ta_sweep<1>(t, A, P, edge_nan, out, &sweep_ms, levels, n_unresolved));
    else PYDEM_TRY(ta_sweep<2>(t, A, P, edge_nan, out, &sweep_ms, levels, n_unresolved));
    // the gather: the list in the int32 plane, the values in the seed plane (both free from the end of the sweep), in pieces
    // of at most the plane's cells
    for (int64_t k0 = 0; k0 < n_at; k0 += t->NN) {
        const int64_t cnt = n_at - k0 < t->NN ? n_at - k0 : t->NN;
        PYDEM_TRY(tile_plane_copy(t, t->dd_queue, const_cast<int32_t *>(at + k0), (size_t)cnt * sizeof(int32_t), false));
        hipLaunchKernelGGL(k_ta_gather, dim3(grid_for(cnt, 2048)), dim3(256), 0, t->stream, (const double *)t->dd_out,
                           (const int32_t *)t->dd_queue, cnt, t->ra_seed);
        HIP_TRY(hipGetLastError());
        PYDEM_TRY(tile_plane_copy(t, t->ra_seed, at_out + k0, (size_t)cnt * sizeof(double), true));
    }
    if (ms) *ms = pre_ms + sweep_ms;
    return 0;
}
