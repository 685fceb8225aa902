// streamnet.hip -- K12: the stream network on the tile's D-infinity flow graph (TauDEM's StreamNet / GridNet, done there on D8;
// no counterpart in the reference; semantics: include/pydem_hip.h, pydem_stream_network): every cell's receiver -- the
// destination of its heaviest out-edge --, the Strahler order and the link of every stream cell, the sub-basin of every cell.
// The D-infinity graph is a DAG with up to two regular out-edges per cell; the receivers pick the one tree it contains, and
// the network is a labelling over that tree.  Three steps:
//
//   the receivers (k_sn_receiver, in streamnet.h with the planes: flowacc_tree.hip runs the same pass): one pass over the
//   rows.  Per cell the first out-edge of greatest weight in the order of
//   dd_for_out_edges; its destination goes to an int32 plane, which edge it is to a byte plane (0..7: the neighbour direction
//   in NB_DI / NB_DJ order, 8: a pit edge, 255: none).  They depend on the graph alone.
//
//   order and links: ONE forward sweep through dist_sweep<du_release> with k_du_recount.  The engine carries one double per
//   cell; it holds order + 64 * (head + 1) as an exact integer (< 2^37 for int32 cells, 0 off the streams, never the open
//   pattern), so the value of a stream inflow says everything its receiver needs: a second plane would have cost a second LDS
//   slot array in the tile kernel, which keeps a finished value in its slot until the store.  Readiness is the engine's: a cell
//   waits for all its graph in-neighbours; only the value rule looks at receivers.  A stream inflow from neighbour d is "value
//   != 0 and code == 7 - d"; a pit in-edge is one when its source's code is 8 and its receiver the cell (sources read from the
//   planes; the drain opens only when all its pits are final from an earlier pass, k_du_tiles' rule).  Maximum, count and head
//   are integers: the result does not depend on the order in which the inflows are looked at.
//
//   basins: one reverse sweep through dist_sweep<dd_release> with k_dd_recount, modelled on k_ra_tiles, launched only when the
//   basins are asked for.  The seed plane (pydem_rev_accum's) holds the forward result, copied device to device; stream cells
//   are absorbing and carry their raw link label (-1 where the forward sweep left them unresolved), a cell without a receiver
//   carries 0, every other cell waits for all its out-neighbours and then takes the value of its receiver's slot.  A cell with
//   pit out-edges only is finished at load time when all its drains are final from an earlier pass; one with both kinds is
//   left to the queue (k_ra_tiles' rule).
//
//   k_sn_unpack turns a result plane into int32 (order, raw link or raw basin; the NaN of an unresolved cell becomes -1) in the
//   sweep's int32 plane, which is free once a sweep has ended, and counts the -1 of the basins.
//
// State: the engine's (flowdist.h) and the seed plane; the two receiver planes (5 B per cell) are the call's own, allocated on
// first use and freed with the tile.  What the compiler reports (-Rpass-analysis=kernel-resource-usage, gfx950):
//       k_sn_receiver       VGPRs  19, no scratch, no LDS,       8 waves per SIMD
//       k_sn_fwd_tiles      VGPRs  54, no scratch, LDS 12,992 B, 8 waves per SIMD
//       k_sn_rev_tiles      VGPRs  34, no scratch, LDS 11,824 B, 8 waves per SIMD
//       k_sn_unpack         VGPRs  12, no scratch, LDS      4 B, 8 waves per SIMD
//       (the level kernels: k_flow_level<SnFwdFinish> 28 VGPRs, k_flow_level<SnRevFinish> 20; k_fa_tiles<false>: 98 VGPRs,
//       21,072 B, 4 waves per SIMD)
#include "streamnet.h"

namespace {

// The switch points of the tile passes (the cells a visit has to finish on average for another pass to beat the queue), one
// per sweep, each started from its sibling's value and timed on the 16384^2 bench tile with the streams at the top 1 % of uca at
// 0, 4, 8, 16, 27 and 37 (profiles/streamnet_cost.txt; forward / reverse sweep, ms): 39.6 / 82.3, 31.9 / 82.4, 32.2 / 82.8,
// 32.0 / 82.8, 31.5 / 84.9, 32.0 / 91.3.  Forward: 2.7 M of 268 M cells are open after the init kernel; the first pass, which
// visits every block, finishes 1.78 cells per visit, so 4 to 37 are one schedule (one pass, then the queue) and 0 -- passes to
// the end -- is 24 % slower: flowacc_fwd.hip's 37 stays.  Reverse: 0, 4 and 8 are one schedule (passes to the end), 27 and 37
// hand 2.7 M and 9.4 M cells to the queue and lose 2.5 and 8.9 ms: flowacc_rev.hip's 4 stays.  The bits are the same at every value.
constexpr int64_t SN_FWD_MIN_PER_VISIT = 37;
constexpr int64_t SN_REV_MIN_PER_VISIT = 4;

constexpr int SN_MINUS = DD_USER;                       // the engine's free 64-bit counter word: the -1 of the basins (k_sn_unpack)

// ---- order and links: the value of a stream cell, and its rule
__device__ __forceinline__ double sn_pack(int order, int64_t head1) { return (double)((int64_t)order + 64 * head1); }

struct SnIn { int n = 0, hi = 0, k = 0; int64_t head1 = 0; };
// one stream inflow of value v (head1: only read when it stays the only one)
__device__ __forceinline__ void sn_add(SnIn &S, double v)
{
    const int64_t x = (int64_t)v;
    const int o = (int)(x & 63);
    S.n++;
    if (o > S.hi) { S.hi = o; S.k = 1; } else if (o == S.hi) S.k++;
    S.head1 = x >> 6;
}
__device__ __forceinline__ double sn_value(const SnIn &S, int32_t c)
{
    if (S.n == 1) return sn_pack(S.hi, S.head1);                        // the inflow's link goes on
    return sn_pack(S.n == 0 ? 1 : (S.k >= 2 ? S.hi + 1 : S.hi), (int64_t)c + 1);    // a source, or a junction: a link head
}

// a pit in-edge e of cell c (source u) is a stream inflow when it is u's receiver edge and u is a stream cell; a source with
// two entries to c counts once (the list is sorted by (dst, src): `last` is the source of the entry before)
__device__ __forceinline__ void sn_pit_in(const DistArgs &A, const SnPlanes &P, SnIn &S, int32_t c, int64_t e, int32_t &last)
{
    const int32_t u = A.pin_src[e];
    if (u != last && P.code[u] == SN_PIT && P.recv[u] == c) {
        const double v = A.D[u];
        if (v != 0.0) sn_add(S, v);
    }
    last = u;
}

// the value of an open cell whose in-neighbours are all final, from the planes (the level kernel's Finish)
struct SnFwdFinish {
    SnPlanes P;
    __device__ __forceinline__ double operator()(const DistArgs &A, int32_t c, uint32_t cw) const
    {
        SnIn S;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            if (!(cw & (1u << d))) continue;
            const int32_t u = c + NB_DI[d] * A.m + NB_DJ[d];
            const double v = A.D[u];
            if (v != 0.0 && P.code[u] == 7 - d) sn_add(S, v);
        }
        if (cw & CI_PIT_IN) {
            int32_t last = -1;
            for (PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c); b.more(); b.e++) sn_pit_in(A, P, S, c, b.e, last);
        }
        return sn_value(S, c);
    }
};

// off the streams (and on NaN elevations): 0; stream cells nothing flows into: order 1, their own link; the others are open
struct SnFwdClassify {
    const double *uca;
    double threshold;
    __device__ __forceinline__ bool operator()(const DistArgs &A, int32_t c, int, int, uint32_t cw, double &value) const
    {
        const double z = A.elev[c];
        const bool tg = z == z && (uca ? uca[c] >= threshold : A.mask[c] != 0);     // (NaN is never a stream)
        value = 0.0;
        if (!tg) return false;
        if (cw & (0xFFu | CI_PIT_IN)) return true;
        value = sn_pack(1, (int64_t)c + 1);
        return false;
    }
};

// ---- tile passes of the forward sweep (the frame and its rules: flowdist.h; which cells wait for what: k_du_tiles)
__global__ __launch_bounds__(256) void k_sn_fwd_tiles(DistArgs A, SnPlanes P, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state)
{
    __shared__ double Dl[DD_H * DD_H];
    __shared__ uint16_t Fl[DD_H * DD_H];
    __shared__ uint8_t Cl[DD_H * DD_H];
    __shared__ int32_t s_done, s_open;
    const TileVisit V = dd_visit_begin(tile_state, pass, tiles_x, tiles_y);
    if (!V.run) return;
    const int i0 = V.i0, j0 = V.j0;
    uint8_t cb = SN_NONE;                               // receiver code of the slot being staged (none off the grid)
    dd_stage(A, pass, V, Dl, Fl, s_done, s_open,
             [&](int32_t c) { cb = P.code[c]; },
             [&](int t) { Cl[t] = cb; cb = SN_NONE; });
    const int32_t *stamp = A.queue;
    int idx[4];
    uint32_t word[4], rem[4];
    bool open[4];
    int n_open = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const CellSlot sl = dd_slot(k, V);
        idx[k] = sl.idx;
        open[k] = false; word[k] = 0; rem[k] = 0;
        if (!dd_slot_open(A, sl, Fl)) continue;
        const int32_t c = dd_slot_cell(A, sl);
        n_open++;
        const uint32_t cw = A.cinfo[c] & (0xFFu | CI_PIT_IN);
        if (cw & CI_PIT_IN) {                           // a drain waits until its pits are final from an earlier pass
            bool settled = true;
            for (PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c); b.more(); b.e++) settled = settled && stamp[A.pin_src[b.e]] < pass;
            if (!settled) continue;
        }
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
            const uint32_t cw = DD_SEL(word, k);
            const int li = ix / DD_H;
            const int32_t c = (i0 + li) * A.m + j0 + ix - li * DD_H;
            SnIn S;
#pragma unroll
            for (int d = 0; d < 8; d++) {
                if (!(cw & (1u << d))) continue;
                const int s = ix + NB_DI[d] * DD_H + NB_DJ[d];
                const double v = Dl[s];
                if (v != 0.0 && Cl[s] == 7 - d) sn_add(S, v);
            }
            if (cw & CI_PIT_IN) {
                int32_t last = -1;
                for (PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c); b.more(); b.e++) sn_pit_in(A, P, S, c, b.e, last);
            }
            Dl[ix] = sn_value(S, c);
            Fl[ix] = (uint16_t)r;
        }
        finished |= fresh;
        if (!__syncthreads_or(fresh != 0)) break;
    }
    dd_visit_end(A, pass, V, s_done, s_open, n_open, finished, [&](int, const CellSlot &sl) { return dd_slot_cell(A, sl); },
                 [&](int, const CellSlot &sl) { return Dl[sl.idx]; });
}

// ---- basins
// the raw label a stream cell carries into the reverse sweep, from the forward result v (!= 0): NaN = unresolved = -1
__device__ __forceinline__ double sn_label(double v) { return v != v ? -1.0 : (double)((int64_t)v >> 6); }

// NaN elevations and cells without an out-edge (no receiver): 0; stream cells: their raw link label; the others are open
struct SnRevClassify {
    const double *fwd;
    __device__ __forceinline__ bool operator()(const DistArgs &A, int32_t c, int, int, uint32_t cw, double &value) const
    {
        const double z = A.elev[c], v = fwd[c];
        value = 0.0;
        if (z != z) return false;
        if (v != 0.0) { value = sn_label(v); return false; }
        return (cw & (CI_OUT1 | CI_OUT2 | CI_PIT_OUT)) != 0;
    }
};

// the value of an open cell whose out-neighbours are all final: its receiver's (the level kernel's Finish)
struct SnRevFinish {
    SnPlanes P;
    __device__ __forceinline__ double operator()(const DistArgs &A, int32_t c, uint32_t) const
    {
        const int32_t rc = P.recv[c];
        return rc >= 0 ? A.D[rc] : 0.0;
    }
};

// tile passes of the reverse sweep (the frame and its rules: flowdist.h; which cells wait for what: k_ra_tiles)
__global__ __launch_bounds__(256) void k_sn_rev_tiles(DistArgs A, SnPlanes P, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state)
{
    __shared__ double Dl[DD_H * DD_H];
    __shared__ uint16_t Fl[DD_H * DD_H];
    __shared__ int32_t s_done, s_open;
    const TileVisit V = dd_visit_begin(tile_state, pass, tiles_x, tiles_y);
    if (!V.run) return;
    dd_stage(A, pass, V, Dl, Fl, s_done, s_open);
    const int32_t *stamp = A.queue;
    int idx[4], rs[4];                                  // rs: LDS slot of the receiver
    uint32_t dst[4];                                    // LDS slots of the two destinations, + 1 (0: no such edge): first | second << 16
    bool open[4], pend[4];
    int n_open = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const CellSlot sl = dd_slot(k, V);
        idx[k] = sl.idx;
        open[k] = false; pend[k] = false; dst[k] = 0; rs[k] = sl.idx;
        if (!dd_slot_open(A, sl, Fl)) continue;
        const int32_t c = dd_slot_cell(A, sl);
        n_open++;
        const uint32_t cw = A.cinfo[c];
        const bool regular = (cw & (CI_OUT1 | CI_OUT2)) != 0;
        if (regular && (cw & CI_PIT_OUT)) continue;
        if (!regular) {
            bool settled = true;
            for (PitBlock b = dd_pit_block(A.pit_src, A.n_pit, c); b.more(); b.e++) settled = settled && stamp[A.pit_dst[b.e]] < pass;
            // (the value waits in LDS behind the cell's open flag: nobody reads it before round 1 has set the flag)
            if (settled) { const int32_t rc = P.recv[c]; pend[k] = true; Dl[idx[k]] = rc >= 0 ? A.D[rc] : 0.0; open[k] = true; }
            continue;
        }
        const int cd = P.code[c];                       // (0..7: the heaviest of regular edges only is a regular edge)
        if (cd > 7) continue;
        const Facet f = dd_facet_sorted(A, cw, 0.0);
        if (f.a.has) dst[k] = (uint32_t)(idx[k] + f.a.di * DD_H + f.a.dj + 1);
        if (f.b.has) dst[k] |= (uint32_t)(idx[k] + f.b.di * DD_H + f.b.dj + 1) << 16;
        rs[k] = idx[k] + NB_DI[cd] * DD_H + NB_DJ[cd];
        open[k] = true;
    }
    // the rounds (their invariant: flowdist.h): a copy of one LDS value per cell, under the slot's predicate
    unsigned finished = 0;
    for (unsigned r = 1;; r++) {
        unsigned fresh = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!open[k]) continue;
            if (!pend[k]) {
                const int d1 = (int)(dst[k] & 0xFFFFu) - 1, d2 = (int)(dst[k] >> 16) - 1;
                if (!((d1 < 0 || Fl[d1] < r) && (d2 < 0 || Fl[d2] < r))) continue;
                Dl[idx[k]] = Dl[rs[k]];
            }
            Fl[idx[k]] = (uint16_t)r;
            open[k] = false;
            fresh |= 1u << k;
        }
        finished |= fresh;
        if (!__syncthreads_or(fresh != 0)) break;
    }
    dd_visit_end(A, pass, V, s_done, s_open, n_open, finished, [&](int, const CellSlot &sl) { return dd_slot_cell(A, sl); },
                 [&](int, const CellSlot &sl) { return Dl[sl.idx]; });
}

// ---- a result plane as int32.  what 0: the order, 1: the raw link label of a forward result; 2: a reverse result as it is,
// its -1 counted into *n_minus.  The NaN of a cell that never became ready: -1.
__global__ __launch_bounds__(256) void k_sn_unpack(const double *__restrict__ src, int64_t NN, int what, int32_t *__restrict__ out,
                                                   unsigned long long *n_minus)
{
    __shared__ int32_t s_minus;
    if (threadIdx.x == 0) s_minus = 0;
    __syncthreads();
    int32_t mine = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const double v = src[c];
        int32_t r = -1;
        if (v == v) {
            const int64_t x = (int64_t)v;
            r = (int32_t)(what == 0 ? x & 63 : (what == 1 ? x >> 6 : x));
        }
        out[c] = r;
        mine += r == -1 ? 1 : 0;
    }
    if (what == 2) {
        if (mine) atomicAdd(&s_minus, mine);
        __syncthreads();
        if (threadIdx.x == 0 && s_minus) atomicAdd(n_minus, (unsigned long long)s_minus);
    }
}

}  // namespace

// a result plane of the sweep that has just ended, as int32 on the host (through the sweep's int32 plane, free from its end to
// the next init); what: k_sn_unpack's
static int sn_download(pydem_tile *t, const double *src, int what, int32_t *host)
{
    hipLaunchKernelGGL(k_sn_unpack, dim3(grid_for(t->NN, 2048)), dim3(256), 0, t->stream, src, t->NN, what, t->dd_queue,
                       reinterpret_cast<unsigned long long *>(t->dd_ctr + SN_MINUS));
    HIP_TRY(hipGetLastError());
    return tile_plane_copy(t, t->dd_queue, host, (size_t)t->NN * sizeof(int32_t), true);
}

extern "C" int pydem_stream_network(pydem_tile *t, const uint8_t *streams, double uca_threshold, int32_t *receiver, int32_t *order,
                                    int32_t *link, int32_t *basin, double *ms, int64_t *levels, int64_t *n_unresolved)
{
    PYDEM_TRY(dist_check_tile(t, "pydem_stream_network"));
    const bool sweeps = order || link || basin;
    if (sweeps) PYDEM_TRY(sn_check_threshold("pydem_stream_network", streams, uca_threshold));
    PYDEM_TRY(dist_check_graph(t, "pydem_stream_network"));
    if (sweeps) PYDEM_TRY(sn_stream_set(t, "pydem_stream_network", streams));
    PYDEM_TRY(tile_alloc(t, &t->sn_recv, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->sn_code, (size_t)t->NN));
    DistArgs A;
    PYDEM_TRY(dist_state(t, A, 0, 0));
    const SnPlanes P = {t->sn_recv, t->sn_code};
    double part_ms[3] = {0.0, 0.0, 0.0};
    int64_t part_levels[2] = {0, 0}, part_left[2] = {0, 0};
    {
        HIP_TRY(hipEventRecord(t->dd_ev[0], t->stream));
        PYDEM_TRY(sn_receivers(t, A));               // (streamnet.h)
        HIP_TRY(hipEventRecord(t->dd_ev[1], t->stream));
        HIP_TRY(hipEventSynchronize(t->dd_ev[1]));
        float el = 0.f;
        HIP_TRY(hipEventElapsedTime(&el, t->dd_ev[0], t->dd_ev[1]));
        part_ms[0] = (double)el;
    }
    if (receiver) PYDEM_TRY(tile_plane_copy(t, t->sn_recv, receiver, (size_t)t->NN * sizeof(int32_t), true));
    if (sweeps) {
        const SnFwdClassify start = {streams ? (const double *)nullptr : (const double *)t->uca, uca_threshold};
        PYDEM_TRY(dist_sweep<du_release>(t, "stream_network order", SN_FWD_MIN_PER_VISIT, A, start, SnFwdFinish{P}, k_du_recount,
            [&](dim3 grid, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state) {
                hipLaunchKernelGGL(k_sn_fwd_tiles, grid, dim3(256), 0, t->stream, A, P, pass, tiles_x, tiles_y, tile_state);
            }, (double *)nullptr, &part_ms[1], &part_levels[0], &part_left[0]));
        if (basin) {                                    // the forward result is the seed of the reverse sweep
            PYDEM_TRY(tile_alloc(t, &t->ra_seed, (size_t)t->NN));
            HIP_TRY(hipMemcpyAsync(t->ra_seed, t->dd_out, (size_t)t->NN * sizeof(double), hipMemcpyDeviceToDevice, t->stream));
        }
        if (order) PYDEM_TRY(sn_download(t, t->dd_out, 0, order));
        if (link) PYDEM_TRY(sn_download(t, t->dd_out, 1, link));
    }
    if (basin) {
        PYDEM_TRY(dist_sweep<dd_release>(t, "stream_network basins", SN_REV_MIN_PER_VISIT, A, SnRevClassify{t->ra_seed}, SnRevFinish{P}, k_dd_recount,
            [&](dim3 grid, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state) {
                hipLaunchKernelGGL(k_sn_rev_tiles, grid, dim3(256), 0, t->stream, A, P, pass, tiles_x, tiles_y, tile_state);
            }, (double *)nullptr, &part_ms[2], &part_levels[1], (int64_t *)nullptr));
        HIP_TRY(hipMemsetAsync(t->dd_ctr + SN_MINUS, 0, 2 * sizeof(int32_t), t->stream));
        PYDEM_TRY(sn_download(t, t->dd_out, 2, basin));
        HIP_TRY(hipMemcpyAsync(t->dd_h_ctr, t->dd_ctr, DD_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        part_left[1] = (int64_t)(((uint64_t)(uint32_t)t->dd_h_ctr[SN_MINUS + 1] << 32) | (uint32_t)t->dd_h_ctr[SN_MINUS]);
    }
    for (int k = 0; k < 3; k++) if (ms) ms[k] = part_ms[k];
    for (int k = 0; k < 2; k++) {
        if (levels) levels[k] = part_levels[k];
        if (n_unresolved) n_unresolved[k] = part_left[k];
    }
    return 0;
}
