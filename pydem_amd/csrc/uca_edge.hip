// uca_edge.hip -- K7 cross-tile edge fix-up: classic, incremental, compact, condensed and queued rounds.
//
// Replaces, for one tile (reference pydem/dem_processing.py unless noted):
//   K7  edge-resolution rounds: calc_uca(uca_init=, edge_init_data=) :724-771 with _calc_uca_chunk_update :778-862
//       (count-based Kahn on the cells downstream of the seeds).
//   K7i incremental rounds: the same rule, with the counts, deltas and FINAL flags kept between rounds, in the plane
//       form, the compact record form and the condensed form on the watched lines (uca_cond.inl; its operator is
//       built on the device by uca_cbuild.inl), singly or as queued waves gated by a device word.
// The rounds run on the flow graph that uca.hip built (uca_graph.h holds what the two units share) and are bounded
// by dependent memory latency: a round touches a few thousand cells downstream of an edge.
#include "uca_graph.h"
#include <hipcub/hipcub.hpp>      // scans / radix sorts of the device operator build (uca_cbuild.inl)
#include <algorithm>
#include <functional>
#include <memory>
#include <thread>
#include <vector>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

namespace {

// ------------------------------------------------------------------------------- K7
// Edge-resolution round for one tile: DEMProcessor.calc_uca(uca_init=..., edge_init_data=...)
// (reference pydem/dem_processing.py:720-771) and _calc_uca_chunk_update (:778-862) with the
// native floods cyutils.drain_connections (cyutils.pyx:35-72) and drain_area (:78-187).
// The reference rebuilds section/proportion/adjacency on every call (:787-793); here the graph
// built by pydem_uca is still resident and is reused.  Only cells downstream of the seeds are
// touched: stamp[c] == epoch marks membership, so nothing of size NN is cleared per round except
// the two byte masks that are outputs.
// Per-cell state of a round lives in two words that are ZERO between rounds (the cells a round touched
// are on its lists and are wiped at its end, so nothing of size NN is cleared per round):
//   flag[c]   EF_S reached from a seed (or a seed), EF_SEED, EF_T visited by the todo flood, EF_DONE swept
//   cinfo[c]  the level field (unused after the main sweep) counts the in-edges of c that come from
//             reached cells; bit 31 marks the seeds.  The reach flood increments it once per edge it
//             walks, the sweep decrements it once per edge it has pulled over: a cell is ready when
//             its count returns to zero -- textbook Kahn, but only on the few thousand cells downstream
//             of an edge, and every step of a level is ONE batch of independent loads/atomics.
constexpr uint32_t EF_S = 1u, EF_SEED = 2u, EF_T = 4u, EF_DONE = 8u;
constexpr uint32_t CI_ESEED = 1u << 31, CI_EONE = 1u << CI_LEVEL_SHIFT;
__device__ __forceinline__ uint32_t ci_ecount(uint32_t w) { return (w >> CI_LEVEL_SHIFT) & 0xFFFFu; }

struct EdgeArgs {
    SweepArgs G;             // graph
    uint32_t *flag;          // [NN]
    double *delta;           // [NN] area delta of this round (valid where EF_DONE)
    const uint8_t *flats;
    uint8_t *edge_done;      // output mask
    // perimeter tables, index p: top row (m), bottom row (m), left col rows 1..n-2, right col rows 1..n-2
    uint8_t *p_done, *p_seed;
    double *p_delta;
    int32_t *rlist, *rcount; // reached cells (seeds first): their uca is updated at the end
    int32_t *tlist, *tcount; // cells whose edge_done byte this round cleared
    const int2 *pit_off;     // per cell {first pit in-edge, first pit out-edge} (valid where the graph word says so)
};

__device__ __forceinline__ int64_t perim_index(int i, int j, int n, int m)
{
    if (i == 0) return j;
    if (i == n - 1) return (int64_t)m + j;
    if (j == 0) return 2 * (int64_t)m + (i - 1);
    if (j == m - 1) return 2 * (int64_t)m + (n - 2) + (i - 1);
    return -1;
}

// the inverse of perim_index
__device__ __forceinline__ void perim_cell(int64_t p, int n, int m, int &i, int &j)
{
    if (p < m) { i = 0; j = (int)p; }
    else if (p < 2 * (int64_t)m) { i = n - 1; j = (int)(p - m); }
    else if (p < 2 * (int64_t)m + (n - 2)) { i = (int)(p - 2 * (int64_t)m) + 1; j = 0; }
    else { i = (int)(p - 2 * (int64_t)m - (n - 2)) + 1; j = m - 1; }
}

// the four neighbour strips -> what they say about perimeter cell (i, j): finished somewhere, 'todo' somewhere, and the sum of the
// finished values (:726-739).  dict order of the reference: left, right, top, bottom (the additions are floating point)
__device__ __forceinline__ void strip_fold(const double *__restrict__ sdata, const uint8_t *__restrict__ sdone, const uint8_t *__restrict__ stodo,
                                           int L, int i, int j, int n, int m, bool &dn, bool &td, double &init)
{
    if (j == 0) { dn |= sdone[0 * L + i] != 0; init += sdata[0 * L + i] * (double)(sdone[0 * L + i] != 0); td |= stodo[0 * L + i] != 0; }
    if (j == m - 1) { dn |= sdone[1 * L + i] != 0; init += sdata[1 * L + i] * (double)(sdone[1 * L + i] != 0); td |= stodo[1 * L + i] != 0; }
    if (i == 0) { dn |= sdone[2 * L + j] != 0; init += sdata[2 * L + j] * (double)(sdone[2 * L + j] != 0); td |= stodo[2 * L + j] != 0; }
    if (i == n - 1) { dn |= sdone[3 * L + j] != 0; init += sdata[3 * L + j] * (double)(sdone[3 * L + j] != 0); td |= stodo[3 * L + j] != 0; }
}

// base value of a cell's delta: edge cells initialised from a finished neighbour start from
// (neighbour value - own uca) (:806-809); flats are NaN (:815); everything else 0 (:802)
__device__ __forceinline__ double edge_base(const EdgeArgs &E, int32_t c)
{
    if (E.flats[c]) return NAN;
    const int i = c / E.G.m, j = c - i * E.G.m;
    const int64_t p = perim_index(i, j, E.G.n, E.G.m);
    if (p >= 0 && E.p_done[p]) return E.p_delta[p];
    return 0.0;
}

// one list slot per calling lane, one atomic per wavefront (works in divergent code: the ballot is
// over the lanes that are executing the call)
__device__ __forceinline__ int32_t agg_slot(int32_t *count)
{
    const unsigned long long bal = __ballot(true);
    const int lane = (int)__lane_id();
    const int leader = __ffsll((long long)bal) - 1;
    int32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (int32_t)__popcll(bal));
    base = __shfl(base, leader);
    return base + __popcll(bal & ((1ull << lane) - 1ull));
}

__global__ void k_edge_clear_levels(uint32_t *__restrict__ cinfo, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x)
        cinfo[c] &= CI_STATIC_MASK;
}

// undo the previous round's edge_done = 0 bytes (the mask is rebuilt from all-True every round, :812)
__global__ void k_edge_restore(const int32_t *__restrict__ tlist, int32_t n, uint8_t *__restrict__ edge_done)
{
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) edge_done[tlist[k]] = 1;
}

// strips -> per-perimeter-cell state (:726-739, :798-809); seeds start the reach flood, cells
// that stay 'todo' start the todo flood
__global__ void k_edge_init(EdgeArgs E, const double *__restrict__ sdata, const uint8_t *__restrict__ sdone,
                            const uint8_t *__restrict__ stodo, int L, const double *__restrict__ uca,
                            uint8_t *__restrict__ edge_todo, QE *q_flood, int32_t *n_flood, QE *q_seed, int32_t *n_seed)
{
    const int n = E.G.n, m = E.G.m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nper) return;
    int i, j;
    perim_cell(p, n, m, i, j);
    const int32_t c = i * m + j;
    bool dn = false, td = false;
    double init = 0.0;
    strip_fold(sdata, sdone, stodo, L, i, j, n, m, dn, td, init);
    if (!dn) init = 0.0;                                                         // :738-739
    const bool seed = dn && td;                                                  // :798
    const bool todo_out = td && !dn;                                             // :799
    E.p_done[p] = dn;
    E.p_seed[p] = seed;
    E.p_delta[p] = dn ? init - uca[c] : 0.0;                                     // :806-809
    edge_todo[c] = todo_out;                                                     // returned as edge_todo_i (:817, :862)
    if (todo_out) {
        E.edge_done[c] = 0;
        E.flag[c] = EF_T;
        E.tlist[agg_slot(E.tcount)] = c;
        QE q; q.c = c; q.cw = (E.G.cinfo[c] & CI_STATIC_MASK) | (1u << 31);     // bit 31 of a flood entry: todo flood
        q_flood[agg_slot(n_flood)] = q;
    }
    if (seed) {
        const uint32_t cw = E.G.cinfo[c] & CI_STATIC_MASK;
        E.flag[c] = EF_S | EF_SEED;
        E.G.cinfo[c] = cw | CI_ESEED;
        E.rlist[agg_slot(E.rcount)] = c;
        QE q; q.c = c; q.cw = cw;
        q_flood[agg_slot(n_flood)] = q;
        q.cw = cw | CI_ESEED;                                                    // bit 31 of a sweep entry: seed
        q_seed[agg_slot(n_seed)] = q;
    }
}

// Both floods in one breadth-first loop (entry bit 31: 0 = reach flood from the seeds, 1 = todo flood).
// Reach (:820-825): every edge walked bumps the target's count; the first visitor lists the target and
// expands it next level.  Todo (:848-853): edge_done = False downstream of the cells that stay 'todo'.
template <typename Push>
__device__ __forceinline__ void edge_flood_cell(const EdgeArgs &E, QE q, int32_t *rcount, int32_t *tcount, Push push)
{
    const SweepArgs &A = E.G;
    const int32_t u = q.c;
    const uint32_t cw = q.cw;
    const bool todo = (cw >> 31) != 0;
    const int s = ci_section(cw);
    int32_t pe = 0;
    if (cw & CI_PIT_OUT) pe = E.pit_off[u].y;
    auto visit = [&](int32_t t) {
        const uint32_t ct = A.cinfo[t];
        if (!todo) {
            const uint32_t old = atomicOr(&E.flag[t], EF_S);
            atomicAdd(&A.cinfo[t], CI_EONE);
            if (!(old & EF_S)) {
                E.rlist[agg_slot(rcount)] = t;
                push(t, ct & CI_STATIC_MASK);
            }
        } else {
            const uint32_t old = atomicOr(&E.flag[t], EF_T);
            if (!(old & EF_T)) {
                E.edge_done[t] = 0;                                              // edge_done = ~edge_todo (:856)
                E.tlist[agg_slot(tcount)] = t;
                push(t, (ct & CI_STATIC_MASK) | (1u << 31));
            }
        }
    };
    if (cw & CI_OUT1) visit(u + fe1r(s) * A.m + fe1c(s));
    if (cw & CI_OUT2) visit(u + fe2r(s) * A.m + fe2c(s));
    if (cw & CI_PIT_OUT)
        for (int32_t e = pe; e < A.n_pit && A.pit_src[e] == u; e++) visit(A.pit_dst[e]);
}

// Seeded sweep (drain_area with skip_edge=False on the flooded sub-graph, :836-842).  Seeds keep the
// edge value itself (a done cell on the tile edge never receives, cyutils.pyx:159-161); every other
// cell pulls from its reached upstream cells in the fixed neighbour order.  All loads and the
// count-down atomics on the targets depend only on the queue entry: one memory round trip per level.
template <typename Push>
__device__ __forceinline__ void edge_sweep_cell(const EdgeArgs &E, QE q, Push push)
{
    const SweepArgs &A = E.G;
    const int32_t c = q.c;
    const uint32_t cw = q.cw;
    const int m = A.m;
    const bool seed = (cw & CI_ESEED) != 0;
    // (a workgroup's memory pipeline moves about one scattered access per ns: only the neighbours in the
    // in-mask are fetched -- all in one batch, the uses come later)
    uint32_t f[8]; double dl[8], pr[8];
#pragma unroll
    for (int d = 0; d < 8; d++) {
        f[d] = 0; dl[d] = 0.0; pr[d] = 0.0;
        if (!seed && (cw & (1u << d))) {
            const int32_t u = c + NB_DI[d] * m + NB_DJ[d];
            f[d] = E.flag[u]; dl[d] = E.delta[u]; pr[d] = A.prop[u];
        }
    }
    int2 po = make_int2(0, 0);
    if (cw & (CI_PIT_IN | CI_PIT_OUT)) po = E.pit_off[c];
    const int s = ci_section(cw);
    int32_t t1 = -1, t2 = -1;
    uint32_t o1 = 0, o2 = 0;
    if (cw & CI_OUT1) { t1 = c + fe1r(s) * m + fe1c(s); o1 = atomicSub(&A.cinfo[t1], CI_EONE); }
    if (cw & CI_OUT2) { t2 = c + fe2r(s) * m + fe2c(s); o2 = atomicSub(&A.cinfo[t2], CI_EONE); }
    double acc = edge_base(E, c);
    if (!seed) {
#pragma unroll
        for (int d = 0; d < 8; d++) {
            if ((cw & (1u << d)) && (f[d] & EF_S)) {
                const bool cardinal = (NB_DI[d] == 0) || (NB_DJ[d] == 0);
                acc += dl[d] * (cardinal ? pr[d] : 1 - pr[d]);
            }
        }
        if (cw & CI_PIT_IN)
            for (int32_t e = po.x; e < A.n_pit && A.pin_dst[e] == c; e++)
                if (E.flag[A.pin_src[e]] & EF_S) acc += E.delta[A.pin_src[e]] * A.pin_w[e];
    }
    E.delta[c] = acc;
    atomicOr(&E.flag[c], EF_DONE);
    if (t1 >= 0 && ci_ecount(o1) == 1u && !(o1 & CI_ESEED)) push(t1, o1 & CI_STATIC_MASK);
    if (t2 >= 0 && ci_ecount(o2) == 1u && !(o2 & CI_ESEED)) push(t2, o2 & CI_STATIC_MASK);
    if (cw & CI_PIT_OUT)
        for (int32_t e = po.y; e < A.n_pit && A.pit_src[e] == c; e++) {
            const int32_t t = A.pit_dst[e];
            const uint32_t o = atomicSub(&A.cinfo[t], CI_EONE);
            if (ci_ecount(o) == 1u && !(o & CI_ESEED)) push(t, o & CI_STATIC_MASK);
        }
}

// one level, many workgroups (large frontiers); counters rotate over 3 slots as in the main sweep
template <int WHICH>   // 0 floods, 1 sweep
__global__ __launch_bounds__(256) void k_edge_level(EdgeArgs E, const QE *__restrict__ qc, QE *__restrict__ qn, int32_t *cnt3, int r)
{
    const int32_t nq = cnt3[r % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt3[(r + 2) % 3] = 0;
    if (nq == 0) return;
    int32_t *cn = &cnt3[(r + 1) % 3];
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nq; k += gridDim.x * blockDim.x) {
        auto push = [&](int32_t t, uint32_t ct) { QE e; e.c = t; e.cw = ct; qn[agg_slot(cn)] = e; };
        if (WHICH == 0) edge_flood_cell(E, qc[k], E.rcount, E.tcount, push);
        else edge_sweep_cell(E, qc[k], push);
    }
}

// Small frontiers: ONE workgroup runs level after level without going back to the host (a kernel
// boundary costs a launch plus a trip across the fabric for every first access; the floods and sweeps
// downstream of an edge are hundreds of levels of a few cells).  Stops when the frontier is empty
// or outgrows SMALL_CAP and reports where it stopped.
constexpr int SMALL_CAP = 4096;

template <int WHICH>
__global__ __launch_bounds__(1024) void k_edge_small(EdgeArgs E, QE *q0, QE *q1, int32_t *cnt3, int r_start, int32_t *state)
{
    // the frontier lives in LDS (and is mirrored to the global queues, stores nobody waits for, so that a
    // frontier that outgrows the cap can be handed back); list counters are LDS copies for the same reason
    __shared__ QE s_q[2][SMALL_CAP];
    __shared__ int32_t s_next, s_rcount, s_tcount;
    int r = r_start;
    int32_t nq = cnt3[r % 3];
    if (threadIdx.x == 0) { s_rcount = *E.rcount; s_tcount = *E.tcount; }
    if (nq > 0 && nq <= SMALL_CAP) {
        const QE *qc = (r % 2) ? q1 : q0;
        for (int32_t k = threadIdx.x; k < nq; k += blockDim.x) s_q[r % 2][k] = qc[k];
    }
    __syncthreads();
    while (nq > 0 && nq <= SMALL_CAP) {
        if (threadIdx.x == 0) s_next = 0;
        __syncthreads();
        QE *qn = (r % 2) ? q0 : q1;
        QE *ln = s_q[(r + 1) % 2];
        for (int32_t k = threadIdx.x; k < nq; k += blockDim.x) {
            auto push = [&](int32_t t, uint32_t ct) {
                QE e; e.c = t; e.cw = ct;
                const int32_t slot = agg_slot(&s_next);
                if (slot < SMALL_CAP) ln[slot] = e;
                qn[slot] = e;
            };
            if (WHICH == 0) edge_flood_cell(E, s_q[r % 2][k], &s_rcount, &s_tcount, push);
            else edge_sweep_cell(E, s_q[r % 2][k], push);
        }
        __syncthreads();
        nq = s_next;
        r++;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        cnt3[r % 3] = nq; cnt3[(r + 1) % 3] = 0; cnt3[(r + 2) % 3] = 0;
        *E.rcount = s_rcount; *E.tcount = s_tcount;
        state[0] = r;
    }
}

// pit edge offsets per cell for the edge rounds (the main sweep keeps them in the area slots it is
// about to overwrite; afterwards the contribution array is free and holds them for good)
__global__ void k_pit_offsets(const int32_t *__restrict__ pin_dst, const int32_t *__restrict__ pit_src, int64_t ne, int2 *off)
{
    int32_t *slots = reinterpret_cast<int32_t *>(off);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        if (e == 0 || pin_dst[e - 1] != pin_dst[e]) slots[2 * (int64_t)pin_dst[e]] = (int32_t)e;
        if (e == 0 || pit_src[e - 1] != pit_src[e]) slots[2 * (int64_t)pit_src[e] + 1] = (int32_t)e;
    }
}

// self.uca += area (:769) on the reached cells
__global__ void k_edge_apply(EdgeArgs E, double *__restrict__ uca, const int32_t *nr)
{
    const int32_t n = *nr;
    for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        const int32_t c = E.rlist[q];
        // cells the sweep never reached (cyclic drainage) keep their initial value, like the reference
        uca[c] += (E.flag[c] & EF_DONE) ? E.delta[c] : edge_base(E, c);
    }
}

// ... plus the finished edge cells the flood never reached
__global__ void k_edge_apply_perimeter(EdgeArgs E, double *__restrict__ uca)
{
    const int n = E.G.n, m = E.G.m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nper) return;
    int i, j;
    if (p < m) { i = 0; j = (int)p; }                                            // (perim_cell, spelled out: the generated code of this kernel stays as it was)
    else if (p < 2 * (int64_t)m) { i = n - 1; j = (int)(p - m); }
    else if (p < 2 * (int64_t)m + (n - 2)) { i = (int)(p - 2 * (int64_t)m) + 1; j = 0; }
    else { i = (int)(p - 2 * (int64_t)m - (n - 2)) + 1; j = m - 1; }
    const int32_t c = i * m + j;
    if (E.p_done[p] && !(E.flag[c] & EF_S)) uca[c] += edge_base(E, c);
}

// wipe the per-round state of every cell this round touched
__global__ void k_edge_cleanup(EdgeArgs E, const int32_t *nr, const int32_t *nt)
{
    const int32_t n_r = *nr, n_t = *nt;
    for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n_r + n_t; q += gridDim.x * blockDim.x) {
        const int32_t c = q < n_r ? E.rlist[q] : E.tlist[q - n_r];
        E.flag[c] = 0;
        if (q < n_r) E.G.cinfo[c] &= CI_STATIC_MASK;
    }
}


// ------------------------------------------------------------------------------- K7i
// Incremental edge rounds (the pool schedule of the ProcessManager).  A round of the kind above walks
// everything downstream of its seeds -- whole rivers -- although most of those cells stay downstream of
// another unresolved inlet and are of no use to anybody until that one resolves too; a river that runs along a
// tile border hands a seed across it dozens of times and each hand-over re-walks the rest of the river
// (measured: 247 rounds, 3-7 ms each, for an 8-tile mosaic).  Here the state of the fix-up persists between
// rounds instead:
//   * ND, the cells that are not 'done' (edge_done == 0: downstream of an unresolved inlet), is closed under
//     "downstream of"; the count field of the graph word holds, for every cell, the number of its in-edges
//     that come from ND cells, plus ONE for the outside of the tile while the cell is an unresolved inlet
//     (edge_todo == 1);
//   * a cell is 'done' when its count reaches zero (nothing unresolved is left upstream of it): it then PULLS
//     the deltas of its upstream cells in the fixed neighbour order (deterministic, no floating-point
//     atomics), adds the sum to its area and counts its targets down.  A seed adopts the neighbour's finished
//     value when the strip arrives (it never receives, cyutils.pyx:159-161) and loses its outside edge; it is
//     'done' like any other cell, when its count reaches zero, and only then lets go of its targets;
//   * deltas wait in the FINAL upstream cells (delta[]) until the cell below them becomes final: every cell is
//     processed exactly once in the whole fix-up, and a round only costs the chain of cells it finishes.
// When the fix-up ends, the cells that are still not done (their inlet never resolved) pull what their FINAL
// upstream cells hold (pydem_uca_edge_flush): the reference propagates those partial sums round by round
// (:836-842), the areas agree up to the order of the additions.  'done' / 'todo' masks after every round are
// the reference's: edge_done = not downstream of a remaining 'todo' inlet (:848-856), edge_todo = the inlets
// that stay 'todo' (:817).
constexpr uint32_t EF_FINAL = 16u, EF_NAN = 32u;      // EF_NAN: flooded by a NaN seed (k_einc_nan_flood)

struct IncArgs {
    SweepArgs G;
    uint32_t *flag;          // [NN] EF_FINAL
    double *delta;           // [NN] valid where EF_FINAL
    const uint8_t *flats;
    uint8_t *edge_done, *edge_todo;
    double *uca;
    const int2 *pit_off;
    int set_done;            // 0 in the final flush: the cells stay 'not done'
    int32_t *nanq, *n_nan;   // cells whose seed value is NaN (k_einc_nan_flood)
    uint32_t round16;        // this round's number (mod 2^16, never 0); flag bits 16-31 = round that last seeded the cell
    int32_t *prof;           // -DPYDEM_EINC_PROF: levels / 10 ns ticks by frontier width (<=8, <=64, <=512, more)
};

// once per fix-up: counts of the ND sub-graph
__global__ __launch_bounds__(256) void k_einc_prepare(IncArgs E, int64_t NN)
{
    const SweepArgs &A = E.G;
    for (int64_t c64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c64 < NN; c64 += (int64_t)gridDim.x * blockDim.x) {
        if (E.edge_done[c64]) continue;
        const int32_t u = (int32_t)c64;
        E.delta[u] = 0.0;
        const uint32_t cw = A.cinfo[u];
        const int s = ci_section(cw);
        if (cw & CI_OUT1) atomicAdd(&A.cinfo[u + fe1r(s) * A.m + fe1c(s)], CI_EONE);
        if (cw & CI_OUT2) atomicAdd(&A.cinfo[u + fe2r(s) * A.m + fe2c(s)], CI_EONE);
        if (cw & CI_PIT_OUT)
            for (int32_t e = E.pit_off[u].y; e < A.n_pit && A.pit_src[e] == u; e++) atomicAdd(&A.cinfo[A.pit_dst[e]], CI_EONE);
        if (E.edge_todo[u]) atomicAdd(&A.cinfo[u], CI_EONE);                     // the outside of the tile
    }
}

// strips -> events on the perimeter (:726-739, :798-809).  Queue entries are cells whose count reached zero.
__global__ void k_einc_seed(IncArgs E, const double *__restrict__ sdata, const uint8_t *__restrict__ sdone,
                            const uint8_t *__restrict__ stodo, int L, QE *q, int32_t *nq)
{
    const int n = E.G.n, m = E.G.m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nper) return;
    int i, j;
    perim_cell(p, n, m, i, j);
    const int32_t c = i * m + j;
    bool dn = false, td = false;
    double init = 0.0;
    strip_fold(sdata, sdone, stodo, L, i, j, n, m, dn, td, init);
    const bool own_todo = E.edge_todo[c] != 0;
    const bool own_done = E.edge_done[c] != 0;
    const uint32_t cw = E.G.cinfo[c] & CI_STATIC_MASK;
    if (dn) {
        const double d = E.flats[c] ? NAN : init - E.uca[c];                     // :806-809, :815
        if (!own_done) E.flag[c] = (E.flag[c] & 0xFFFFu) | (E.round16 << 16);     // a seed of this round: upstream values do not enter it
        if (!(E.flag[c] & EF_FINAL) && !own_done) {
            // a seed (:798), or a cell below one of the tile's own unresolved inlets whose neighbour copy is finished:
            // it adopts the finished value (it will not pull) and holds the difference for the cells below it.  It is
            // 'done' -- and lets go of its targets -- once nothing unresolved is left upstream of it inside the tile
            E.uca[c] += d;
            E.delta[c] = d;
            E.flag[c] = (E.flag[c] & (EF_NAN | 0xFFFF0000u)) | EF_FINAL;
            if (d != d) E.nanq[atomicAdd(E.n_nan, 1)] = c;
            E.edge_todo[c] = 0;
            if (own_todo) {
                const uint32_t old = atomicSub(&E.G.cinfo[c], CI_EONE);          // the outside of the tile
                if (ci_ecount(old) == 1u) { QE e; e.c = c; e.cw = cw; q[agg_slot(nq)] = e; }
            }
        } else {
            E.uca[c] += d;                                                      // finished on both sides: re-synchronised
            E.edge_todo[c] = 0;
            if (!own_done) {                                                    // ... or a seed of an earlier round that still waits: the
                E.delta[c] += d;                                                // difference joins what it holds for its targets
                if (d != d) E.nanq[atomicAdd(E.n_nan, 1)] = c;
            }
        }
    } else if (own_todo && !td) {
        // the 'todo' flag was dropped without a value (rule :274 / the mosaic border): the outside edge goes away
        E.edge_todo[c] = 0;
        const uint32_t old = atomicSub(&E.G.cinfo[c], CI_EONE);
        if (ci_ecount(old) == 1u) { QE e; e.c = c; e.cw = cw; q[agg_slot(nq)] = e; }
    }
}

// the final flush: the remaining inlets let go of the outside (their flags stay)
__global__ void k_einc_release_todo(IncArgs E, QE *q, int32_t *nq)
{
    const int n = E.G.n, m = E.G.m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nper) return;
    int i, j;
    perim_cell(p, n, m, i, j);
    const int32_t c = i * m + j;
    if (!E.edge_todo[c] || (E.flag[c] & EF_FINAL)) return;
    const uint32_t old = atomicSub(&E.G.cinfo[c], CI_EONE);
    if (ci_ecount(old) == 1u) { QE e; e.c = c; e.cw = E.G.cinfo[c] & CI_STATIC_MASK; q[agg_slot(nq)] = e; }
}

template <typename Push>
__device__ __forceinline__ void einc_cell(const IncArgs &E, QE q, Push push)
{
    const SweepArgs &A = E.G;
    const int32_t c = q.c;
    const uint32_t cw = q.cw;
    const int m = A.m;
    // every load of the cell in ONE batch (own flag / area, the in-neighbours' flag / delta / proportion): the cascade
    // is a chain of dependent memory round trips and nothing else
    int2 po = make_int2(0, 0);
    if (cw & (CI_PIT_IN | CI_PIT_OUT)) po = E.pit_off[c];
    const uint32_t own_flag = E.flag[c];
    const double own_uca = E.uca[c];
    const bool flat = E.flats[c] != 0;
    uint32_t f[8]; double dl[8], pr[8];
#pragma unroll
    for (int d = 0; d < 8; d++) {
        f[d] = 0; dl[d] = 0.0; pr[d] = 0.0;
        if (cw & (1u << d)) {
            const int32_t u = c + NB_DI[d] * m + NB_DJ[d];
            f[d] = E.flag[u]; dl[d] = E.delta[u]; pr[d] = A.prop[u];
        }
    }
    if (!(own_flag & EF_FINAL)) {                                                // (seeds keep the value they adopted)
        double acc = flat ? NAN : 0.0;                                           // :815
#pragma unroll
        for (int d = 0; d < 8; d++) {
            if ((cw & (1u << d)) && (f[d] & EF_FINAL)) {
                const bool cardinal = (NB_DI[d] == 0) || (NB_DJ[d] == 0);
                acc += dl[d] * (cardinal ? pr[d] : 1 - pr[d]);
            }
        }
        if (cw & CI_PIT_IN)
            for (int32_t e = po.x; e < A.n_pit && A.pin_dst[e] == c; e++)
                if (E.flag[A.pin_src[e]] & EF_FINAL) acc += E.delta[A.pin_src[e]] * A.pin_w[e];
        E.delta[c] = acc;
        E.uca[c] = own_uca + acc;
        E.flag[c] = (own_flag & EF_NAN) | EF_FINAL;
    }
    if (E.set_done) E.edge_done[c] = 1;
    const int s = ci_section(cw);
    auto release = [&](int32_t t) {
        const uint32_t old = atomicSub(&A.cinfo[t], CI_EONE);
        if (ci_ecount(old) == 1u) push(t, old & CI_STATIC_MASK);
    };
    if (cw & CI_OUT1) release(c + fe1r(s) * m + fe1c(s));
    if (cw & CI_OUT2) release(c + fe2r(s) * m + fe2c(s));
    if (cw & CI_PIT_OUT)
        for (int32_t e = po.y; e < A.n_pit && A.pit_src[e] == c; e++) release(A.pit_dst[e]);
}

// NaN is absorbing in the reference's rounds and floods everything below the seed in the round it arrives (see
// k_cinc_nan_flood for the argument); cell-indexed form: breadth first over the out-edges of the graph words
__global__ __launch_bounds__(1024) void k_einc_nan_flood(IncArgs E)
{
    __shared__ int32_t s_tail;
    const SweepArgs &A = E.G;
    if (threadIdx.x == 0) s_tail = *E.n_nan;
    __syncthreads();
    int32_t head = 0, tail = s_tail;
    const int32_t n_origin = tail;             // the NaN seeds themselves
    while (head < tail) {
        for (int32_t q = head + threadIdx.x; q < tail; q += blockDim.x) {
            const int32_t c = E.nanq[q];
            if (q >= n_origin && (E.flag[c] >> 16) == E.round16) continue;       // a seed of this round keeps its value
            if (atomicOr(&E.flag[c], EF_NAN) & EF_NAN) continue;
            E.uca[c] = NAN;
            const uint32_t cw = A.cinfo[c];
            const int s = ci_section(cw);
            auto visit = [&](int32_t t) { if (!(E.flag[t] & EF_NAN)) E.nanq[atomicAdd(&s_tail, 1)] = t; };
            if (cw & CI_OUT1) visit(c + fe1r(s) * A.m + fe1c(s));
            if (cw & CI_OUT2) visit(c + fe2r(s) * A.m + fe2c(s));
            if (cw & CI_PIT_OUT)
                for (int32_t e = E.pit_off[c].y; e < A.n_pit && A.pit_src[e] == c; e++) visit(A.pit_dst[e]);
        }
        __syncthreads();
        head = tail; tail = s_tail;
        __syncthreads();
    }
    if (threadIdx.x == 0) *E.n_nan = 0;
}

__global__ __launch_bounds__(256) void k_einc_level(IncArgs E, const QE *__restrict__ qc, QE *__restrict__ qn, int32_t *cnt3, int r)
{
    const int32_t nq = cnt3[r % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt3[(r + 2) % 3] = 0;
    if (nq == 0) return;
    int32_t *cn = &cnt3[(r + 1) % 3];
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nq; k += gridDim.x * blockDim.x) {
        auto push = [&](int32_t t, uint32_t ct) { QE e; e.c = t; e.cw = ct; qn[agg_slot(cn)] = e; };
        einc_cell(E, qc[k], push);
    }
}

// small frontiers: one workgroup, level after level (see k_edge_small)
__global__ __launch_bounds__(1024) void k_einc_small(IncArgs E, QE *q0, QE *q1, int32_t *cnt3, int r_start, int32_t *state)   // (launched with 64..1024 threads)
{
    __shared__ QE s_q[2][SMALL_CAP];
    __shared__ int32_t s_next;
    int r = r_start;
    int32_t nq = cnt3[r % 3];
    if (nq > 0 && nq <= SMALL_CAP) {
        const QE *qc = (r % 2) ? q1 : q0;
        for (int32_t k = threadIdx.x; k < nq; k += blockDim.x) s_q[r % 2][k] = qc[k];
    }
#ifdef PYDEM_EINC_PROF
    long long prof_t[4] = {0, 0, 0, 0}; int prof_n[4] = {0, 0, 0, 0};
#endif
    __syncthreads();
    while (nq > 0 && nq <= SMALL_CAP) {
#ifdef PYDEM_EINC_PROF
        const long long t0 = wall_clock64();
        const int cls = nq <= 8 ? 0 : (nq <= 64 ? 1 : (nq <= 512 ? 2 : 3));
#endif
        if (threadIdx.x == 0) s_next = 0;
        __syncthreads();
        QE *qn = (r % 2) ? q0 : q1;
        QE *ln = s_q[(r + 1) % 2];
        for (int32_t k = threadIdx.x; k < nq; k += blockDim.x) {
            auto push = [&](int32_t t, uint32_t ct) {
                QE e; e.c = t; e.cw = ct;
                const int32_t slot = agg_slot(&s_next);
                if (slot < SMALL_CAP) ln[slot] = e;
                qn[slot] = e;
            };
            einc_cell(E, s_q[r % 2][k], push);
        }
        __syncthreads();
        nq = s_next;
        r++;
        __syncthreads();
#ifdef PYDEM_EINC_PROF
        prof_t[cls] += wall_clock64() - t0; prof_n[cls]++;
#endif
    }
    if (threadIdx.x == 0) {
        cnt3[r % 3] = nq; cnt3[(r + 1) % 3] = 0; cnt3[(r + 2) % 3] = 0;
        state[0] = r;
#ifdef PYDEM_EINC_PROF
        for (int k = 0; k < 4; k++) { atomicAdd(&E.prof[k], prof_n[k]); atomicAdd(&E.prof[4 + k], (int)prof_t[k]); }
#endif
    }
}


// ---- compact form of the incremental rounds ----------------------------------------------------------------
// The cascade above is a chain of dependent accesses into seven tile-sized arrays: a level costs 5-7 us, most of
// it address translation and HBM misses (measured: 35 k levels = 230 ms for an 8-tile fix-up at 16384^2) although
// the cells it will ever touch -- ND, 50-70 k per tile -- would fit the L2.  So the fix-up state moves into ONE
// 128-byte record per ND cell (compact id k: the cell, its graph word, the compact ids and weights of its
// in-edges, the ids of its two targets, count, flags, delta); a finished cell writes its contribution into its
// targets' in-slots (plain stores, one slot per edge: the sum stays in the fixed neighbour order) and counts them
// down, so a cell that becomes ready needs nothing but its own record -- ONE dependent access per level plus the
// count-down atomics.  The cascade runs on records only, and the
// areas / masks of the tile are updated from the records by a streaming kernel after the cascade (nothing in the
// chain waits for the big arrays).  Tiles whose ND set is too large for that (a tile that is one single
// catchment below its inlet edge) keep the cell-indexed form.
struct __attribute__((aligned(128))) NDRec {
    int32_t cell;
    uint32_t cw;
    int32_t out_id[2];       // compact ids of the two targets (-1: no such edge)
    uint8_t out_slot[2];     // which in-slot of the target this cell feeds (the target's neighbour index NW..SE)
    uint16_t seed_round;     // round (mod 2^16) in which the strips last initialised the cell: a NaN flood of that round stops here
    int32_t cnt;             // unresolved in-edges (+1 for the outside of the tile while the cell is a 'todo' inlet)
    uint32_t flag;
    int32_t wid;             // condensed form (uca_cond.inl): node of a watched cell, -1 otherwise
    double delta;
    double out_w[2];         // proportion, 1 - proportion (:1082)
    double in_delta[8];      // what the finished in-neighbour NW..SE has handed over (0 until then)
};
static_assert(sizeof(NDRec) == 128, "one cache line per ND cell");
constexpr uint32_t NF_FINAL = 1u, NF_DONE = 2u, NF_APPLIED = 4u, NF_SEED = 8u, NF_NAN = 16u;
constexpr uint32_t ND_FLAT = 1u << 16;            // in the record's graph word: the cell is a flat (its delta is NaN, :815)
constexpr int64_t ND_COMPACT_MAX = 6 << 20;      // records (768 MiB)

struct CIncArgs {
    SweepArgs G;
    NDRec *rec; int32_t nd;
    int32_t *cid;            // [NN] compact id + 1 (0: not an ND cell)
    const int2 *pit_off;
    const uint8_t *flats;
    uint8_t *edge_done, *edge_todo;
    double *uca;
    int set_done;
    int32_t *prof;
    int32_t *nanq, *n_nan;   // records whose delta is NaN (k_cinc_nan_flood)
    uint32_t round16;        // this round's number (mod 2^16, never 0)
};

// bytes of a 32-bit word that are zero, exactly (0x80 per zero byte)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x)
{
    const uint32_t y = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(y | x | 0x7F7F7F7Fu);
}

// (both kernels read the mask sixteen cells per load: the not-done cells are ~0.1 % of a tile, and one byte per thread made these
// two passes over a 268 MB plane 0.43 + 0.69 ms of a round-1 fix-up -- round 6)
__global__ __launch_bounds__(256) void k_nd_count(const uint8_t *__restrict__ edge_done, int64_t NN, unsigned long long *count)
{
    unsigned long long c = 0;
    const int64_t n16 = NN / 16;
    const uint4 *v = reinterpret_cast<const uint4 *>(edge_done);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 x = v[i];
        c += __popc(zero_bytes(x.x)) + __popc(zero_bytes(x.y)) + __popc(zero_bytes(x.z)) + __popc(zero_bytes(x.w));
    }
    if (blockIdx.x == 0) for (int64_t i = n16 * 16 + threadIdx.x; i < NN; i += blockDim.x) c += edge_done[i] == 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

__device__ __forceinline__ void nd_assign_cell(const CIncArgs &E, int64_t c64, int32_t k)
{
    E.cid[c64] = k + 1;
    NDRec &R = E.rec[k];
    R.cell = (int32_t)c64;
    R.cw = (E.G.cinfo[c64] & CI_STATIC_MASK) | (E.flats[c64] ? ND_FLAT : 0u);
    R.flag = 0; R.delta = 0.0; R.seed_round = 0; R.wid = -1;
}

__global__ __launch_bounds__(256) void k_nd_assign(CIncArgs E, int64_t NN, int32_t *counter)
{
    const int64_t n16 = NN / 16;
    const uint4 *v = reinterpret_cast<const uint4 *>(E.edge_done);
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n16; i0 += (int64_t)gridDim.x * blockDim.x) {      // (uniform per workgroup)
        const int64_t i = i0 + threadIdx.x;
        const uint4 x = i < n16 ? v[i] : make_uint4(~0u, ~0u, ~0u, ~0u);
        const uint32_t w[4] = {zero_bytes(x.x), zero_bytes(x.y), zero_bytes(x.z), zero_bytes(x.w)};
        const int nz = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
        if (__ballot(nz > 0) == 0) continue;                           // (almost always: nothing to do for these 1024 cells)
        // record ids for the wavefront's cells with ONE atomic: inclusive scan of the counts over the lanes
        int incl = nz;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        int32_t base = 0;
        if (lane == 63) base = atomicAdd(counter, incl);
        int32_t k = __shfl(base, 63) + incl - nz;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t z = w[q];
            while (z) { const int b = __ffs((int)z) - 1; z &= z - 1; nd_assign_cell(E, i * 16 + q * 4 + (b >> 3), k++); }
        }
    }
    if (blockIdx.x == 0) for (int64_t c64 = n16 * 16 + threadIdx.x; c64 < NN; c64 += blockDim.x) if (!E.edge_done[c64]) nd_assign_cell(E, c64, atomicAdd(counter, 1));
}

__global__ __launch_bounds__(256) void k_nd_link(CIncArgs E)
{
    const SweepArgs &A = E.G;
    const int m = A.m;
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                   // the sink of the missing edges
        NDRec &S = E.rec[E.nd];
        S.cell = -1; S.cw = 0; S.out_id[0] = S.out_id[1] = -1; S.out_slot[0] = S.out_slot[1] = 0; S.cnt = 1 << 30; S.flag = 0; S.delta = 0.0; S.wid = -1;
    }
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < E.nd; k += gridDim.x * blockDim.x) {
        NDRec &R = E.rec[k];
        const int32_t c = R.cell;
        const uint32_t cw = R.cw;
        int32_t cnt = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            if (cw & (1u << d)) cnt += E.cid[c + NB_DI[d] * m + NB_DJ[d]] != 0;
            R.in_delta[d] = 0.0;
        }
        if (cw & CI_PIT_IN)
            for (int32_t e = E.pit_off[c].x; e < A.n_pit && A.pin_dst[e] == c; e++) cnt += E.cid[A.pin_src[e]] != 0;
        const int s = ci_section(cw);
        const double p = A.prop[c];
        const int dr[2] = {fe1r(s), fe2r(s)}, dc[2] = {fe1c(s), fe2c(s)};
        const uint32_t has[2] = {cw & CI_OUT1, cw & CI_OUT2};
        for (int j = 0; j < 2; j++) {
            int32_t id = -1; int slot = 0;
            if (has[j]) {
                id = E.cid[c + dr[j] * m + dc[j]] - 1;
                // seen from the target, this cell sits at (-dr, -dc): its index in the neighbour order NW..SE
                for (int d = 0; d < 8; d++) if (NB_DI[d] == -dr[j] && NB_DJ[d] == -dc[j]) slot = d;
            }
            R.out_id[j] = id; R.out_slot[j] = (uint8_t)slot;
        }
        R.out_w[0] = p; R.out_w[1] = 1 - p;
        if (E.edge_todo[c]) cnt += 1;                                            // the outside of the tile
        R.cnt = cnt;
    }
}

__global__ void k_cinc_seed(CIncArgs E, const double *__restrict__ sdata, const uint8_t *__restrict__ sdone,
                            const uint8_t *__restrict__ stodo, int L, QE *q, int32_t *nq)
{
    const int n = E.G.n, m = E.G.m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nper) return;
    int i, j;
    perim_cell(p, n, m, i, j);
    const int32_t c = i * m + j;
    bool dn = false, td = false;
    double init = 0.0;
    strip_fold(sdata, sdone, stodo, L, i, j, n, m, dn, td, init);
    const bool own_todo = E.edge_todo[c] != 0;
    const bool own_done = E.edge_done[c] != 0;
    const int32_t k = E.cid[c] - 1;
    if (dn) {
        const double d = E.flats[c] ? NAN : init - E.uca[c];
        E.uca[c] += d;
        E.edge_todo[c] = 0;
        if (k >= 0 && !own_done) E.rec[k].seed_round = (uint16_t)E.round16;     // a seed of this round (:798): upstream values do not enter it
        if (k >= 0 && !own_done && !(E.rec[k].flag & NF_FINAL)) {
            NDRec &R = E.rec[k];
            R.delta = d;
            R.flag = (R.flag & NF_NAN) | NF_FINAL | NF_SEED;
            if (d != d) E.nanq[atomicAdd(E.n_nan, 1)] = k;                       // (k_cinc_nan_flood)
            if (own_todo) {
                const int32_t old = atomicSub(&R.cnt, 1);
                if (old == 1) { QE e; e.c = k; e.cw = 0; q[agg_slot(nq)] = e; }
            }
        } else if (k >= 0 && !own_done) {
            // a seed of an earlier round that still waits for its own upstream cells, and the neighbour's copy has moved
            // on since: the reference re-initialises it in every round (`area_edges - uca`, :806-809) and lets the
            // difference run down; here it joins what the cell holds for its targets
            E.rec[k].delta += d;
            if (d != d) E.nanq[atomicAdd(E.n_nan, 1)] = k;
        }
    } else if (own_todo && !td) {
        E.edge_todo[c] = 0;
        if (k >= 0) {
            const int32_t old = atomicSub(&E.rec[k].cnt, 1);
            if (old == 1) { QE e; e.c = k; e.cw = 0; q[agg_slot(nq)] = e; }
        }
    }
}

__global__ void k_cinc_release_todo(CIncArgs E, QE *q, int32_t *nq)
{
    const int n = E.G.n, m = E.G.m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nper) return;
    int i, j;
    perim_cell(p, n, m, i, j);
    const int32_t c = i * m + j;
    const int32_t k = E.cid[c] - 1;
    if (k < 0 || !E.edge_todo[c] || (E.rec[k].flag & NF_FINAL)) return;
    const int32_t old = atomicSub(&E.rec[k].cnt, 1);
    if (old == 1) { QE e; e.c = k; e.cw = 0; q[agg_slot(nq)] = e; }
}

template <typename Push>
__device__ __forceinline__ void cinc_cell(const CIncArgs &E, QE q, Push push)
{
    // (letting the lane walk on along the chain it releases -- one count-down atomic plus one record load per step, no
    // queue, no barrier -- was measured and is slower: 323 instead of 209 ms of rounds for the 8-tile fix-up at
    // 16384^2; the side branches a walking lane pushes wait for the whole walk)
    const int32_t k = q.c;
    NDRec &R = E.rec[k];
    // the only dependent access of a level: the cell's own record, one cache line, loaded whole
    const uint4 *line = reinterpret_cast<const uint4 *>(&R);
    uint4 L[8];
#pragma unroll
    for (int i = 0; i < 8; i++) L[i] = line[i];
    NDRec V;
    __builtin_memcpy(&V, L, sizeof(V));
    const uint32_t cw = V.cw;
    double delta = V.delta;
    if (!(V.flag & NF_FINAL)) {
        double acc = (cw & ND_FLAT) ? NAN : 0.0;                                 // :815
#pragma unroll
        for (int d = 0; d < 8; d++) acc += V.in_delta[d];                        // fixed order NW..SE; untouched slots are 0
        if (cw & CI_PIT_IN) {
            // (fetching the pits eight at a time -- list entries, record ids, records each together -- was measured in round 6 and is
            // slower: most drains have one or two pits, and the flush went from 6.2-7.6 to 6.7-8.3 ms per tile)
            const SweepArgs &A = E.G;
            for (int32_t e = E.pit_off[V.cell].x; e < A.n_pit && A.pin_dst[e] == V.cell; e++) {
                const int32_t ks = E.cid[A.pin_src[e]] - 1;
                if (ks >= 0 && (E.rec[ks].flag & NF_FINAL)) acc += E.rec[ks].delta * A.pin_w[e];
            }
        }
        delta = acc;
        R.delta = acc;
        R.flag = (V.flag & NF_NAN) | NF_FINAL | NF_DONE;
    } else {
        R.flag = V.flag | NF_DONE;                                               // a seed keeps the value it adopted
    }
    // hand the contribution over, then count the targets down.  A missing edge points at the sink record rec[nd]
    // (its count never reaches zero), so both stores and both atomics are issued unconditionally, back to back
    const int32_t o0 = V.out_id[0] >= 0 ? V.out_id[0] : E.nd, o1 = V.out_id[1] >= 0 ? V.out_id[1] : E.nd;
    E.rec[o0].in_delta[V.out_slot[0]] = delta * V.out_w[0];
    E.rec[o1].in_delta[V.out_slot[1]] = delta * V.out_w[1];
    const int32_t old0 = atomicSub(&E.rec[o0].cnt, 1);
    const int32_t old1 = atomicSub(&E.rec[o1].cnt, 1);
    if (old0 == 1) push(o0, 0u);
    if (old1 == 1) push(o1, 0u);
    if (cw & CI_PIT_OUT) {
        const SweepArgs &A = E.G;
        for (int32_t e = E.pit_off[V.cell].y; e < A.n_pit && A.pit_src[e] == V.cell; e++) {
            const int32_t kt = E.cid[A.pit_dst[e]] - 1;
            if (kt >= 0 && atomicSub(&E.rec[kt].cnt, 1) == 1) push(kt, 0u);
        }
    }
}

// A round of the reference propagates whatever a seed carries through ALL cells below it at once (:826-840), and NaN is
// absorbing there: a cell that received NaN in one round stays NaN when a later round re-initialises it from a finished
// neighbour (`area_edges - uca`, :806-809).  The incremental rounds hold deltas back until a cell's last upstream cell is
// done, and a cell that adopts a neighbour's value in the meantime drops them -- harmless for numbers (the adopted value
// contains them), wrong for NaN.  So a NaN seed floods its NaN through everything downstream in the round it arrives --
// except the other seeds of that round, which are 'done' from the start in the reference's sweep and take nothing from
// upstream (:826-829): one workgroup, breadth first over the out-links of the records, each record claimed once.
__global__ __launch_bounds__(1024) void k_cinc_nan_flood(CIncArgs E)
{
    __shared__ int32_t s_tail;
    if (threadIdx.x == 0) s_tail = *E.n_nan;
    __syncthreads();
    int32_t head = 0, tail = s_tail;
    const int32_t n_origin = tail;             // the NaN seeds themselves
    while (head < tail) {
        for (int32_t q = head + threadIdx.x; q < tail; q += blockDim.x) {
            const int32_t k = E.nanq[q];
            NDRec &R = E.rec[k];
            if (q >= n_origin && R.seed_round == (uint16_t)E.round16) continue;  // a seed of this round keeps its value
            if (atomicOr(&R.flag, NF_NAN) & NF_NAN) continue;                     // flooded in an earlier round
            E.uca[R.cell] = NAN;
            for (int o = 0; o < 2; o++) {
                const int32_t t = R.out_id[o];
                if (t >= 0 && !(E.rec[t].flag & NF_NAN)) E.nanq[atomicAdd(&s_tail, 1)] = t;
            }
            if (R.cw & CI_PIT_OUT) {
                const SweepArgs &A = E.G;
                for (int32_t e = E.pit_off[R.cell].y; e < A.n_pit && A.pit_src[e] == R.cell; e++) {
                    const int32_t t = E.cid[A.pit_dst[e]] - 1;
                    if (t >= 0 && !(E.rec[t].flag & NF_NAN)) E.nanq[atomicAdd(&s_tail, 1)] = t;
                }
            }
        }
        __syncthreads();
        head = tail; tail = s_tail;
        __syncthreads();
    }
    if (threadIdx.x == 0) *E.n_nan = 0;
}

__global__ __launch_bounds__(256) void k_cinc_level(CIncArgs E, const QE *__restrict__ qc, QE *__restrict__ qn, int32_t *cnt3, int r)
{
    const int32_t nq = cnt3[r % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt3[(r + 2) % 3] = 0;
    if (nq == 0) return;
    int32_t *cn = &cnt3[(r + 1) % 3];
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nq; k += gridDim.x * blockDim.x) {
        auto push = [&](int32_t t, uint32_t ct) { QE e; e.c = t; e.cw = ct; qn[agg_slot(cn)] = e; };
        cinc_cell(E, qc[k], push);
    }
}

__global__ __launch_bounds__(1024) void k_cinc_small(CIncArgs E, QE *q0, QE *q1, int32_t *cnt3, int r_start, int32_t *state, int cap)
{
    __shared__ QE s_q[2][SMALL_CAP];
    __shared__ int32_t s_cnt[3];     // pushes of level r go to s_cnt[(r + 1) % 3]; s_cnt[(r + 2) % 3] is zeroed meanwhile: ONE barrier per level
    int r = r_start;
    int32_t nq = cnt3[r % 3];
    if (nq > 0 && nq <= cap) {
        const QE *qc = (r % 2) ? q1 : q0;
        for (int32_t k = threadIdx.x; k < nq; k += blockDim.x) s_q[r % 2][k] = qc[k];
    }
    if (threadIdx.x == 0) { s_cnt[0] = s_cnt[1] = s_cnt[2] = 0; }
#ifdef PYDEM_EINC_PROF
    long long prof_t[4] = {0, 0, 0, 0}; int prof_n[4] = {0, 0, 0, 0};
#endif
    __syncthreads();
    while (nq > 0 && nq <= cap) {
#ifdef PYDEM_EINC_PROF
        const long long t0 = wall_clock64();
        const int cls = nq <= 8 ? 0 : (nq <= 64 ? 1 : (nq <= 512 ? 2 : 3));
#endif
        int32_t *cn = &s_cnt[(r + 1) % 3];
        if (threadIdx.x == 0) s_cnt[(r + 2) % 3] = 0;
        QE *qn = (r % 2) ? q0 : q1;
        QE *ln = s_q[(r + 1) % 2];
        for (int32_t k = threadIdx.x; k < nq; k += blockDim.x) {
            auto push = [&](int32_t t, uint32_t ct) {
                QE e; e.c = t; e.cw = ct;
                const int32_t slot = agg_slot(cn);
                if (slot < SMALL_CAP) ln[slot] = e;
                else qn[slot] = e;                           // beyond the LDS queue: straight to the global one
            };
            cinc_cell(E, s_q[r % 2][k], push);
        }
        __syncthreads();
        nq = *cn;
        r++;
#ifdef PYDEM_EINC_PROF
        prof_t[cls] += wall_clock64() - t0; prof_n[cls]++;
#endif
    }
    if (nq > cap && r > r_start) {
        // the frontier outgrew the workgroup: the level kernels take over from the global queue, whose head is still in LDS
        QE *qg = (r % 2) ? q1 : q0;
        for (int32_t k = threadIdx.x; k < SMALL_CAP; k += blockDim.x) qg[k] = s_q[r % 2][k];
    }
    if (threadIdx.x == 0) {
        cnt3[r % 3] = nq; cnt3[(r + 1) % 3] = 0; cnt3[(r + 2) % 3] = 0;
        state[0] = r;
#ifdef PYDEM_EINC_PROF
        for (int k = 0; k < 4; k++) { atomicAdd(&E.prof[k], prof_n[k]); atomicAdd(&E.prof[4 + k], (int)prof_t[k]); }
#endif
    }
}

// records -> tile: areas and masks of the cells the last cascade finished
__global__ __launch_bounds__(256) void k_cinc_apply(CIncArgs E)
{
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < E.nd; k += gridDim.x * blockDim.x) {
        NDRec &R = E.rec[k];
        const uint32_t f = R.flag;
        if ((f & NF_DONE) && !(f & NF_APPLIED)) {
            if (!(f & NF_SEED)) E.uca[R.cell] += R.delta;                       // (a seed took its value when the strip arrived)
            if (E.set_done) E.edge_done[R.cell] = 1;
            R.flag = f | NF_APPLIED;
        }
    }
}


#include "uca_cond.inl"
#include "uca_cbuild.inl"

}  // namespace

static double host_now_ms()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// The wide levels of a cascade: while the frontier of level r (queue[r % 2], counters[CS_FRONTIER + r % 3]) is wider than `cap`,
// batches of level kernels over the chip -- launch(lv, grid) starts the kernel of level lv -- with ONE look of the host per batch.
// r and last (the width of level r) are those of the first level on entry and of the first level left to the caller on return.
template <typename Launch>
static int edge_wide_levels(pydem_tile *t, int32_t cap, int &r, int32_t &last, Launch launch)
{
    while (last > cap) {
        const int batch = last > 65536 ? 4 : 16;
        const int grid = grid_for(last, 1024);
        for (int b = 0; b < batch; b++, r++) launch(r, grid);
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        last = t->h_counters[CS_FRONTIER + r % 3];
        if (r > (1 << 24)) { pydem_set_error("edge update: flow paths too long"); return -5; }
    }
    return 0;
}

// What PYDEM_EDGE_DEBUG reports of a cascade (host counters around the launches): its levels, how many of them the level
// kernels ran (a batch that overshoots an emptied frontier included) and how often it passed between the one-workgroup
// kernel and the level kernels with levels run on both sides.
struct CascadeDbg {
    int levels = 0, wide = 0, handovers = 0;
    int prev = -1;                  // who ran the levels before: 0 the one-workgroup kernel, 1 the level kernels
    void ran(int kind, int from, int to)
    {
        if (to <= from) return;
        if (prev >= 0 && prev != kind) handovers++;
        if (kind == 1) wide += to - from;
        prev = kind; levels = to;
    }
};

int stage_edge_update(pydem_tile *t, const pydem_options *opt, const double *const data[4], const uint8_t *const done[4],
                      const uint8_t *const todo[4])
{
    (void)opt;
    if (t->einc_ready) PYDEM_TRY(stage_edge_flush(t));      // incremental rounds left deltas waiting: settle them first
    const double t_begin = host_now_ms();
    const int n = (int)t->n, m = (int)t->m;
    PYDEM_TRY(tile_alloc(t, &t->row_area, (size_t)t->n));
    const int L = n > m ? n : m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    PYDEM_TRY(tile_alloc(t, &t->estamp, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->edelta, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->labels, (size_t)t->NN));        // rlist
    PYDEM_TRY(tile_alloc(t, &t->flatlist, (size_t)t->NN));      // tlist (kept until the next round restores the mask)
    PYDEM_TRY(tile_alloc(t, &t->queue[0], (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->queue[1], (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->eseed, (size_t)(nper > 0 ? nper : 1) * 2));
    PYDEM_TRY(tile_alloc(t, &t->p_delta, (size_t)nper));
    PYDEM_TRY(tile_alloc(t, &t->p_flags, (size_t)nper * 2));
    PYDEM_TRY(tile_alloc(t, &t->s_data, (size_t)L * 4));
    PYDEM_TRY(tile_alloc(t, &t->s_flags, (size_t)L * 8));
    EdgeArgs E;
    SweepArgs &A = E.G;
    fill_sweep_args(t, A);
    E.flag = (uint32_t *)t->estamp; E.delta = t->edelta; E.flats = t->flats; E.edge_done = t->edge_done;
    E.p_done = t->p_flags; E.p_seed = t->p_flags + nper; E.p_delta = t->p_delta;
    E.rlist = t->labels; E.rcount = t->counters + CS_EDGE_REACHED;
    E.tlist = t->flatlist; E.tcount = t->counters + CS_EDGE_CLEARED;
    // int2 per cell = half of a double2 slot: the offsets use the first NN * 8 bytes of the contribution array
    PYDEM_TRY(tile_alloc(t, &t->contrib, (size_t)t->NN * 2));
    E.pit_off = reinterpret_cast<const int2 *>(t->contrib);
    if (!t->edge_clean) {
        if (A.n_pit > 0)
            hipLaunchKernelGGL(k_pit_offsets, dim3(grid_for(A.n_pit, 2048)), dim3(256), 0, t->stream, A.pin_dst, A.pit_src, A.n_pit,
                               reinterpret_cast<int2 *>(t->contrib));
        // first round after the graph was (re)built: flags and counts to zero, masks to their defaults (:812, :817)
        HIP_TRY(hipMemsetAsync(t->estamp, 0, (size_t)t->NN * 4, t->stream));
        hipLaunchKernelGGL(k_edge_clear_levels, dim3(grid_for(t->NN, 8192)), dim3(256), 0, t->stream, A.cinfo, t->NN);
        HIP_TRY(hipMemsetAsync(t->edge_todo, 0, (size_t)t->NN, t->stream));
        HIP_TRY(hipMemsetAsync(t->edge_done, 1, (size_t)t->NN, t->stream));
        t->edge_clean = true;
    } else if (t->etodo_prev > 0) {
        hipLaunchKernelGGL(k_edge_restore, dim3(grid_for(t->etodo_prev, 1024)), dim3(256), 0, t->stream, t->flatlist, t->etodo_prev,
                           t->edge_done);
    }
    // strips -> device (left, right, top, bottom), padded to L entries each (data == NULL: they are there already, written
    // by the edge board)
    if (data) {
        // (pinned staging like the incremental rounds: asynchronous copies from pageable memory make the runtime pin and unpin pages
        // behind the caller's back, and the next GPU call waits for that)
        if (t->h_strip_cap < (size_t)L) {
            if (t->h_strip_d) { (void)hipHostFree(t->h_strip_d); (void)hipHostFree(t->h_strip_f); }
            HIP_TRY(hipHostMalloc((void **)&t->h_strip_d, (size_t)L * 4 * sizeof(double)));
            HIP_TRY(hipHostMalloc((void **)&t->h_strip_f, (size_t)L * 8));
            t->h_strip_cap = (size_t)L;
        }
        double *hd = t->h_strip_d;
        uint8_t *hf = t->h_strip_f;
        memset(hd, 0, (size_t)L * 4 * sizeof(double));
        memset(hf, 0, (size_t)L * 8);
        for (int s = 0; s < 4; s++) {
            const int len = s < 2 ? n : m;
            for (int k = 0; k < len; k++) {
                hd[(size_t)s * L + k] = data[s][k];
                hf[(size_t)s * L + k] = done[s][k] != 0;
                hf[(size_t)(4 + s) * L + k] = todo[s][k] != 0;
            }
        }
        HIP_TRY(hipMemcpyAsync(t->s_data, hd, (size_t)L * 4 * 8, hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipMemcpyAsync(t->s_flags, hf, (size_t)L * 8, hipMemcpyHostToDevice, t->stream));
    }
    HIP_TRY(hipMemsetAsync(t->counters, 0, CS_WINDOW * sizeof(int32_t), t->stream));
    int32_t *cnt3 = t->counters + CS_FRONTIER;      // rotating frontier sizes; level r reads queue[r % 2] / cnt3[r % 3]
    int32_t *n_seed = t->counters + CS_EDGE_SEEDS;
    QE *q0 = (QE *)t->queue[0], *q1 = (QE *)t->queue[1];
    hipLaunchKernelGGL(k_edge_init, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, E, t->s_data, t->s_flags,
                       t->s_flags + (size_t)4 * L, L, t->uca, t->edge_todo, q0, &cnt3[0], (QE *)t->eseed, n_seed);
    HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    const int32_t nflood = t->h_counters[CS_FRONTIER], nseed = t->h_counters[CS_EDGE_SEEDS];
    CascadeDbg dbg[2];
    auto run_levels = [&](int which, int32_t first) -> int {
        // which: 0 floods, 1 seeded sweep.  The frontier of level 0 is in queue[0] / cnt3[0].
        int r = 0;
        int32_t last = first;
        int32_t *state = t->counters + CS_CASCADE_STATE;
        static int small_cap = -1;
        if (small_cap < 0) { const char *e = getenv("PYDEM_EDGE_SMALL_CAP"); small_cap = e ? atoi(e) : SMALL_CAP; if (small_cap > SMALL_CAP) small_cap = SMALL_CAP; }
        while (last > 0) {
            if (last <= small_cap) {
                if (which == 0) hipLaunchKernelGGL(k_edge_small<0>, dim3(1), dim3(1024), 0, t->stream, E, q0, q1, cnt3, r, state);
                else hipLaunchKernelGGL(k_edge_small<1>, dim3(1), dim3(1024), 0, t->stream, E, q0, q1, cnt3, r, state);
                HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
                HIP_TRY(hipStreamSynchronize(t->stream));
                const int r0 = r;
                r = t->h_counters[CS_CASCADE_STATE];
                last = t->h_counters[CS_FRONTIER + r % 3];
                dbg[which].ran(0, r0, r);
                continue;
            }
            const int r0 = r;
            PYDEM_TRY(edge_wide_levels(t, std::max(small_cap, 0), r, last, [&](int lv, int grid) {
                if (which == 0) hipLaunchKernelGGL(k_edge_level<0>, dim3(grid), dim3(256), 0, t->stream, E, (lv % 2) ? q1 : q0, (lv % 2) ? q0 : q1, cnt3, lv);
                else hipLaunchKernelGGL(k_edge_level<1>, dim3(grid), dim3(256), 0, t->stream, E, (lv % 2) ? q1 : q0, (lv % 2) ? q0 : q1, cnt3, lv);
            }));
            dbg[which].ran(1, r0, r);
        }
        return 0;
    };
    if (nflood > 0) PYDEM_TRY(run_levels(0, nflood));
    if (nseed > 0) {
        int32_t three[3] = {nseed, 0, 0};
        HIP_TRY(hipMemcpyAsync(q0, t->eseed, (size_t)nseed * sizeof(QE), hipMemcpyDeviceToDevice, t->stream));
        HIP_TRY(hipMemcpyAsync(cnt3, three, sizeof(three), hipMemcpyHostToDevice, t->stream));
        PYDEM_TRY(run_levels(1, nseed));
        hipLaunchKernelGGL(k_edge_apply, dim3(grid_for(t->NN < (1 << 20) ? t->NN : (1 << 20), 1024)), dim3(256), 0, t->stream, E, t->uca,
                           E.rcount);
    }
    hipLaunchKernelGGL(k_edge_apply_perimeter, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, E, t->uca);
    hipLaunchKernelGGL(k_edge_cleanup, dim3(256), dim3(256), 0, t->stream, E, (const int32_t *)E.rcount, (const int32_t *)E.tcount);
    HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    t->etodo_prev = t->h_counters[CS_EDGE_CLEARED];
    if (getenv("PYDEM_EDGE_DEBUG"))
        fprintf(stderr, "edge round: %d seeds, %d todo cells, %d cells reached; levels: floods %d (%d wide), sweep %d (%d wide); hand-overs %d + %d; %.3f ms\n",
                nseed, t->h_counters[CS_EDGE_CLEARED], t->h_counters[CS_EDGE_REACHED], dbg[0].levels, dbg[0].wide, dbg[1].levels, dbg[1].wide,
                dbg[0].handovers, dbg[1].handovers, host_now_ms() - t_begin);
    return 0;
}

// ---- incremental edge rounds: host side ----------------------------------------------------------------
static int einc_args(pydem_tile *t, IncArgs &E)
{
    PYDEM_TRY(tile_alloc(t, &t->row_area, (size_t)t->n));
    PYDEM_TRY(tile_alloc(t, &t->estamp, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->edelta, (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->queue[0], (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->queue[1], (size_t)t->NN));
    PYDEM_TRY(tile_alloc(t, &t->contrib, (size_t)t->NN * 2));
    fill_sweep_args(t, E.G);
    E.flag = (uint32_t *)t->estamp; E.delta = t->edelta; E.flats = t->flats; E.edge_done = t->edge_done; E.edge_todo = t->edge_todo;
    E.uca = t->uca; E.pit_off = reinterpret_cast<const int2 *>(t->contrib); E.set_done = 1;
    E.prof = t->counters + CS_EINC_PROF;
    E.nanq = reinterpret_cast<int32_t *>(t->queue[1]); E.n_nan = t->counters + CS_NAN_SEEDS;   // (queue 1 is empty until the cascade's first level)
    E.round16 = (uint32_t)(t->einc_round % 65535) + 1u;
    return 0;
}

// run the cascade whose first frontier is in queue[0] / counters[CS_FRONTIER]; ONE host synchronisation when the frontier stays small
static int einc_cascade(pydem_tile *t, const IncArgs &E, CascadeDbg *dbg)
{
    int32_t *cnt3 = t->counters + CS_FRONTIER;
    int32_t *state = t->counters + CS_CASCADE_STATE;
    QE *q0 = (QE *)t->queue[0], *q1 = (QE *)t->queue[1];
    int r = 0;
    for (;;) {
        static int einc_block = -1;
        if (einc_block < 0) { const char *e = getenv("PYDEM_EINC_BLOCK"); einc_block = e ? atoi(e) : 1024; }
        hipLaunchKernelGGL(k_einc_small, dim3(1), dim3(einc_block), 0, t->stream, E, q0, q1, cnt3, r, state);
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        const int r_small = r;
        r = t->h_counters[CS_CASCADE_STATE];
        if (dbg) dbg->ran(0, r_small, r);
        int32_t last = t->h_counters[CS_FRONTIER + r % 3];
        if (last == 0) break;
        // the frontier outgrew one workgroup: level kernels until it is small again
        const int r_wide = r;
        PYDEM_TRY(edge_wide_levels(t, SMALL_CAP, r, last, [&](int lv, int grid) {
            hipLaunchKernelGGL(k_einc_level, dim3(grid), dim3(256), 0, t->stream, E, (lv % 2) ? q1 : q0, (lv % 2) ? q0 : q1, cnt3, lv);
        }));
        if (dbg) dbg->ran(1, r_wide, r);
        if (last == 0) break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}


static int cinc_args(pydem_tile *t, CIncArgs &E)
{
    fill_sweep_args(t, E.G);
    E.rec = (NDRec *)t->nd_rec; E.nd = t->nd; E.cid = t->estamp;
    E.pit_off = reinterpret_cast<const int2 *>(t->contrib);
    E.flats = t->flats; E.edge_done = t->edge_done; E.edge_todo = t->edge_todo; E.uca = t->uca; E.set_done = 1;
    E.prof = t->counters + CS_EINC_PROF;
    E.nanq = reinterpret_cast<int32_t *>(t->edelta); E.n_nan = t->counters + CS_NAN_SEEDS;     // (the delta plane is idle in the compact form)
    E.round16 = (uint32_t)(t->einc_round % 65535) + 1u;
    return 0;
}

static int cinc_cascade(pydem_tile *t, const CIncArgs &E, CascadeDbg *dbg)
{
    int32_t *cnt3 = t->counters + CS_FRONTIER;
    int32_t *state = t->counters + CS_CASCADE_STATE;
    QE *q0 = (QE *)t->queue[0], *q1 = (QE *)t->queue[1];
    int r = 0;
    for (;;) {
        static int cinc_block = -1;
        if (cinc_block < 0) { const char *e = getenv("PYDEM_EINC_BLOCK"); cinc_block = e ? atoi(e) : 1024; }
        // (PYDEM_CINC_SMALL: the frontier width up to which ONE workgroup walks the levels; wider levels are launches over the chip)
        static int cinc_cap = -1;
        if (cinc_cap < 0) { const char *e = getenv("PYDEM_CINC_SMALL"); cinc_cap = e ? std::max(1, std::min(atoi(e), SMALL_CAP)) : 1024; }      // (measured on the flush of 8 x 16384^2: 4096 -> 1024 -0.8 ms per tile, 256 the same)
        hipLaunchKernelGGL(k_cinc_small, dim3(1), dim3(cinc_block), 0, t->stream, E, q0, q1, cnt3, r, state, cinc_cap);
        // (the usual case: the frontier stayed small and the cascade is over -- the records go to the tile right away,
        // ONE host synchronisation per round; cells finished so far are applied either way)
        hipLaunchKernelGGL(k_cinc_apply, dim3(grid_for(E.nd, 1024)), dim3(256), 0, t->stream, E);
        HIP_TRY(hipMemcpyAsync(t->h_counters, t->counters, CS_WINDOW * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        const int r_small = r;
        r = t->h_counters[CS_CASCADE_STATE];
        if (dbg) dbg->ran(0, r_small, r);
        int32_t last = t->h_counters[CS_FRONTIER + r % 3];
        if (last == 0) break;
        const bool wide = last > cinc_cap;
        const int r_wide = r;
        PYDEM_TRY(edge_wide_levels(t, cinc_cap, r, last, [&](int lv, int grid) {
            hipLaunchKernelGGL(k_cinc_level, dim3(grid), dim3(256), 0, t->stream, E, (lv % 2) ? q1 : q0, (lv % 2) ? q0 : q1, cnt3, lv);
        }));
        if (dbg) dbg->ran(1, r_wide, r);
        if (last == 0) {
            if (wide) { hipLaunchKernelGGL(k_cinc_apply, dim3(grid_for(E.nd, 1024)), dim3(256), 0, t->stream, E); HIP_TRY(hipStreamSynchronize(t->stream)); }
            break;
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// first incremental round after the graph was (re)built: count the cells that are not done and choose the form
static int einc_prepare(pydem_tile *t, IncArgs &E)
{
    if (E.G.n_pit > 0)
        hipLaunchKernelGGL(k_pit_offsets, dim3(grid_for(E.G.n_pit, 2048)), dim3(256), 0, t->stream, E.G.pin_dst, E.G.pit_src, E.G.n_pit,
                           reinterpret_cast<int2 *>(t->contrib));
    HIP_TRY(hipMemsetAsync(t->estamp, 0, (size_t)t->NN * 4, t->stream));
    unsigned long long *cnt64 = reinterpret_cast<unsigned long long *>(t->counters + CS_ND_COUNT);
    HIP_TRY(hipMemsetAsync(t->counters + CS_ND_COUNT, 0, 8 * sizeof(int32_t), t->stream));       // (CS_NAN_SEEDS with them)
    hipLaunchKernelGGL(k_nd_count, dim3(grid_for(t->NN, 4096)), dim3(256), 0, t->stream, t->edge_done, t->NN, cnt64);
    HIP_TRY(hipMemcpyAsync(t->h_counters + CS_ND_COUNT, t->counters + CS_ND_COUNT, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    const int64_t nd = (int64_t)*reinterpret_cast<unsigned long long *>(t->h_counters + CS_ND_COUNT);
    int64_t compact_max = ND_COMPACT_MAX;            // (read per fix-up: the tests switch the form)
    { const char *e = getenv("PYDEM_EINC_COMPACT_MAX"); if (e) compact_max = atoll(e); }
    t->einc_compact = nd <= compact_max;
    if (t->einc_compact) {
        PYDEM_TRY(tile_reserve(t, &t->nd_rec, &t->nd_bytes, (size_t)nd * sizeof(NDRec), (size_t)(nd + nd / 8 + 1024) * sizeof(NDRec), false));
        t->nd = (int32_t)nd;
        CIncArgs C;
        PYDEM_TRY(cinc_args(t, C));
        HIP_TRY(hipMemsetAsync(t->counters + CS_ND_NEXT, 0, sizeof(int32_t), t->stream));
        if (nd > 0) {
            hipLaunchKernelGGL(k_nd_assign, dim3(grid_for(t->NN, 4096)), dim3(256), 0, t->stream, C, t->NN, t->counters + CS_ND_NEXT);
            hipLaunchKernelGGL(k_nd_link, dim3(grid_for(nd, 1024)), dim3(256), 0, t->stream, C);
        }
    } else {
        hipLaunchKernelGGL(k_edge_clear_levels, dim3(grid_for(t->NN, 8192)), dim3(256), 0, t->stream, E.G.cinfo, t->NN);
        hipLaunchKernelGGL(k_einc_prepare, dim3(grid_for(t->NN, 8192)), dim3(256), 0, t->stream, E, t->NN);
    }
    HIP_TRY(hipGetLastError());
    t->einc_ready = true;
    t->edge_clean = false;          // the classic rounds find their zeroed state gone
    return 0;
}

// ---- condensed incremental rounds: host side (kernels in uca_cond.inl) ----------------------------------------
void tile_watch_line(pydem_tile *t, int axis, int64_t index)
{
    const int64_t lim = axis == 0 ? t->n : t->m;
    if (index < 0) index += lim;
    if (index == 0 || index == lim - 1) return;                    // perimeter: always watched
    for (const auto &w : t->watch) if (w.first == axis && w.second == index) return;
    t->watch.emplace_back(axis, index);
}

bool tile_line_watched(const pydem_tile *t, int axis, int64_t index)
{
    if (!(t->einc_ready && t->cond_live)) return true;             // nothing is deferred
    const int64_t lim = axis == 0 ? t->n : t->m;
    if (index < 0) index += lim;
    if (index == 0 || index == lim - 1) return true;
    for (size_t k = 0; k < t->watch_built && k < t->watch.size(); k++)
        if (t->watch[k].first == axis && t->watch[k].second == index) return true;
    return false;
}

static int cond_args(pydem_tile *t, CondArgsE &X)
{
    PYDEM_TRY(cinc_args(t, X.C));
    X.node = (CNode *)t->cond_node; X.nw = t->cond_nw; X.edge = (const CEdge *)t->cond_edge; X.slot = t->cond_slot;
    X.q0 = t->cond_q0; X.q1 = t->cond_q1; X.nanq = t->cond_nanq; X.nan_cap = t->cond_nan_cap; X.cnt = t->cond_cnt;
    X.gate = nullptr; X.gate_bit = 0; X.round_base = nullptr; X.round_add = nullptr;
    return 0;
}

// Build the condensed graph of the watched cells from the compact records (just linked by einc_prepare) ON THE HOST: the
// build of rounds 4-5, since round 6 the fall-back and the checker of the device build (cond_build_device below).  Returns 0
// and leaves cond_live false when the tile does not qualify (a cycle among the records, a pathological fan).
static thread_local const char *g_cond_host_gave_up = "";       // why the host build left the tile to the plain cascade (PYDEM_COND_BUILD=check reports it)
static int cond_build_host(pydem_tile *t)
{
    t->cond_live = false; t->cond_pending = false;
    g_cond_host_gave_up = "";
    const double t_begin = host_now_ms();
    const int32_t nd = t->nd;
    const int n = (int)t->n, m = (int)t->m;
    CIncArgs C;
    PYDEM_TRY(cinc_args(t, C));
    // ---- watched records: the perimeter and the lines other tiles read
    auto mark = [&](int axis, int64_t index) {
        const int64_t count = axis == 0 ? m : n;
        hipLaunchKernelGGL(k_cond_mark, dim3((unsigned)std::min<int64_t>(cdiv(count, 256), 64)), dim3(256), 0, t->stream, C, axis, index);
    };
    mark(0, 0); mark(0, n - 1); mark(1, 0); mark(1, m - 1);
    for (const auto &w : t->watch) mark(w.first, w.second);
    // ---- pit -> drain edges between records and the records' graph fields (scratch: the two queue buffers, idle until the
    // first cascade), through pinned staging
    CPitEdge *d_pe = reinterpret_cast<CPitEdge *>(t->queue[1]);
    const int32_t pe_cap = (int32_t)std::min<int64_t>(t->NN / 4, (int64_t)1 << 24);
    int32_t *d_npe = t->counters + CS_COND_EDGES;
    HIP_TRY(hipMemsetAsync(d_npe, 0, sizeof(int32_t), t->stream));
    if (C.G.n_pit > 0)
        hipLaunchKernelGGL(k_cond_pit_edges, dim3(grid_for(nd, 1024)), dim3(256), 0, t->stream, C, (const double *)t->pits.w, d_pe, d_npe, pe_cap);
    CRecH *d_hr = reinterpret_cast<CRecH *>(t->queue[0]);
    DevTemp d_tmp;
    if ((int64_t)nd * (int64_t)sizeof(CRecH) > t->NN * 4) {       // (small tiles that are mostly 'not done': the queue buffer is too short)
        PYDEM_TRY(d_tmp.alloc((size_t)nd * sizeof(CRecH)));
        d_hr = d_tmp.as<CRecH>();
    }
    hipLaunchKernelGGL(k_cond_extract, dim3(grid_for(nd, 1024)), dim3(256), 0, t->stream, C, d_hr);
    void *pin_v = nullptr;
    // (pinned staging: the records' extract, and behind it room for the nodes -- at most one per cell of a watched line)
    const size_t hr_bytes = (((size_t)nd * sizeof(CRecH) + 64) + 127) & ~(size_t)127;
    const size_t nw_bound = (size_t)std::min<int64_t>((int64_t)nd, (int64_t)(4 + t->watch.size()) * (int64_t)std::max(n, m));
    PYDEM_TRY(tile_pinned(t, hr_bytes + nw_bound * sizeof(CNode), &pin_v));
    const CRecH *hr = reinterpret_cast<const CRecH *>((char *)pin_v + 64);
    int32_t *h_npe = reinterpret_cast<int32_t *>(pin_v);
    HIP_TRY(hipMemcpyAsync(h_npe, d_npe, sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync((void *)hr, d_hr, (size_t)nd * sizeof(CRecH), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    const int32_t npe = *h_npe;
    if (npe > pe_cap) { g_cond_host_gave_up = "more pit edges among the records than its scratch holds"; return 0; }
    std::vector<CPitEdge> pe((size_t)npe);
    if (npe) HIP_TRY(hipMemcpy(pe.data(), d_pe, (size_t)npe * sizeof(CPitEdge), hipMemcpyDeviceToHost));
    const double t_copied = host_now_ms();
    std::sort(pe.begin(), pe.end(), [](const CPitEdge &a, const CPitEdge &b) { return a.src != b.src ? a.src < b.src : a.dst < b.dst; });
    // The order of the watched nodes is formed on a thread of its own beside the adjacency.  The counting passes of the
    // adjacency CAN run on several threads (PYDEM_COND_THREADS=<n>), but the default is one: on the two-socket hosts of the
    // GPU boxes the arrays the workers touch first land on their memory nodes, and the reverse sweep that follows (one thread,
    // random access into exactly those arrays) loses more (12-13 -> 14-25 ms) than the passes gain (8 -> 5 ms).
    // (Also measured and not kept: the sweep as a depth-first post-order over the out-edges alone, without predecessor lists --
    // adjacency 8 -> 5 ms, sweep 12.5 -> 17 ms: every record is visited twice and its targets' states once more.)
    static int n_thr = -1;
    if (n_thr < 0) {
        const char *e = getenv("PYDEM_COND_THREADS");
        const int hw = (int)std::thread::hardware_concurrency();
        n_thr = e ? atoi(e) : 1;
        n_thr = std::max(1, std::min(n_thr, std::min(16, hw > 0 ? hw : 1)));
    }
    const int T = nd < 20000 ? 1 : n_thr;
    const bool order_thread = nd >= 20000;
    auto par_for = [&](int64_t count, const std::function<void(int64_t, int64_t, int)> &fn) {
        if (T == 1 || count < 4096) { fn(0, count, 0); return; }
        std::vector<std::thread> th;
        for (int q = 1; q < T; q++) th.emplace_back(fn, count * q / T, count * (q + 1) / T, q);
        fn(0, count / T, 0);
        for (auto &x : th) x.join();
    };
    // ---- watched records in ascending cell order (on its own thread beside the adjacency)
    std::vector<int32_t> wrec, wid((size_t)nd, -1);
    auto node_order = [&]() {
        std::vector<std::pair<int32_t, int32_t>> key;
        for (int32_t k = 0; k < nd; k++) if (hr[k].wid == -2) key.emplace_back(hr[k].cell, k);
        std::sort(key.begin(), key.end());
        wrec.resize(key.size());
        for (size_t w = 0; w < key.size(); w++) { wrec[w] = key[w].second; wid[(size_t)key[w].second] = (int32_t)w; }
    };
    std::thread th_order;
    if (order_thread) th_order = std::thread(node_order);
    struct JoinGuard { std::thread &t; ~JoinGuard() { if (t.joinable()) t.join(); } } guard_order{th_order};
    // ---- out-edges per record (regular ones first, then the pit edges), in-degrees, predecessor lists
    std::vector<int32_t> ob((size_t)nd + 1, 0);
    par_for(nd, [&](int64_t k0, int64_t k1, int) { for (int64_t k = k0; k < k1; k++) ob[(size_t)k + 1] = (hr[k].out_id[0] >= 0) + (hr[k].out_id[1] >= 0); });
    for (const auto &e : pe) ob[(size_t)e.src + 1]++;
    for (int32_t k = 0; k < nd; k++) ob[(size_t)k + 1] += ob[(size_t)k];
    const int64_t n_out = ob[(size_t)nd];
    std::vector<int32_t> ot((size_t)n_out); std::vector<double> ow((size_t)n_out);
    std::vector<int32_t> indeg((size_t)nd, 0), pb((size_t)nd + 1, 0);
    bool bad_target = false;
    par_for(nd, [&](int64_t k0, int64_t k1, int) {
        const CPitEdge *q = std::lower_bound(pe.data(), pe.data() + pe.size(), (int32_t)k0, [](const CPitEdge &a, int32_t v) { return a.src < v; });
        const CPitEdge *qe = pe.data() + pe.size();
        for (int64_t k = k0; k < k1; k++) {
            int32_t f = ob[(size_t)k];
            for (int j = 0; j < 2; j++)
                if (hr[k].out_id[j] >= 0) { ot[(size_t)f] = hr[k].out_id[j]; ow[(size_t)f++] = hr[k].out_w[j]; }
            for (; q != qe && q->src == (int32_t)k; q++) { ot[(size_t)f] = q->dst; ow[(size_t)f++] = q->w; }
            for (int32_t e = ob[(size_t)k]; e < f; e++) {
                const int32_t tg = ot[(size_t)e];
                if (tg < 0 || tg >= nd) { bad_target = true; continue; }
                __atomic_fetch_add(&indeg[(size_t)tg], 1, __ATOMIC_RELAXED);
            }
        }
    });
    if (bad_target) { g_cond_host_gave_up = "an out-edge that leaves the records"; return 0; }
    for (int32_t k = 0; k < nd; k++) pb[(size_t)k + 1] = pb[(size_t)k] + indeg[(size_t)k];
    std::vector<int32_t> pred((size_t)n_out);
    {
        std::vector<int32_t> fill(pb.begin(), pb.end() - 1);
        par_for(nd, [&](int64_t k0, int64_t k1, int) {
            for (int64_t k = k0; k < k1; k++)
                for (int32_t e = ob[(size_t)k]; e < ob[(size_t)k + 1]; e++)
                    pred[(size_t)__atomic_fetch_add(&fill[(size_t)ot[(size_t)e]], 1, __ATOMIC_RELAXED)] = (int32_t)k;
        });
    }
    const double t_csr = host_now_ms();
    if (order_thread) th_order.join(); else node_order();
    const int32_t nw = (int32_t)wrec.size();
    const double t_wsort = host_now_ms();
    // ---- reverse topological order: X(k) = the watched cells the water of k reaches next, with the path weights, kept as
    // scale[k] * V(rep[k]): a cell with ONE out-edge shares the vector of its target (rep < 0: the unit vector of watched
    // node -1 - rep), only the cells where the flow splits merge two (sorted) vectors into a new one.  Vectors live in
    // chunks that never move; vref[id] = where vector id is.
    typedef std::pair<int32_t, double> Ent;
    struct VecRef { const Ent *p; int64_t n; };
    std::unique_ptr<VecRef[]> vref(new VecRef[(size_t)nd + 1]);
    int32_t n_vec = 0;
    int64_t n_ent = 0;
    std::vector<int32_t> rep((size_t)nd, INT32_MIN);     // INT32_MIN: the empty vector (the water ends inside the tile)
    std::vector<double> scale((size_t)nd, 0.0);
    // (the sweep itself stays on one thread: the graph of the records is a bundle of rivers, narrow and thousands of records
    // deep -- a Kahn pass shared by 4 / 8 threads over a common ready list measured 100-150 ms against 12: every record then
    // costs a few cache-line transfers between cores.  Last in, first out: a river is walked while its lines are warm.)
    std::vector<int32_t> out_left((size_t)nd), stack;
    for (int32_t k = 0; k < nd; k++) { out_left[(size_t)k] = ob[(size_t)k + 1] - ob[(size_t)k]; if (!out_left[(size_t)k]) stack.push_back(k); }
    constexpr size_t CHUNK = (size_t)1 << 18;
    std::vector<std::unique_ptr<Ent[]>> chunks;
    Ent *cur = nullptr; size_t cur_left = 0;
    int64_t processed = 0;
    std::vector<Ent> acc, nxt;
    // the vector of target tg as seen through an edge of weight w: (rep, factor)
    auto through = [&](int32_t tg, double w, int32_t &r, double &f) {
        if (wid[(size_t)tg] >= 0) { r = -1 - wid[(size_t)tg]; f = w; }
        else { r = rep[(size_t)tg]; f = w * scale[(size_t)tg]; }
    };
    auto add_into = [&](int32_t r, double f) {            // acc += f * V(r), both sorted by node
        if (r == INT32_MIN) return;
        Ent unit(-1 - r, 1.0);
        const Ent *vb = r < 0 ? &unit : vref[(size_t)r].p, *ve = r < 0 ? &unit + 1 : vref[(size_t)r].p + vref[(size_t)r].n;
        nxt.clear();
        size_t i = 0;
        for (const Ent *p = vb; p != ve; p++) {
            while (i < acc.size() && acc[i].first < p->first) nxt.push_back(acc[i++]);
            if (i < acc.size() && acc[i].first == p->first) { nxt.emplace_back(p->first, acc[i].second + f * p->second); i++; }
            else nxt.emplace_back(p->first, f * p->second);
        }
        while (i < acc.size()) nxt.push_back(acc[i++]);
        acc.swap(nxt);
    };
    while (!stack.empty()) {
        const int32_t k = stack.back(); stack.pop_back();
        processed++;
        const int32_t e0 = ob[(size_t)k], e1 = ob[(size_t)k + 1];
        if (e1 - e0 == 1) through(ot[(size_t)e0], ow[(size_t)e0], rep[(size_t)k], scale[(size_t)k]);
        else if (e1 - e0 >= 2) {
            acc.clear();
            for (int32_t e = e0; e < e1; e++) { int32_t r; double f; through(ot[(size_t)e], ow[(size_t)e], r, f); add_into(r, f); }
            if (!acc.empty()) {
                if (acc.size() > cur_left) {
                    const size_t sz = std::max(CHUNK, acc.size());
                    chunks.emplace_back(new Ent[sz]);
                    cur = chunks.back().get(); cur_left = sz;
                }
                std::copy(acc.begin(), acc.end(), cur);
                vref[(size_t)n_vec].p = cur; vref[(size_t)n_vec].n = (int64_t)acc.size();
                cur += acc.size(); cur_left -= acc.size();
                rep[(size_t)k] = n_vec++; scale[(size_t)k] = 1.0;
                n_ent += (int64_t)acc.size();
                if (n_ent > ((int64_t)1 << 27)) { g_cond_host_gave_up = "a pathological fan"; return 0; }    // (keep the cell-by-cell rounds)
            }
        }
        for (int32_t e = pb[(size_t)k]; e < pb[(size_t)k + 1]; e++) if (--out_left[(size_t)pred[(size_t)e]] == 0) stack.push_back(pred[(size_t)e]);
    }
    if (processed != nd) { g_cond_host_gave_up = "a cycle among the records"; return 0; }       // not a DAG: plain cascade
    const double t_swept = host_now_ms();
    // ---- nodes, edges, slots
    if ((size_t)nw > nw_bound) { pydem_set_error("condensed edge rounds: %d watched nodes, expected at most %zu", nw, nw_bound); return -5; }
    CNode *nodes = reinterpret_cast<CNode *>((char *)pin_v + hr_bytes);
    auto vsize = [&](int32_t r) -> int64_t { return r == INT32_MIN ? 0 : (r < 0 ? 1 : vref[(size_t)r].n); };
    int64_t ne_all = 0;
    for (int32_t w = 0; w < nw; w++) ne_all += vsize(rep[(size_t)wrec[(size_t)w]]);
    if (ne_all > INT32_MAX / 2) { g_cond_host_gave_up = "too many edges"; return 0; }
    // all edges in source order first (dst, weight), in-degrees; then the split into inline / array parts
    std::vector<int32_t> e_dst((size_t)ne_all); std::vector<double> e_w((size_t)ne_all);
    std::vector<int32_t> ebeg((size_t)nw + 1, 0), n_in((size_t)nw, 0);
    {
        int64_t e = 0;
        for (int32_t w = 0; w < nw; w++) {
            const int32_t k = wrec[(size_t)w];
            const int32_t r = rep[(size_t)k];
            const double f = scale[(size_t)k];
            if (r != INT32_MIN && r < 0) { e_dst[(size_t)e] = -1 - r; e_w[(size_t)e] = f; e++; }
            else if (r != INT32_MIN)
                for (int64_t q = 0; q < vref[(size_t)r].n; q++) { e_dst[(size_t)e] = vref[(size_t)r].p[q].first; e_w[(size_t)e] = f * vref[(size_t)r].p[q].second; e++; }
            ebeg[(size_t)w + 1] = (int32_t)e;
        }
        for (int64_t q = 0; q < ne_all; q++) n_in[(size_t)e_dst[(size_t)q]]++;
    }
    std::vector<int32_t> in_base((size_t)nw + 1, 0), out_base((size_t)nw + 1, 0);
    for (int32_t w = 0; w < nw; w++) {
        in_base[(size_t)w + 1] = in_base[(size_t)w] + std::max(0, n_in[(size_t)w] - 2);
        out_base[(size_t)w + 1] = out_base[(size_t)w] + std::max(0, ebeg[(size_t)w + 1] - ebeg[(size_t)w] - 2);
    }
    const int64_t ne = out_base[(size_t)nw], nslot = in_base[(size_t)nw];      // array parts
    std::vector<CEdge> edges((size_t)std::max<int64_t>(ne, 1));
    std::vector<int32_t> fill((size_t)nw, 0);                                    // next in-slot of a node (sources ascend with the edge order)
    for (int32_t w = 0; w < nw; w++) {
        CNode &N = nodes[(size_t)w];
        memset(&N, 0, sizeof(N));
        const int32_t k = wrec[(size_t)w];
        N.rec = k; N.cell = hr[k].cell; N.cw = hr[k].cw;
        N.n_in = n_in[(size_t)w]; N.n_out = ebeg[(size_t)w + 1] - ebeg[(size_t)w];
        N.in_base = in_base[(size_t)w]; N.out_base = out_base[(size_t)w];
        for (int e = 0; e < N.n_out; e++) {
            const int64_t q = (int64_t)ebeg[(size_t)w] + e;
            CEdge ed;
            ed.dst = e_dst[(size_t)q]; ed.w = e_w[(size_t)q];
            const int32_t sl = fill[(size_t)ed.dst]++;
            ed.slot = sl < 2 ? -1 - sl : in_base[(size_t)ed.dst] + sl - 2;
            if (e < 2) N.e_inl[e] = ed; else edges[(size_t)(N.out_base + e - 2)] = ed;
        }
        const int32_t outside = hr[k].cnt - indeg[(size_t)k];                    // +1 while the cell is a 'todo' inlet (k_nd_link)
        if (outside != 0 && outside != 1) { pydem_set_error("condensed edge rounds: inconsistent count of record %d", k); return -5; }
        N.cnt = N.n_in + outside;
    }
    // ---- device copy (one allocation: nodes | edges | slots | two queues | NaN list | counters)
    const size_t nan_cap = (size_t)ne_all + (size_t)nw + 64;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_node = take((size_t)nw * sizeof(CNode)), o_edge = take((size_t)(ne + 1) * sizeof(CEdge)), o_slot = take((size_t)(nslot + 1) * 8),
                 o_q0 = take((size_t)nw * 4), o_q1 = take((size_t)nw * 4), o_nan = take(nan_cap * 4), o_cnt = take(64);
    PYDEM_TRY(tile_reserve(t, &t->cond_mem, &t->cond_bytes, off, off + off / 8, false));
    char *base = (char *)t->cond_mem;
    t->cond_node = base + o_node; t->cond_edge = base + o_edge; t->cond_slot = (double *)(base + o_slot);
    t->cond_q0 = (int32_t *)(base + o_q0); t->cond_q1 = (int32_t *)(base + o_q1); t->cond_nanq = (int32_t *)(base + o_nan);
    t->cond_cnt = (int32_t *)(base + o_cnt); t->cond_nw = nw; t->cond_nan_cap = (int32_t)std::min<size_t>(nan_cap, (size_t)INT32_MAX);
    HIP_TRY(hipMemsetAsync(base + o_slot, 0, off - o_slot, t->stream));
    if (nw) HIP_TRY(hipMemcpyAsync(t->cond_node, nodes, (size_t)nw * sizeof(CNode), hipMemcpyHostToDevice, t->stream));
    if (ne) HIP_TRY(hipMemcpyAsync(t->cond_edge, edges.data(), (size_t)ne * sizeof(CEdge), hipMemcpyHostToDevice, t->stream));
    CondArgsE X;
    t->cond_live = true;                  // (cond_args reads the fields set above)
    PYDEM_TRY(cond_args(t, X));
    if (nw) hipLaunchKernelGGL(k_cond_attach, dim3(grid_for(nw, 256)), dim3(256), 0, t->stream, X);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));     // (nodes / edges are host vectors about to go out of scope)
    t->watch_built = t->watch.size();
    if (getenv("PYDEM_EDGE_DEBUG"))
        fprintf(stderr, "condensed edge rounds: %d records -> %d watched nodes, %lld edges (%d pit edges among the records); %.2f ms "
                "(copy %.2f, adjacency %.2f, node order %.2f, reverse sweep %.2f [%zu vectors, %zu entries], nodes + upload %.2f)\n",
                nd, nw, (long long)ne_all, npe, host_now_ms() - t_begin, t_copied - t_begin, t_csr - t_copied, t_wsort - t_csr, t_swept - t_wsort,
                (size_t)n_vec, (size_t)n_ent, host_now_ms() - t_swept);
    return 0;
}

// ---- the same graph built on the device (kernels in uca_cbuild.inl) ---------------------------------------------------
static int cb_reserve(pydem_tile *t, int which, size_t bytes)
{
    if (t->cb_bytes[which] >= bytes) return 0;
    if (t->cb_mem[which]) HIP_TRY(hipStreamSynchronize(t->stream));      // (kernels of the build may still read the old block)
    const size_t want = (bytes + bytes / 4 + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);     // (headroom + 1 MiB steps: run-to-run sizes move by a few records)
    return tile_reserve(t, &t->cb_mem[which], &t->cb_bytes[which], bytes, want, false);
}

struct CBump {
    char *base; size_t off = 0;
    explicit CBump(void *b) : base((char *)b) {}
    template <typename T> T *take(size_t count) { T *p = base ? (T *)(base + off) : nullptr; off += (count * sizeof(T) + 255) & ~(size_t)255; return p; }
};

// *status: 1 built (cond_live), 0 the tile does not qualify (a cycle among the records: the host build would say the same),
// -1 the device build gave up (a vector of more than CB_RUN entries, pool overflow): try the host build
static int cond_build_device(pydem_tile *t, int *status)
{
    *status = -1;
    t->cond_live = false; t->cond_pending = false;
    const double t_begin = host_now_ms();
    const int32_t nd = t->nd;
    const int n = (int)t->n, m = (int)t->m;
    CBArgs B;
    memset(&B, 0, sizeof(B));
    PYDEM_TRY(cinc_args(t, B.C));
    const CIncArgs &C = B.C;
    auto mark = [&](int axis, int64_t index) {
        const int64_t count = axis == 0 ? m : n;
        hipLaunchKernelGGL(k_cond_mark, dim3((unsigned)std::min<int64_t>(cdiv(count, 256), 64)), dim3(256), 0, t->stream, C, axis, index);
    };
    mark(0, 0); mark(0, n - 1); mark(1, 0); mark(1, m - 1);
    for (const auto &w : t->watch) mark(w.first, w.second);
    const size_t nw_bound = (size_t)std::min<int64_t>((int64_t)nd, (int64_t)(4 + t->watch.size()) * (int64_t)std::max(n, m));
    const int nd1 = nd + 1;
    size_t tmp_scan = 0, tmp_sortw = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_scan, (int32_t *)nullptr, (int32_t *)nullptr, nd1, t->stream));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sortw, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                                               (int)nw_bound, 0, 32, t->stream));
    const size_t tmp1 = std::max(tmp_scan, tmp_sortw) + 256;
    // ---- phase 1: per-record state, counts
    void *tmp_a = nullptr;
    auto lay1 = [&](void *base) {
        CBump A(base);
        B.rv = A.take<CBVal>((size_t)nd); B.ri = A.take<CBRec>((size_t)nd);
        B.pred_cnt = A.take<int32_t>((size_t)nd1); B.pit_cnt = A.take<int32_t>((size_t)nd1);
        B.pred_beg = A.take<int32_t>((size_t)nd1); B.pit_beg = A.take<int32_t>((size_t)nd1);
        B.q0 = A.take<int32_t>((size_t)nd * CB_NQ); B.q1 = A.take<int32_t>((size_t)nd * CB_NQ);     // (CB_NQ sub-queues each: any of them may hold a whole level)
        B.qcnt = A.take<int32_t>((size_t)3 * CB_NQ * CB_PAD); B.poolc = A.take<int32_t>((size_t)CB_NQ * CB_PAD);
        B.wcell = A.take<int32_t>(nw_bound); B.wrec = A.take<int32_t>(nw_bound);
        B.wcell_s = A.take<int32_t>(nw_bound); B.wrec_s = A.take<int32_t>(nw_bound);
        B.ctr = A.take<int32_t>(CBC_WORDS);
        tmp_a = A.take<char>(tmp1);
        return A.off;
    };
    PYDEM_TRY(cb_reserve(t, 0, lay1(nullptr)));
    lay1(t->cb_mem[0]);
    B.w_cap = (int32_t)nw_bound;
    B.w_sorted = t->pits.w;
    HIP_TRY(hipMemsetAsync(B.ctr, 0, CBC_WORDS * sizeof(int32_t), t->stream));
    HIP_TRY(hipMemsetAsync(B.qcnt, 0, (size_t)4 * CB_NQ * CB_PAD * sizeof(int32_t), t->stream));      // (qcnt and, behind it, poolc)
    B.qcap = nd;
    const int g_nd = grid_for(nd, 1024);
    hipLaunchKernelGGL(k_cb_count, dim3(g_nd), dim3(256), 0, t->stream, B);
    { size_t tb = tmp1; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_a, tb, B.pred_cnt, B.pred_beg, nd1, t->stream)); }
    { size_t tb = tmp1; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_a, tb, B.pit_cnt, B.pit_beg, nd1, t->stream)); }
    int32_t *h = t->h_counters;          // (here the mirror of the build's own counters B.ctr, and two list totals behind them)
    static_assert(CBC_WORDS <= CS_H_CB_TOTALS, "the list totals follow the build's counters in the pinned mirror");
    HIP_TRY(hipMemcpyAsync(h, B.ctr, CBC_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync(h + CS_H_CB_TOTALS, B.pred_beg + nd, sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync(h + CS_H_CB_TOTALS + 1, B.pit_beg + nd, sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    const int32_t nw = h[CBC_NW], n_pred = h[CS_H_CB_TOTALS], n_pit = h[CS_H_CB_TOTALS + 1];
    if (h[CBC_FAIL] & 2) { pydem_set_error("condensed edge rounds: inconsistent in-edge count of a record"); return -5; }
    if ((size_t)nw > nw_bound) { pydem_set_error("condensed edge rounds: %d watched nodes, expected at most %zu", nw, nw_bound); return -5; }
    const double t_counted = host_now_ms();
    // ---- phase 2: lists, node order, the reverse sweep
    const int64_t pool_cap = std::min<int64_t>((int64_t)nd + 16384, (int64_t)1 << 24);       // entries per region (CB_NQ regions: 16 x nd in all, ~8 x what the merges of a 16384^2 tile take)
    const int nw1 = nw + 1;
    auto lay2 = [&](void *base) {
        CBump A(base);
        B.pred = A.take<int32_t>((size_t)n_pred + 1); B.pit = A.take<CBPit>((size_t)n_pit + 1);
        B.pool = A.take<CBEnt>((size_t)pool_cap * CB_NQ);
        B.nout_c = A.take<int32_t>((size_t)nw1); B.nout = A.take<int32_t>((size_t)nw1);
        B.n_in = A.take<int32_t>((size_t)nw1); B.in_first = A.take<int32_t>((size_t)nw1);
        B.exc_in_c = A.take<int32_t>((size_t)nw1); B.exc_in = A.take<int32_t>((size_t)nw1);
        B.exc_out_c = A.take<int32_t>((size_t)nw1); B.exc_out = A.take<int32_t>((size_t)nw1);
        return A.off;
    };
    PYDEM_TRY(cb_reserve(t, 1, lay2(nullptr)));
    lay2(t->cb_mem[1]);
    B.pool_cap = (int32_t)pool_cap; B.nw = nw;
    hipLaunchKernelGGL(k_cb_fill, dim3(g_nd), dim3(256), 0, t->stream, B);
    int cell_bits = 1;
    while (((int64_t)1 << cell_bits) < t->NN) cell_bits++;
    if (nw > 0) {
        size_t tb = tmp1;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp_a, tb, B.wcell, B.wcell_s, B.wrec, B.wrec_s, nw, 0, cell_bits, t->stream));
        hipLaunchKernelGGL(k_cb_wid, dim3(grid_for(nw, 256)), dim3(256), 0, t->stream, B);
    }
    // the levels: one launch per level over the whole chip, in batches; one look from the host per batch (the launches behind the
    // end of the sweep find empty sub-queues and return at once)
    static int cb_grid = -1, cb_chain = -1;
    if (cb_grid < 0) { const char *e = getenv("PYDEM_CB_GRID"); cb_grid = e ? std::max(1, std::min(atoi(e), 65536)) : CB_GRID; cb_grid = ((cb_grid + CB_NQ - 1) / CB_NQ) * CB_NQ; }
    if (cb_chain < 0) { const char *e = getenv("PYDEM_CB_CHAIN"); cb_chain = e ? std::max(0, atoi(e)) : 2; }
    B.max_chain = cb_chain;
    int32_t *d_dbg = nullptr;                              // PYDEM_CB_DEBUG=1: per-level statistics of the sweep to stderr (diagnostic, one extra allocation)
    const int dbg_levels = 4096;
    DevTemp dbg_mem;
    if (getenv("PYDEM_CB_DEBUG")) { PYDEM_TRY(dbg_mem.alloc((size_t)dbg_levels * 4 * sizeof(int32_t))); d_dbg = dbg_mem.as<int32_t>(); HIP_TRY(hipMemsetAsync(d_dbg, 0, (size_t)dbg_levels * 4 * sizeof(int32_t), t->stream)); }
    B.dbg = d_dbg; B.level = 0;
    int levels_run = 0;
    void *pin_q = nullptr;
    PYDEM_TRY(tile_pinned(t, (size_t)3 * CB_NQ * CB_PAD * sizeof(int32_t), &pin_q));
    const int32_t *hq = (const int32_t *)pin_q;
    for (;;) {
        for (int b = 0; b < 64; b++, levels_run++) {
            B.level = levels_run < dbg_levels ? levels_run : dbg_levels - 1;
            hipLaunchKernelGGL(k_cb_level, dim3(cb_grid), dim3(CB_LANES), 0, t->stream, B, levels_run);
        }
        HIP_TRY(hipMemcpyAsync(h, B.ctr, CBC_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipMemcpyAsync(pin_q, B.qcnt, (size_t)3 * CB_NQ * CB_PAD * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        int64_t left = 0;
        for (int q = 0; q < CB_NQ; q++) left += hq[((levels_run % 3) * CB_NQ + q) * CB_PAD];
        if (left == 0 || (h[CBC_FAIL] & 1)) break;
        if (levels_run > (1 << 22)) { pydem_set_error("condensed edge rounds: flow paths too long"); return -5; }
    }
    if (d_dbg) {
        std::vector<int32_t> hd((size_t)dbg_levels * 4);
        HIP_TRY(hipMemcpy(hd.data(), d_dbg, hd.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        fprintf(stderr, "cb levels (frontier / largest merge / entries merged / deepest chain):");
        for (int l = 0; l < levels_run && l < dbg_levels; l++) { if (l % 8 == 0) fprintf(stderr, "\n  %4d:", l); fprintf(stderr, " %d/%d/%d/%d", hd[4 * l], hd[4 * l + 1], hd[4 * l + 2], hd[4 * l + 3]); }
        fprintf(stderr, "\n");
        B.dbg = nullptr;
    }
    hipLaunchKernelGGL(k_cb_nout, dim3(grid_for(nw1, 256)), dim3(256), 0, t->stream, B);
    { size_t tb = tmp1; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_a, tb, B.nout_c, B.nout, nw1, t->stream)); }
    HIP_TRY(hipMemcpyAsync(h, B.ctr, CBC_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync(h + CS_H_CB_TOTALS, B.nout + nw, sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    const double t_swept = host_now_ms();
    const int32_t ne_all = h[CS_H_CB_TOTALS], levels = h[CBC_LEVELS], n_slow = h[CBC_SLOW];
    if (h[CBC_FAIL] & 1) return 0;                              // (*status == -1: the host build takes over)
    { const char *e = getenv("PYDEM_CB_FORCE_FALLBACK"); if (e && atoi(e) > 0) return 0; }      // (tests: the hand-over to the host build after a finished sweep)
    if (h[CBC_PROC] != nd) { *status = 0; return 0; }           // a cycle among the records: not a DAG, plain cascade
    if (ne_all > INT32_MAX / 2) { *status = 0; return 0; }
    // ---- phase 3: edges, slots, nodes -- straight into the round's arrays (one allocation: nodes | edges | slots | two queues |
    // NaN list | counters; edge / slot arrays sized by the bound ne_all)
    size_t tmp_sorte = 0, tmp_scanw = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sorte, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                                               (int)std::max(ne_all, 1), 0, 32, t->stream));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_scanw, (int32_t *)nullptr, (int32_t *)nullptr, nw1, t->stream));
    const size_t tmp3 = std::max(tmp_sorte, tmp_scanw) + 256;
    void *tmp_c = nullptr;
    auto lay3 = [&](void *base) {
        CBump A(base);
        const size_t ne1 = (size_t)ne_all + 1;
        B.e_dst = A.take<int32_t>(ne1); B.e_q = A.take<int32_t>(ne1); B.e_dst_s = A.take<int32_t>(ne1); B.e_q_s = A.take<int32_t>(ne1);
        B.e_slot = A.take<int32_t>(ne1); B.e_w = A.take<double>(ne1);
        tmp_c = A.take<char>(tmp3);
        return A.off;
    };
    PYDEM_TRY(cb_reserve(t, 2, lay3(nullptr)));
    lay3(t->cb_mem[2]);
    const size_t nan_cap = (size_t)ne_all + (size_t)nw + 64;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_node = take((size_t)nw * sizeof(CNode)), o_edge = take((size_t)(ne_all + 1) * sizeof(CEdge)), o_slot = take((size_t)(ne_all + 1) * 8),
                 o_q0 = take((size_t)nw * 4), o_q1 = take((size_t)nw * 4), o_nan = take(nan_cap * 4), o_cnt = take(64);
    PYDEM_TRY(tile_reserve(t, &t->cond_mem, &t->cond_bytes, off, (off + off / 4 + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1), false));
    char *base = (char *)t->cond_mem;
    t->cond_node = base + o_node; t->cond_edge = base + o_edge; t->cond_slot = (double *)(base + o_slot);
    t->cond_q0 = (int32_t *)(base + o_q0); t->cond_q1 = (int32_t *)(base + o_q1); t->cond_nanq = (int32_t *)(base + o_nan);
    t->cond_cnt = (int32_t *)(base + o_cnt); t->cond_nw = nw; t->cond_nan_cap = (int32_t)std::min<size_t>(nan_cap, (size_t)INT32_MAX);
    B.node = (CNode *)t->cond_node; B.edge = (CEdge *)t->cond_edge;
    HIP_TRY(hipMemsetAsync(base + o_slot, 0, off - o_slot, t->stream));
    if (nw > 0) {
        const int g_nw = grid_for(nw1, 256);
        hipLaunchKernelGGL(k_cb_edges, dim3(g_nw), dim3(256), 0, t->stream, B);
        hipLaunchKernelGGL(k_cb_excess, dim3(g_nw), dim3(256), 0, t->stream, B);
        { size_t tb = tmp3; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_c, tb, B.n_in, B.in_first, nw1, t->stream)); }
        { size_t tb = tmp3; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_c, tb, B.exc_in_c, B.exc_in, nw1, t->stream)); }
        { size_t tb = tmp3; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp_c, tb, B.exc_out_c, B.exc_out, nw1, t->stream)); }
        if (ne_all > 0) {
            int node_bits = 1;
            while (((int64_t)1 << node_bits) < nw) node_bits++;
            size_t tb = tmp3;
            HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp_c, tb, B.e_dst, B.e_dst_s, B.e_q, B.e_q_s, ne_all, 0, node_bits, t->stream));
            hipLaunchKernelGGL(k_cb_slots, dim3(grid_for(ne_all, 256)), dim3(256), 0, t->stream, B, ne_all);
        }
        hipLaunchKernelGGL(k_cb_nodes, dim3(g_nw), dim3(256), 0, t->stream, B);
    }
    CondArgsE X;
    t->cond_live = true;                  // (cond_args reads the fields set above)
    PYDEM_TRY(cond_args(t, X));
    if (nw) hipLaunchKernelGGL(k_cond_attach, dim3(grid_for(nw, 256)), dim3(256), 0, t->stream, X);
    HIP_TRY(hipGetLastError());
    t->watch_built = t->watch.size();
    *status = 1;
    if (getenv("PYDEM_EDGE_DEBUG")) {
        HIP_TRY(hipStreamSynchronize(t->stream));
        fprintf(stderr, "condensed edge rounds (device build): %d records -> %d watched nodes, %d edges (%d pit edges among the records); %.2f ms "
                "(lists %.2f, reverse sweep %.2f [%d levels, %d launches, %d merges from the pool], nodes %.2f)\n",
                nd, nw, ne_all, n_pit, host_now_ms() - t_begin, t_counted - t_begin, t_swept - t_counted, levels, levels_run, n_slow, host_now_ms() - t_swept);
    }
    return 0;
}

// PYDEM_COND_BUILD=check: the device build against the host build, node by node (same nodes, counts, edges and slots;
// weights to 1e-12 relative: the host sorts the pit edges of one pit by record id, the device by drain cell)
static int cond_build_check(pydem_tile *t)
{
    int st = -1;
    PYDEM_TRY(cond_build_device(t, &st));
    if (st != 1) { PYDEM_TRY(cond_build_host(t)); if (st == 0 && t->cond_live) { pydem_set_error("condensed build check: the device build found a cycle, the host build none"); return -5; } return 0; }
    HIP_TRY(hipStreamSynchronize(t->stream));
    const int32_t nw = t->cond_nw;
    std::vector<CNode> dn((size_t)std::max(nw, 1));
    std::vector<CEdge> de;
    auto grab = [&](std::vector<CNode> &nodes, std::vector<CEdge> &edges) -> int {
        nodes.resize((size_t)std::max(t->cond_nw, 1));
        if (t->cond_nw) HIP_TRY(hipMemcpy(nodes.data(), t->cond_node, (size_t)t->cond_nw * sizeof(CNode), hipMemcpyDeviceToHost));
        int64_t ne = 0;
        for (int32_t w = 0; w < t->cond_nw; w++) ne = std::max<int64_t>(ne, (int64_t)nodes[(size_t)w].out_base + std::max(0, nodes[(size_t)w].n_out - 2));
        edges.resize((size_t)std::max<int64_t>(ne, 1));
        if (ne) HIP_TRY(hipMemcpy(edges.data(), t->cond_edge, (size_t)ne * sizeof(CEdge), hipMemcpyDeviceToHost));
        return 0;
    };
    PYDEM_TRY(grab(dn, de));
    // (the device build has attached the nodes to their records: undo that before the host build reads them again)
    std::vector<CNode> hn; std::vector<CEdge> he;
    {
        CondArgsE X; PYDEM_TRY(cond_args(t, X));
        if (nw) hipLaunchKernelGGL(k_cond_detach, dim3(grid_for(nw, 256)), dim3(256), 0, t->stream, X);
    }
    PYDEM_TRY(cond_build_host(t));
    if (!t->cond_live) {
        // (a capacity limit of the host build -- the pit edges among the records go through a scratch of NN / 4 entries -- is not a
        // difference: the device build has no such limit and its operator stands; anything else is)
        if (!strcmp(g_cond_host_gave_up, "more pit edges among the records than its scratch holds")) {
            if (getenv("PYDEM_EDGE_DEBUG")) fprintf(stderr, "condensed build check: host build skipped (%s); device operator rebuilt and kept\n", g_cond_host_gave_up);
            int st2 = -1;
            PYDEM_TRY(cond_build_device(t, &st2));
            if (st2 != 1) { pydem_set_error("condensed build check: the device build did not repeat itself"); return -5; }
            return 0;
        }
        pydem_set_error("condensed build check: the host build gave up (%s) where the device build did not", g_cond_host_gave_up);
        return -5;
    }
    HIP_TRY(hipStreamSynchronize(t->stream));
    PYDEM_TRY(grab(hn, he));
    if (t->cond_nw != nw) { pydem_set_error("condensed build check: %d nodes on the device, %d on the host", nw, t->cond_nw); return -5; }
    double worst = 0.0;
    for (int32_t w = 0; w < nw; w++) {
        const CNode &a = dn[(size_t)w], &b = hn[(size_t)w];
        if (a.cell != b.cell || a.cw != b.cw || a.cnt != b.cnt || a.n_in != b.n_in || a.n_out != b.n_out || a.in_base != b.in_base || a.out_base != b.out_base) {
            pydem_set_error("condensed build check: node %d (cell %d / %d): cnt %d / %d, in %d / %d, out %d / %d, bases %d %d / %d %d", w, a.cell, b.cell, a.cnt, b.cnt,
                            a.n_in, b.n_in, a.n_out, b.n_out, a.in_base, a.out_base, b.in_base, b.out_base);
            return -5;
        }
        for (int e = 0; e < a.n_out; e++) {
            const CEdge &x = e < 2 ? a.e_inl[e] : de[(size_t)(a.out_base + e - 2)], &y = e < 2 ? b.e_inl[e] : he[(size_t)(b.out_base + e - 2)];
            if (x.dst != y.dst || x.slot != y.slot) { pydem_set_error("condensed build check: node %d edge %d: dst %d / %d, slot %d / %d", w, e, x.dst, y.dst, x.slot, y.slot); return -5; }
            const double d = fabs(x.w - y.w) / (fabs(y.w) > 0 ? fabs(y.w) : 1.0);
            if (!(d <= 1e-12)) { pydem_set_error("condensed build check: node %d edge %d: weight %.17g / %.17g", w, e, x.w, y.w); return -5; }
            worst = std::max(worst, d);
        }
    }
    if (getenv("PYDEM_EDGE_DEBUG")) {
        int64_t h_out[6] = {0, 0, 0, 0, 0, 0}, h_in[6] = {0, 0, 0, 0, 0, 0};      // <= 2, 3-4, 5-8, 9-16, 17-64, more
        int mx_out = 0, mx_in = 0;
        auto cls = [](int n) { return n <= 2 ? 0 : (n <= 4 ? 1 : (n <= 8 ? 2 : (n <= 16 ? 3 : (n <= 64 ? 4 : 5)))); };
        for (int32_t w = 0; w < nw; w++) { h_out[cls(dn[(size_t)w].n_out)]++; h_in[cls(dn[(size_t)w].n_in)]++; mx_out = std::max(mx_out, dn[(size_t)w].n_out); mx_in = std::max(mx_in, dn[(size_t)w].n_in); }
        fprintf(stderr, "condensed build check: %d nodes identical, weights within %.3g relative; out-edges per node <=2 / 3-4 / 5-8 / 9-16 / 17-64 / more: %lld %lld %lld %lld %lld %lld (max %d); "
                "in-edges: %lld %lld %lld %lld %lld %lld (max %d)\n", nw, worst, (long long)h_out[0], (long long)h_out[1], (long long)h_out[2], (long long)h_out[3], (long long)h_out[4], (long long)h_out[5], mx_out,
                (long long)h_in[0], (long long)h_in[1], (long long)h_in[2], (long long)h_in[3], (long long)h_in[4], (long long)h_in[5], mx_in);
    }
    return 0;
}

// Build the condensed graph of the watched cells from the compact records (just linked by einc_prepare).  Returns 0 and
// leaves cond_live false when the tile does not qualify (switched off, too many records, a cycle among the records).
static int cond_build(pydem_tile *t)
{
    t->cond_live = false; t->cond_pending = false;
    static int enabled = -1;
    if (enabled < 0) { const char *e = getenv("PYDEM_EDGE_COND"); enabled = e ? atoi(e) : 1; }
    int64_t max_nd = 1 << 20;
    { const char *e = getenv("PYDEM_EDGE_COND_MAX"); if (e) max_nd = atoll(e); }
    if (!enabled || !t->einc_compact || t->nd <= 0 || t->nd > max_nd) return 0;
    const char *how = getenv("PYDEM_COND_BUILD");           // (read per build: the tests switch it) device (default) | host | check
    if (how && !strcmp(how, "host")) return cond_build_host(t);
    if (how && !strcmp(how, "check")) return cond_build_check(t);
    int st = -1;
    PYDEM_TRY(cond_build_device(t, &st));
    if (st < 0) {
        if (getenv("PYDEM_EDGE_DEBUG")) fprintf(stderr, "condensed edge rounds (device build): gave up, the host build takes over\n");
        return cond_build_host(t);
    }
    return 0;
}

// the interior catches up: done watched nodes -> their records, the NaN flood below the nodes it passed, ONE cascade
static int cond_catchup(pydem_tile *t, int set_done, CascadeDbg *dbg)
{
    if (!(t->einc_ready && t->cond_live)) return 0;
    CondArgsE X;
    PYDEM_TRY(cond_args(t, X));
    X.C.set_done = set_done;
    HIP_TRY(hipMemsetAsync(t->counters, 0, CS_WINDOW * sizeof(int32_t), t->stream));
    if (X.nw > 0) {
        hipLaunchKernelGGL(k_cond_release, dim3(grid_for(X.nw, 256)), dim3(256), 0, t->stream, X, (QE *)t->queue[0], t->counters + CS_FRONTIER);
        hipLaunchKernelGGL(k_cond_nan_interior, dim3(1), dim3(1024), 0, t->stream, X);
    }
    PYDEM_TRY(cinc_cascade(t, X.C, dbg));
    t->cond_pending = false;
    return 0;
}

int stage_edge_catchup(pydem_tile *t)
{
    if (!(t->einc_ready && t->cond_live && t->cond_pending)) return 0;
    HIP_TRY(hipSetDevice(t->device));
    CascadeDbg dbg;
    PYDEM_TRY(cond_catchup(t, 1, &dbg));
    if (getenv("PYDEM_EDGE_DEBUG"))
        fprintf(stderr, "condensed edge catch-up (interior cascade): %d levels, %d by the level kernels, %d hand-overs\n", dbg.levels, dbg.wide, dbg.handovers);
    return 0;
}

int stage_edge_round_inc(pydem_tile *t, const pydem_options *opt, const double *const data[4], const uint8_t *const done[4],
                         const uint8_t *const todo[4])
{
    if (opt->apply_uca_limit_edges) {
        // edge_done is then more than "not downstream of a 'todo' inlet" (:977-980): the counts below would be wrong
        pydem_set_error("incremental edge rounds do not support apply_uca_limit_edges; use pydem_uca_edge_update");
        return -6;
    }
    // The counts of the incremental form assume that the cells that are not done form a DAG.  A tile with circular drainage
    // (the re-seed replay ran in its sweep: cells on and below a loop never count down to zero, while the reference's masks
    // only ask whether a 'todo' inlet lies upstream) runs the plain round instead; so does a tile resumed from the store,
    // whose sweep did not run in this process.
    if (t->circular_cells != 0) return stage_edge_update(t, opt, data, done, todo);
    const double t_begin = host_now_ms();
    const int n = (int)t->n, m = (int)t->m;
    const int L = n > m ? n : m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    t->einc_round++;
    IncArgs E;
    PYDEM_TRY(einc_args(t, E));
    PYDEM_TRY(tile_alloc(t, &t->s_data, (size_t)L * 4));
    PYDEM_TRY(tile_alloc(t, &t->s_flags, (size_t)L * 8));
    if (!t->einc_ready) { PYDEM_TRY(einc_prepare(t, E)); PYDEM_TRY(cond_build(t)); }
    // strips -> device (left, right, top, bottom), padded to L entries each (pinned staging: the copies are asynchronous);
    // data == NULL: the edge board's evaluation kernel has already written them (comm.hip)
    if (data) {
        if (t->h_strip_cap < (size_t)L) {
            if (t->h_strip_d) { (void)hipHostFree(t->h_strip_d); (void)hipHostFree(t->h_strip_f); }
            HIP_TRY(hipHostMalloc((void **)&t->h_strip_d, (size_t)L * 4 * sizeof(double)));
            HIP_TRY(hipHostMalloc((void **)&t->h_strip_f, (size_t)L * 8));
            t->h_strip_cap = (size_t)L;
        }
        double *hd = t->h_strip_d;
        uint8_t *hf = t->h_strip_f;
        for (int s = 0; s < 4; s++) {
            const int len = s < 2 ? n : m;
            for (int k = 0; k < len; k++) {
                hd[(size_t)s * L + k] = data[s][k];
                hf[(size_t)s * L + k] = done[s][k] != 0;
                hf[(size_t)(4 + s) * L + k] = todo[s][k] != 0;
            }
        }
        HIP_TRY(hipMemcpyAsync(t->s_data, hd, (size_t)L * 4 * 8, hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipMemcpyAsync(t->s_flags, hf, (size_t)L * 8, hipMemcpyHostToDevice, t->stream));
    }
    HIP_TRY(hipMemsetAsync(t->counters, 0, CS_WINDOW * sizeof(int32_t), t->stream));
#ifdef PYDEM_EINC_PROF
    HIP_TRY(hipMemsetAsync(t->counters + CS_EINC_PROF, 0, 8 * sizeof(int32_t), t->stream));
#endif
    CascadeDbg dbg;
    if (t->einc_compact && t->cond_live) {
        // condensed form: seeds + NaN flood + cascade on the watched nodes, two launches and no host look (the edge board's
        // pack kernels follow on the same stream); the interior catches up later (stage_edge_catchup / the flush)
        CondArgsE X;
        PYDEM_TRY(cond_args(t, X));
        hipLaunchKernelGGL(k_cond_seed, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, X, t->s_data, t->s_flags,
                           t->s_flags + (size_t)4 * L, L);
        hipLaunchKernelGGL(k_cond_run, dim3(1), dim3(COND_THREADS), 0, t->stream, X);
        t->cond_pending = true;
        HIP_TRY(hipGetLastError());
        static int sync_rounds = -1;       // PYDEM_EDGE_SYNC=1: wait for the round (per-round timings of tools/pm_multitile_timing.py)
        if (sync_rounds < 0) { const char *e = getenv("PYDEM_EDGE_SYNC"); sync_rounds = e ? atoi(e) : 0; }
        if (data || sync_rounds || getenv("PYDEM_EDGE_DEBUG")) {
            HIP_TRY(hipStreamSynchronize(t->stream));            // (host strips: the pinned staging is reused by the next round)
            if (getenv("PYDEM_EDGE_DEBUG")) {
                int32_t lv[3];
                HIP_TRY(hipMemcpy(lv, t->cond_cnt, sizeof(lv), hipMemcpyDeviceToHost));
                fprintf(stderr, "condensed edge round: %d levels on %d nodes; %.3f ms\n", lv[2], t->cond_nw, host_now_ms() - t_begin);
            }
        }
        return 0;
    }
    if (t->einc_compact) {
        CIncArgs C;
        PYDEM_TRY(cinc_args(t, C));
        hipLaunchKernelGGL(k_cinc_seed, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, C, t->s_data, t->s_flags,
                           t->s_flags + (size_t)4 * L, L, (QE *)t->queue[0], t->counters + CS_FRONTIER);
        hipLaunchKernelGGL(k_cinc_nan_flood, dim3(1), dim3(1024), 0, t->stream, C);
        PYDEM_TRY(cinc_cascade(t, C, &dbg));
    } else {
        hipLaunchKernelGGL(k_einc_seed, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, E, t->s_data, t->s_flags,
                           t->s_flags + (size_t)4 * L, L, (QE *)t->queue[0], t->counters + CS_FRONTIER);
        hipLaunchKernelGGL(k_einc_nan_flood, dim3(1), dim3(1024), 0, t->stream, E);
        PYDEM_TRY(einc_cascade(t, E, &dbg));
    }
    if (getenv("PYDEM_EDGE_DEBUG"))
        fprintf(stderr, "incremental edge round (%s): %d levels, %d by the level kernels, %d hand-overs; %.3f ms\n", t->einc_compact ? "compact" : "cell-indexed",
                dbg.levels, dbg.wide, dbg.handovers, host_now_ms() - t_begin);
#ifdef PYDEM_EINC_PROF
    if (getenv("PYDEM_EDGE_DEBUG")) {
        int32_t pr[8];
        HIP_TRY(hipMemcpy(pr, t->counters + CS_EINC_PROF, sizeof(pr), hipMemcpyDeviceToHost));
        fprintf(stderr, "   levels by frontier width <=8 / <=64 / <=512 / more: %d %d %d %d; us: %.0f %.0f %.0f %.0f\n", pr[0], pr[1], pr[2], pr[3],
                pr[4] * 0.01, pr[5] * 0.01, pr[6] * 0.01, pr[7] * 0.01);
    }
#endif
    return 0;
}

// Queued waves of the fix-up (pydem_board_run_waves, comm.hip): can this tile's next round be queued without the host knowing
// whether it will run?  Only the condensed form qualifies (two launches, no host look), after the tile's first round has
// built it.
bool tile_edge_queue_ready(const pydem_tile *t)
{
    return t->einc_ready && t->einc_compact && t->cond_live && t->circular_cells == 0 && t->s_data && t->s_flags;
}

// Entry of the queued waves' tile table (opaque to comm.hip): the condensed round of tile t, run only while bit `bit` of the
// device word *gate is set (the members of a queued wave are chosen on the device); the strips are in the tile's buffers
// (written by the board's evaluation kernel).  The seed stamp is *round_base + *round_add + 1 (mod 65535), both read on the
// device: the launches can be captured in a graph and replayed wave after wave.  The caller advances the tile's round
// counter by the waves it ran (tile_edge_rounds_ran).
size_t tile_edge_queue_desc_bytes() { return sizeof(QTile); }

int tile_edge_queue_desc(pydem_tile *t, void *out, const unsigned long long *gate, int bit, const unsigned long long *round_base,
                         const unsigned long long *round_add, int64_t *nper)
{
    if (!tile_edge_queue_ready(t)) { pydem_set_error("queued edge round: the tile's condensed fix-up state is not built"); return -3; }
    const int n = (int)t->n, m = (int)t->m;
    QTile q;
    memset(&q, 0, sizeof(q));
    PYDEM_TRY(cond_args(t, q.X));
    q.X.gate = gate; q.X.gate_bit = bit; q.X.round_base = round_base; q.X.round_add = round_add;
    q.sdata = t->s_data; q.sflags = t->s_flags; q.L = n > m ? n : m;
    q.nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    *nper = q.nper;
    memcpy(out, &q, sizeof(q));
    return 0;
}

// the rounds of `count` tiles (device table d_q), two launches on stream s
int stage_edge_rounds_queued(hipStream_t s, const void *d_q, int count, int64_t max_nper)
{
    if (count <= 0) return 0;
    hipLaunchKernelGGL(k_cond_seed_q, dim3((unsigned)cdiv(max_nper, 128), (unsigned)count), dim3(128), 0, s, (const QTile *)d_q);
    hipLaunchKernelGGL(k_cond_run_q, dim3((unsigned)count), dim3(COND_THREADS), 0, s, (const QTile *)d_q);
    return 0;
}

unsigned long long tile_edge_round_counter(const pydem_tile *t) { return (unsigned long long)t->einc_round; }

void tile_edge_rounds_ran(pydem_tile *t, int waves)
{
    t->einc_round += waves;
    if (waves > 0) t->cond_pending = true;
}

int stage_edge_flush(pydem_tile *t)
{
    if (!t->einc_ready) return 0;
    const int n = (int)t->n, m = (int)t->m;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    if (t->einc_compact && t->cond_live) {
        // condensed form: the interior catches up with what is done, the remaining inlets let go on the watched graph
        // (nothing becomes 'done' any more), and the interior follows once more
        const double t_flush0 = host_now_ms();
        CascadeDbg dbg[2];
        PYDEM_TRY(cond_catchup(t, 1, &dbg[0]));
        CondArgsE X;
        PYDEM_TRY(cond_args(t, X));
        X.C.set_done = 0;
        hipLaunchKernelGGL(k_cond_release_todo, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, X);
        hipLaunchKernelGGL(k_cond_run, dim3(1), dim3(COND_THREADS), 0, t->stream, X);
        PYDEM_TRY(cond_catchup(t, 0, &dbg[1]));
        t->einc_ready = false; t->cond_live = false;
        if (getenv("PYDEM_EDGE_DEBUG")) {
            HIP_TRY(hipStreamSynchronize(t->stream));
            int32_t tot[6];
            HIP_TRY(hipMemcpy(tot, t->cond_cnt, sizeof(tot), hipMemcpyDeviceToHost));
            fprintf(stderr, "condensed edge rounds: flush (interior cascade) %.3f ms; %d rounds ran on the watched graph, %d levels, %d nodes finished; "
                    "interior: %d + %d levels, %d by the level kernels, %d hand-overs\n",
                    host_now_ms() - t_flush0, tot[4], tot[3], tot[5], dbg[0].levels, dbg[1].levels, dbg[0].wide + dbg[1].wide, dbg[0].handovers + dbg[1].handovers);
        }
        return 0;
    }
    HIP_TRY(hipMemsetAsync(t->counters, 0, CS_WINDOW * sizeof(int32_t), t->stream));
    CascadeDbg dbg;
    if (t->einc_compact) {
        CIncArgs C;
        PYDEM_TRY(cinc_args(t, C));
        C.set_done = 0;
        hipLaunchKernelGGL(k_cinc_release_todo, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, C, (QE *)t->queue[0], t->counters + CS_FRONTIER);
        PYDEM_TRY(cinc_cascade(t, C, &dbg));
    } else {
        IncArgs E;
        PYDEM_TRY(einc_args(t, E));
        E.set_done = 0;
        hipLaunchKernelGGL(k_einc_release_todo, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, E, (QE *)t->queue[0], t->counters + CS_FRONTIER);
        PYDEM_TRY(einc_cascade(t, E, &dbg));
    }
    if (getenv("PYDEM_EDGE_DEBUG"))
        fprintf(stderr, "incremental edge rounds (%s): flush %d levels, %d by the level kernels, %d hand-overs\n", t->einc_compact ? "compact" : "cell-indexed",
                dbg.levels, dbg.wide, dbg.handovers);
    t->einc_ready = false;              // counts and deltas are spent: the next incremental round starts from the masks again
    return 0;
}

