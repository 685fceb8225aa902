// flowacc_rev.hip -- K10: reverse accumulation on the tile's D-infinity flow graph (TauDEM's DinfUpDependence and DinfRevAccum;
// no counterpart in the reference; semantics: include/pydem_hip.h, pydem_rev_accum): a linear (op 0) or max (op 1) recursion
// over the OUT-edges, swept from the outlets to the sources like the downslope distance of flowdist.hip.
//
//     V[c] = seed[c] + sum_e w_e * V[v_e]      (op 0; not normalised: flow that leaves the tile reaches nothing inside it)
//     V[c] = max(seed[c], max_e V[v_e])        (op 1)
//
// over the out-edges e = c -> v_e in the order of dd_for_out_edges.  A cell is open until every cell its out-edges lead to is
// final; then ONE lane finishes it by pulling their final values: no floating-point atomics, and a value does not depend on the
// schedule that produced it.  The sweep's own parts are the recursion, the classification of a cell at the start and the rounds
// of a tile visit; everything else -- state, encoding, counters, switches, the visit frame, the init and level kernels, the
// queue of a reverse sweep (k_dd_recount, dd_release), the host's schedule -- is the engine's (flowdist.h).  The seed is one more
// plane of the call's own.
//
//   the init kernel (RevClassify): NaN where the elevation is NaN, absorb_value on the absorbing cells, the seed on the cells
//   without an out-edge (all three final), the open pattern elsewhere.
//
//   tile passes (k_ra_tiles): a drained pit with pit edges only is finished at load time when all its drains are final from an
//   earlier pass; a cell with regular and pit out-edges is left to the queue.  A cell's work is a multiply-add or a max of at
//   most two LDS values and its seed, which stays in a register with the cell's proportion: no edge cost, no hypot, no
//   division.  A finished value lives in the cell's LDS slot until the store (68 VGPRs, no scratch, 11.8 KB LDS).
//
//   the queue (k_dd_recount, k_flow_level): reverse Kahn; a level finishes its cells with the full merge of regular and pit
//   edges (RevFinish), then releases the upstream counts (dd_release).
#include "flowdist.h"

namespace {

// The switch point of the tile passes: the cells a visit has to finish on average for another pass to beat the queue.  A visit
// stages what k_dd_tiles stages (value and stamp of tile + halo: 12 B per cell) plus 8 B of seed per open cell it owns, and
// its rounds are cheaper (no cost term, no division).  Measured on the 16384^2 bench tile (profiles/rev_accum_cost.txt): with
// the distance's 16 the dependence on the streams takes 74.6 ms and every value from 0 to 8 gives 73.1-73.3 ms; without an
// absorbing set only the cells without an out-edge are final at the start, the FIRST pass -- which visits every tile -- finishes
// 15.2 cells per visit, and 16 hands 264 M cells to the queue (1011 levels, 422 ms) where 0 to 8 stay with the passes (229-230
// ms, at most 10 cells left to the queue).  4 leaves the first pass a margin of 4 x on that tile.
constexpr int64_t RA_MIN_PER_VISIT = 4;

// the recursion of one cell: the seed first, then the out-edges in their fixed order
struct RevAcc {
    double acc = 0.0, hi;
    bool nan;
};
__device__ __forceinline__ RevAcc ra_start(double seed) { RevAcc S; S.hi = seed; S.nan = seed != seed; return S; }
__device__ __forceinline__ void ra_add(RevAcc &S, int op, double w, double v)
{
    if (op == 0) S.acc += w * v;
    else { S.nan = S.nan || v != v; S.hi = v > S.hi ? v : S.hi; }
}
// (op 0: a NaN operand makes the sum NaN by itself; every NaN is stored canonical -- no arithmetic here produces DD_OPEN_HI)
__device__ __forceinline__ double ra_result(const RevAcc &S, int op, double seed)
{
    double r = op == 0 ? seed + S.acc : S.hi;
    if (r != r || (op != 0 && S.nan)) r = dd_nan();
    return r;
}

// the value of an open cell whose out-neighbours are all final, from the result plane (the level kernel's Finish)
struct RevFinish {
    int op;
    const double *seed;
    __device__ __forceinline__ double operator()(const DistArgs &A, int32_t c, uint32_t cw) const
    {
        const double sd = seed ? seed[c] : 0.0;
        RevAcc S = ra_start(sd);
        dd_for_out_edges(A, c, cw, [&](int32_t dst, int, int, double w) { ra_add(S, op, w, A.D[dst]); });
        return ra_result(S, op, sd);
    }
};

// NaN elevations: NaN; absorbing cells: absorb_value; cells without an out-edge: their seed; the others are open
struct RevClassify {
    const double *seed;
    const uint8_t *absorb;
    double absorb_value;
    __device__ __forceinline__ bool operator()(const DistArgs &A, int32_t c, int, int, uint32_t cw, double &value) const
    {
        const double z = A.elev[c];
        value = dd_nan();
        if (z == z) {
            if (absorb && absorb[c] != 0) value = absorb_value;
            else if (cw & (CI_OUT1 | CI_OUT2 | CI_PIT_OUT)) return true;
            else {
                const double sd = seed ? seed[c] : 0.0;
                value = sd == sd ? sd : dd_nan();
            }
        }
        return false;
    }
};

// ---- tile passes (the frame and its rules: flowdist.h; which cells wait for what: k_dd_tiles)
__global__ __launch_bounds__(256) void k_ra_tiles(DistArgs A, int op, const double *__restrict__ seed, int32_t pass, int tiles_x, int tiles_y,
                                                  int32_t *tile_state)
{
    __shared__ double Dl[DD_H * DD_H];
    __shared__ uint16_t Fl[DD_H * DD_H];
    __shared__ int32_t s_done, s_open;
    const TileVisit V = dd_visit_begin(tile_state, pass, tiles_x, tiles_y);
    if (!V.run) return;
    dd_stage(A, pass, V, Dl, Fl, s_done, s_open);
    const int32_t *stamp = A.queue;
    int idx[4];
    uint32_t dst[4];                                    // LDS slots of the two destinations, + 1 (0: no such edge): first | second << 16
    double pr[4], sd[4];                                // proportion (the weight of the facet's first neighbour) and seed
    bool open[4], pend[4], swap[4];                     // swap: the facet's SECOND neighbour is the lower cell (comes first)
    int n_open = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const CellSlot sl = dd_slot(k, V);
        idx[k] = sl.idx;
        open[k] = false; pend[k] = false; swap[k] = false; dst[k] = 0; pr[k] = sd[k] = 0.0;
        if (!dd_slot_open(A, sl, Fl)) continue;
        const int32_t c = dd_slot_cell(A, sl);
        n_open++;
        const uint32_t cw = A.cinfo[c];
        const bool regular = (cw & (CI_OUT1 | CI_OUT2)) != 0;
        if (regular && (cw & CI_PIT_OUT)) continue;
        sd[k] = seed ? seed[c] : 0.0;
        if (!regular) {
            RevAcc S = ra_start(sd[k]);
            bool settled = true;
            for (PitBlock b = dd_pit_block(A.pit_src, A.n_pit, c); b.more(); b.e++) {
                const int32_t pd = A.pit_dst[b.e];
                settled = settled && stamp[pd] < pass;
                ra_add(S, op, A.pit_w[b.e], A.D[pd]);
            }
            // (the value waits in LDS behind the cell's open flag: nobody reads it before round 1 has set the flag)
            if (settled) { pend[k] = true; Dl[idx[k]] = ra_result(S, op, sd[k]); open[k] = true; }
            continue;
        }
        pr[k] = A.prop[c];
        const Facet f = dd_facet_sorted(A, cw, pr[k]);
        swap[k] = f.swapped;
        if (f.a.has) dst[k] = (uint32_t)(idx[k] + f.a.di * DD_H + f.a.dj + 1);
        if (f.b.has) dst[k] |= (uint32_t)(idx[k] + f.b.di * DD_H + f.b.dj + 1) << 16;
        open[k] = true;
    }
    // the rounds (their invariant: flowdist.h).  The evaluation is a multiply-add (or a compare) per edge: it runs per cell
    // slot, under the slot's predicate.  A finished value goes to the cell's LDS slot only; it is read back for the store.
    unsigned finished = 0;
    for (unsigned r = 1;; r++) {
        unsigned fresh = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!open[k]) continue;
            if (!pend[k]) {
                const int d1 = (int)(dst[k] & 0xFFFFu) - 1, d2 = (int)(dst[k] >> 16) - 1;
                if (!((d1 < 0 || Fl[d1] < r) && (d2 < 0 || Fl[d2] < r))) continue;
                RevAcc S = ra_start(sd[k]);
                if (d1 >= 0) ra_add(S, op, swap[k] ? 1 - pr[k] : pr[k], Dl[d1]);
                if (d2 >= 0) ra_add(S, op, swap[k] ? pr[k] : 1 - pr[k], Dl[d2]);
                Dl[idx[k]] = ra_result(S, op, sd[k]);
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

}  // namespace

extern "C" int pydem_rev_accum(pydem_tile *t, int op, const double *seed, const uint8_t *absorb, double absorb_value, double *out, double *ms,
                               int64_t *levels, int64_t *n_unresolved)
{
    PYDEM_TRY(dist_check_tile(t, "pydem_rev_accum"));
    if (op < 0 || op > 1) { pydem_set_error("pydem_rev_accum: op %d out of range (0 sum, 1 max)", op); return -2; }
    if (op == 1 && !seed) { pydem_set_error("pydem_rev_accum: op 1 (max) needs a seed"); return -2; }
    if (!(absorb_value - absorb_value == 0.0)) { pydem_set_error("pydem_rev_accum: absorb_value must be finite (got %g)", absorb_value); return -2; }
    PYDEM_TRY(dist_check_graph(t, "pydem_rev_accum"));
    if (absorb) PYDEM_TRY(dist_upload(t, &t->dd_mask, absorb));
    if (seed) PYDEM_TRY(dist_upload(t, &t->ra_seed, seed));
    DistArgs A;
    PYDEM_TRY(dist_state(t, A, 0, 0));
    const double *sd = seed ? (const double *)t->ra_seed : (const double *)nullptr;
    const uint8_t *ab = absorb ? (const uint8_t *)t->dd_mask : (const uint8_t *)nullptr;
    return dist_sweep<dd_release>(t, "rev_accum", RA_MIN_PER_VISIT, A, RevClassify{sd, ab, absorb_value}, RevFinish{op, sd}, k_dd_recount,
        [&](dim3 grid, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state) {
            hipLaunchKernelGGL(k_ra_tiles, grid, dim3(256), 0, t->stream, A, op, sd, pass, tiles_x, tiles_y, tile_state);
        }, out, ms, levels, n_unresolved);
}
