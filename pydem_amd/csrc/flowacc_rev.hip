// flowacc_rev.hip -- K10: reverse accumulation on the tile's D-infinity flow graph (TauDEM's DinfUpDependence and DinfRevAccum;
// no counterpart in the reference; semantics: include/pydem_hip.h, pydem_rev_accum): a linear (op 0) or max (op 1) recursion
// over the OUT-edges, swept from the outlets to the sources like the downslope distance of flowdist.hip.
//
//     V[c] = seed[c] + sum_e w_e * V[v_e]      (op 0; not normalised: flow that leaves the tile reaches nothing inside it)
//     V[c] = max(seed[c], max_e V[v_e])        (op 1)
//
// over the out-edges e = c -> v_e in ascending destination order, a regular edge before a pit edge to the same cell -- the
// order of dd_finish.  A cell is open until every cell its out-edges lead to is final; then ONE lane finishes it by pulling
// their final values: no floating-point atomics, and a value does not depend on the schedule that produced it.  State, encoding
// of an open cell, counters, switches and the host's schedule are those of pydem_dist_down (flowdist.h), and so are the two
// parts of the queue that depend on the graph alone (k_dd_recount, dd_release); the seed is one more plane of the call's own.
//
//   k_ra_init: NaN where the elevation is NaN, absorb_value on the absorbing cells, the seed on the cells without an out-edge
//   (all three final: stamp 0), the open pattern and DD_STAMP_OPEN elsewhere.
//
//   tile passes (k_ra_tiles), under the rules that make k_dd_tiles deterministic: one workgroup per 32 x 32 tile, four cells
//   per thread, final flags and values of tile + halo in LDS (11.8 KB), rounds to the fixed point with one barrier each, results
//   and stamps stored once after the rounds.  A cell outside the tile is final only if its stamp is from an EARLIER pass; a
//   drained pit with pit edges only is finished at load time when all its drains are final from an earlier pass; a cell with
//   regular and pit out-edges is left to the queue.  A cell's work is a multiply-add or a max of at most two LDS values and its
//   seed, which stays in a register with the cell's proportion: no edge cost, no hypot, no division.  A finished value lives in
//   the cell's LDS slot until the store (66 VGPRs, no scratch).
//
//   the queue (k_dd_recount, k_ra_level): reverse Kahn; a level finishes its cells with the full merge of regular and pit
//   edges, then releases the upstream counts (dd_release).
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

// the value of an open cell whose out-neighbours are all final, from the result plane: the merge of dd_finish
__device__ __forceinline__ double ra_finish(const DistArgs &A, int op, const double *__restrict__ seed, int32_t c, uint32_t cw)
{
    int nr = 0;
    int32_t rd[2]; double rw[2];
    if (cw & (CI_OUT1 | CI_OUT2)) {
        const int s = ci_section(cw);
        const double p = A.prop[c];
        if (cw & CI_OUT1) { rd[nr] = c + fe1r(s) * A.m + fe1c(s); rw[nr] = p; nr++; }
        if (cw & CI_OUT2) { rd[nr] = c + fe2r(s) * A.m + fe2c(s); rw[nr] = 1 - p; nr++; }
        if (nr == 2 && rd[1] < rd[0]) {
            const int32_t a = rd[0]; const double w = rw[0];
            rd[0] = rd[1]; rw[0] = rw[1];
            rd[1] = a; rw[1] = w;
        }
    }
    const double sd = seed ? seed[c] : 0.0;
    RevAcc S = ra_start(sd);
    int64_t e = A.n_pit;
    if (cw & CI_PIT_OUT) e = dd_lower_bound(A.pit_src, A.n_pit, c);
    int ir = 0;
    for (;;) {
        const bool hr = ir < nr, hp = e < A.n_pit && A.pit_src[e] == c;
        if (!hr && !hp) break;
        const int32_t pd = hp ? A.pit_dst[e] : 0;
        if (hr && (!hp || rd[ir] <= pd)) { ra_add(S, op, rw[ir], A.D[rd[ir]]); ir++; }
        else { ra_add(S, op, A.pit_w[e], A.D[pd]); e++; }
    }
    return ra_result(S, op, sd);
}

// NaN elevations, absorbing cells, cells without an out-edge (their seed), the open pattern and the stamps of the others
__global__ __launch_bounds__(256) void k_ra_init(DistArgs A, const double *__restrict__ seed, const uint8_t *__restrict__ absorb, double absorb_value)
{
    unsigned long long *n_open = reinterpret_cast<unsigned long long *>(A.ctr + DD_NOPEN);
    __shared__ int32_t s_open;
    if (threadIdx.x == 0) s_open = 0;
    __syncthreads();
    int32_t mine = 0;
    for (int i = blockIdx.y; i < A.n; i += gridDim.y)
    for (int j0 = blockIdx.x * blockDim.x; j0 < A.m; j0 += gridDim.x * blockDim.x) {
        const int j = j0 + (int)threadIdx.x;
        bool open = false;
        if (j < A.m) {
            const int32_t c = i * A.m + j;
            const uint32_t cw = A.cinfo[c];
            const double z = A.elev[c];
            double v = dd_nan();
            if (z == z) {
                if (absorb && absorb[c] != 0) v = absorb_value;
                else if (cw & (CI_OUT1 | CI_OUT2 | CI_PIT_OUT)) open = true;
                else {
                    const double sd = seed ? seed[c] : 0.0;
                    v = sd == sd ? sd : dd_nan();
                }
            }
            if (open) reinterpret_cast<uint2 *>(A.D)[c] = make_uint2(0u, DD_OPEN_HI);
            else A.D[c] = v;
            A.queue[c] = open ? DD_STAMP_OPEN : 0;
        }
        mine += open ? 1 : 0;
    }
    // one global atomic per workgroup, as in k_dd_init
    if (mine) atomicAdd(&s_open, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_open) atomicAdd(n_open, (unsigned long long)s_open);
}

// ---- tile passes
// One workgroup, one tile, four cells per thread.  A cell with regular out-edges waits for the flags of its one or two
// destinations in LDS; a drained pit (pit edges only) is finished when it is loaded if all its drains are final from an
// earlier pass; a cell with both kinds of edges is left to the queue.
__global__ __launch_bounds__(256) void k_ra_tiles(DistArgs A, int op, const double *__restrict__ seed, int32_t pass, int tiles_x, int tiles_y,
                                                  int32_t *tile_state)
{
    __shared__ double Dl[DD_H * DD_H];
    __shared__ uint16_t Fl[DD_H * DD_H];        // round of the visit in which the cell became final (0: before it, DD_FL_OPEN: not yet)
    __shared__ int32_t s_done, s_open;
    const int ntiles = tiles_x * tiles_y;
    int32_t *tile_open = tile_state, *prog_w = tile_state + (1 + (pass & 1)) * (int64_t)ntiles, *tile_done = tile_state + 3 * (int64_t)ntiles;
    const int32_t *prog_r = tile_state + (1 + ((pass - 1) & 1)) * (int64_t)ntiles;
    const int tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    if (pass > 1) {                                     // (uniform per workgroup: everything read here is from earlier launches)
        bool visit = false;
        if (tile_open[tile] > 0)
            for (int a = -1; a <= 1; a++)
                for (int b = -1; b <= 1; b++) {
                    const int yy = ty + a, xx = tx + b;
                    if (yy >= 0 && yy < tiles_y && xx >= 0 && xx < tiles_x && prog_r[yy * tiles_x + xx] == pass - 1) visit = true;
                }
        if (!visit) {
            if (threadIdx.x == 0) tile_done[tile] = -1;
            return;
        }
    }
    int32_t *stamp = A.queue;
    const int i0 = ty * DD_T - 1, j0 = tx * DD_T - 1;
    if (threadIdx.x == 0) { s_done = 0; s_open = 0; }
    for (int t = threadIdx.x; t < DD_H * DD_H; t += 256) {
        const int li = t / DD_H, lj = t - li * DD_H;
        const int gi = i0 + li, gj = j0 + lj;
        bool fin = false;
        double d = 0.0;
        if (gi >= 0 && gi < A.n && gj >= 0 && gj < A.m) {
            const int32_t c = gi * A.m + gj;
            fin = stamp[c] < pass;                      // (a stamp of this pass, written by whoever owns the cell, reads as open)
            if (fin) d = A.D[c];
        }
        Dl[t] = d; Fl[t] = fin ? (uint16_t)0 : DD_FL_OPEN;
    }
    __syncthreads();
    // this thread's cells: k-th cell = row (threadIdx.x / 32) + 8 k of the tile, column threadIdx.x % 32
    int idx[4];
    uint32_t dst[4];                                    // LDS slots of the two destinations, + 1 (0: no such edge): first | second << 16
    double pr[4], sd[4];                                // proportion (the weight of the facet's first neighbour) and seed
    bool open[4], pend[4], swap[4];                     // swap: the facet's SECOND neighbour is the lower cell (comes first)
    int n_open = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ti = (int)(threadIdx.x >> 5) + 8 * k, tj = (int)(threadIdx.x & 31);
        const int gi = i0 + 1 + ti, gj = j0 + 1 + tj;
        idx[k] = (ti + 1) * DD_H + tj + 1;
        open[k] = false; pend[k] = false; swap[k] = false; dst[k] = 0; pr[k] = sd[k] = 0.0;
        if (gi >= A.n || gj >= A.m || Fl[idx[k]] == 0) continue;
        const int32_t c = gi * A.m + gj;
        n_open++;
        const uint32_t cw = A.cinfo[c];
        const bool regular = (cw & (CI_OUT1 | CI_OUT2)) != 0;
        if (regular && (cw & CI_PIT_OUT)) continue;
        sd[k] = seed ? seed[c] : 0.0;
        if (!regular) {
            RevAcc S = ra_start(sd[k]);
            bool settled = true;
            for (int64_t e = dd_lower_bound(A.pit_src, A.n_pit, c); e < A.n_pit && A.pit_src[e] == c; e++) {
                const int32_t pd = A.pit_dst[e];
                settled = settled && stamp[pd] < pass;
                ra_add(S, op, A.pit_w[e], A.D[pd]);
            }
            // (the value waits in LDS behind the cell's open flag: nobody reads it before round 1 has set the flag)
            if (settled) { pend[k] = true; Dl[idx[k]] = ra_result(S, op, sd[k]); open[k] = true; }
            continue;
        }
        const int s = ci_section(cw);
        pr[k] = A.prop[c];
        // the facet's two neighbours in ascending cell order
        int ai = fe1r(s), aj = fe1c(s), bi = fe2r(s), bj = fe2c(s);
        bool ha = (cw & CI_OUT1) != 0, hb = (cw & CI_OUT2) != 0;
        if (bi * A.m + bj < ai * A.m + aj) {
            const int x = ai, y = aj; ai = bi; aj = bj; bi = x; bj = y;
            const bool h = ha; ha = hb; hb = h;
            swap[k] = true;
        }
        if (ha) dst[k] = (uint32_t)(idx[k] + ai * DD_H + aj + 1);
        if (hb) dst[k] |= (uint32_t)(idx[k] + bi * DD_H + bj + 1) << 16;
        open[k] = true;
    }
    // Rounds to the fixed point, one barrier each: a cell is ready in round r when its destinations became final in an
    // EARLIER round (flag < r), so what this round writes -- flags = r, values of cells nobody may read yet -- cannot change
    // what this round reads.  The evaluation is a multiply-add (or a compare) per edge: it runs per cell slot, under the
    // slot's predicate.  A finished value goes to the cell's LDS slot only; it is read back for the store after the rounds.
    unsigned finished = 0;
    for (unsigned r = 1;; r++) {                        // (at most 1024 rounds: every round but the last finishes a cell)
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
    // results leave once, after the rounds
    int n_done = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (finished & (1u << k)) {
            const int32_t c = (i0 + 1 + (int)(threadIdx.x >> 5) + 8 * k) * A.m + j0 + 1 + (int)(threadIdx.x & 31);
            A.D[c] = Dl[idx[k]]; stamp[c] = pass; n_done++;
        }
    if (n_open) atomicAdd(&s_open, n_open - n_done);
    if (n_done) atomicAdd(&s_done, n_done);
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_open[tile] = s_open;
        if (s_done) prog_w[tile] = pass;
        tile_done[tile] = s_done;                       // (summed by k_dd_pass_sum)
    }
}

// ---- queue: one level (the cells the level before appended; k_dd_recount of flowdist.h starts it)
__global__ __launch_bounds__(256) void k_ra_level(DistArgs A, int op, const double *__restrict__ seed)
{
    const int64_t lo = A.ctr[DD_LO], hi = A.ctr[DD_HI];
    for (int64_t base = lo + (int64_t)blockIdx.x * blockDim.x; base < hi; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = base + threadIdx.x;
        int32_t v = 0;
        uint32_t cw = 0;
        if (k < hi) {
            v = A.queue[k];
            cw = A.cinfo[v];
            A.D[v] = ra_finish(A, op, seed, v, cw);
        }
        dd_release(A, v, cw);
    }
}

}  // namespace

extern "C" int pydem_rev_accum(pydem_tile *t, int op, const double *seed, const uint8_t *absorb, double absorb_value, double *out, double *ms,
                               int64_t *levels, int64_t *n_unresolved)
{
    if (!t) { pydem_set_error("pydem_rev_accum: no tile"); return -2; }
    HIP_TRY(hipSetDevice(t->device));
    if (op < 0 || op > 1) { pydem_set_error("pydem_rev_accum: op %d out of range (0 sum, 1 max)", op); return -2; }
    if (op == 1 && !seed) { pydem_set_error("pydem_rev_accum: op 1 (max) needs a seed"); return -2; }
    if (!(absorb_value - absorb_value == 0.0)) { pydem_set_error("pydem_rev_accum: absorb_value must be finite (got %g)", absorb_value); return -2; }
    if (!t->graph_valid || !t->cinfo || !t->prop || !t->have[PYDEM_PROPORTION] || !t->have[PYDEM_ELEV] || !t->spacing_set) {
        pydem_set_error("pydem_rev_accum: no flow graph on this tile (pydem_uca / pydem_build_graph first)");
        return -3;
    }
    if (absorb) {
        PYDEM_TRY(tile_alloc(t, &t->dd_mask, (size_t)t->NN));
        PYDEM_TRY(tile_plane_copy(t, t->dd_mask, const_cast<uint8_t *>(absorb), (size_t)t->NN, false));
    }
    if (seed) {
        PYDEM_TRY(tile_alloc(t, &t->ra_seed, (size_t)t->NN));
        PYDEM_TRY(tile_plane_copy(t, t->ra_seed, const_cast<double *>(seed), (size_t)t->NN * 8, false));
    }
    DistArgs A;
    PYDEM_TRY(dist_state(t, A, 0, 0));
    const dim3 rows = dist_row_grid(t);
    const double *sd = seed ? (const double *)t->ra_seed : (const double *)nullptr;
    const uint8_t *ab = absorb ? (const uint8_t *)t->dd_mask : (const uint8_t *)nullptr;
    return dist_schedule(t, "rev_accum", RA_MIN_PER_VISIT, out, ms, levels, n_unresolved,
        [&] { hipLaunchKernelGGL(k_ra_init, rows, dim3(256), 0, t->stream, A, sd, ab, absorb_value); },
        [&](int pass, int tiles_x, int tiles_y, int32_t *tile_state) {
            hipLaunchKernelGGL(k_ra_tiles, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, t->stream, A, op, sd, (int32_t)pass, tiles_x, tiles_y, tile_state);
        },
        [&] { hipLaunchKernelGGL(k_dd_recount, rows, dim3(256), 0, t->stream, A); },
        [&](int grid) { hipLaunchKernelGGL(k_ra_level, dim3(grid), dim3(256), 0, t->stream, A, op, sd); });
}
