// flowdist_up.hip -- K9: upslope flow-path distance on the tile's D-infinity flow graph (TauDEM's DinfDistUp; no counterpart in
// the reference; semantics: include/pydem_hip.h, pydem_dist_up): the FORWARD (divide-to-outlet) sweep of the path statistic
// that flowdist.hip sweeps in reverse.  Its `max` is the longest flow path into a cell.
//
// A cell is open until every cell with an edge into it is final; then ONE lane finishes it: it PULLS the final values of its
// in-neighbours in a fixed order (ascending source, a regular edge before a pit edge from the same source), so there are no
// floating-point atomics and a value does not depend on the schedule that produced it.  The in-neighbours of a cell are bits
// 0-7 of its graph word (NW N NE W E SW S SE, which is ascending cell order) and its block of the pit in-list; the weight of
// a regular in-edge from u is p[u] when the cell is u's first (cardinal) facet neighbour and 1 - p[u] when it is the second
// (diagonal) one; the cost is dd_cost with u as the source.  State, encoding, counters, switches, the frame of a tile visit,
// the init and level kernels and the host's schedule are the engine's (flowdist.h): a call overwrites the other sweeps' result.
//
//   the init kernel (UpClassify, flowdist.h): NaN where the elevation is NaN and, under edge_nan, on the tile's border and
//   beside a NaN elevation; 0 where nothing flows in; the open pattern and the stamp elsewhere.
//
//   tile passes (k_du_tiles).  A cell has up to eight regular in-edges (the reverse sweep: two out-edges), so their weights and
//   costs do not fit in registers next to four cells' state; what is staged instead is what they are made of, for tile + halo:
//   value (8 B), proportion (8 B), elevation (8 B, not loaded for kind h), the round flag (2 B) and the spacing of the 34
//   rows -- 30.9 KB, which would let five workgroups share a CU's 160 KB; the 158 VGPRs of the inlined evaluation (eight
//   edges, hypot) allow three (3 wavefronts per SIMD, no scratch).  A cell's weights and costs are computed when it is
//   finished, from LDS alone: once per cell and call, where operands computed at load time would be computed again at every
//   visit of the tile that leaves the cell open, and no round waits for global memory.  The exception is a cell with pit
//   in-edges (a drain: about one per pit): it is opened only when all its pits are final from an earlier pass, and its lane
//   then reads their values and list entries from global memory in the round that finishes it.
//
//   the queue (k_du_recount and du_release of flowdist.h, k_flow_level): plain Kahn.  k_du_recount writes the number of open
//   in-neighbours into every open cell's slot and appends the cells with none; a level finishes the cells the previous one appended, then
//   takes one off the counts of the open cells its one or two regular out-edges and its pit out-edges lead to (integer
//   atomics), and the lane whose decrement is the last appends that cell.  A value is always written in a launch before the
//   one that reads it.
#include "flowdist.h"

namespace {

// The switch point of the forward sweep.  What a visit costs is what it stages: 28 B per cell of block + halo here (value,
// proportion, elevation, stamp) against 12 B in the reverse sweep's (value, stamp), whose switch point of 16 cells per visit
// was measured; the queue's cost per cell is the same in both directions.  16 * 28 / 12 = 37.
constexpr int64_t DU_MIN_PER_VISIT = 37;

// The value of the open cell c = (i, j) whose in-neighbours are all final.  `reg(d, u, p, du, zu, dx, dy)` hands out what a
// regular in-edge from neighbour d (cell u) needs: u's proportion, value, elevation and the cell size of u's row -- from the
// planes (the queue) or from LDS (the tile passes); pit edges always come from the planes.  zc: elevation of c (kind != h).
template <class Reg>
__device__ __forceinline__ double du_gather(const DistArgs &A, int32_t c, uint32_t cw, int i, int j, double zc, Reg reg)
{
    DistAcc S;
    PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c, (cw & CI_PIT_IN) != 0);
    auto pit = [&](int64_t k) {
        const int32_t u = A.pin_src[k];
        const int ui = u / A.m, uj = u - ui * A.m;
        dd_add(S, A.pin_w[k], A.D[u] + dd_cost(A.kind, i - ui, j - uj, A.dX2[ui], A.dY2[ui], A.kind != 0 ? A.elev[u] : 0.0, zc));
    };
#pragma unroll
    for (int d = 0; d < 8; d++) {
        if (!(cw & (1u << d))) continue;
        const int32_t u = c + NB_DI[d] * A.m + NB_DJ[d];
        for (; b.more() && A.pin_src[b.e] < u; b.e++) pit(b.e);
        double p, du, zu, dx, dy;
        reg(d, u, p, du, zu, dx, dy);
        dd_add(S, du_cardinal(d) ? p : 1 - p, du + dd_cost(A.kind, -NB_DI[d], -NB_DJ[d], dx, dy, zu, zc));
    }
    for (; b.more(); b.e++) pit(b.e);
    return dd_result(A.stat, S);
}

// ---- tile passes (the frame and its rules: flowdist.h)
__global__ __launch_bounds__(256) void k_du_tiles(DistArgs A, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state)
{
    __shared__ double Dl[DD_H * DD_H], Pl[DD_H * DD_H], El[DD_H * DD_H];
    __shared__ double Xl[DD_H], Yl[DD_H];
    __shared__ uint16_t Fl[DD_H * DD_H];
    __shared__ int32_t s_done, s_open;
    const TileVisit V = dd_visit_begin(tile_state, pass, tiles_x, tiles_y);
    if (!V.run) return;
    const int i0 = V.i0, j0 = V.j0;
    if (threadIdx.x < DD_H) {
        const int gi = i0 + (int)threadIdx.x;
        const bool in = gi >= 0 && gi < A.n;
        Xl[threadIdx.x] = in ? A.dX2[gi] : 0.0; Yl[threadIdx.x] = in ? A.dY2[gi] : 0.0;
    }
    double p = 0.0, z = 0.0;                            // proportion and elevation of the slot being staged (0 off the grid)
    dd_stage(A, pass, V, Dl, Fl, s_done, s_open,
             [&](int32_t c) { p = A.prop[c]; if (A.kind != 0) z = A.elev[c]; },
             [&](int t) { Pl[t] = p; El[t] = z; p = z = 0.0; });
    const int32_t *stamp = A.queue;
    int32_t cell[4];
    int idx[4];
    uint32_t word[4], rem[4];
    double val[4];
    bool open[4];
    int n_open = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const CellSlot sl = dd_slot(k, V);
        idx[k] = sl.idx;
        open[k] = false; cell[k] = 0; word[k] = 0; rem[k] = 0; val[k] = 0.0;
        if (!dd_slot_open(A, sl, Fl)) continue;
        const int32_t c = dd_slot_cell(A, sl);
        cell[k] = c;
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
    // which in-neighbours it has seen final and asks only for the others; the evaluation runs on selected operands (DD_SEL).
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
            if (w == 0) fresh |= 1u << k;
        }
        unsigned todo = fresh;
        while (todo) {
            const int k = __ffs((int)todo) - 1;
            todo &= todo - 1;
            const int ix = DD_SEL(idx, k);
            const int32_t c = DD_SEL(cell, k);
            const int li = ix / DD_H;
            const double v = du_gather(A, c, DD_SEL(word, k), i0 + li, j0 + ix - li * DD_H, El[ix],
                [&](int d, int32_t, double &p, double &du, double &zu, double &dx, double &dy) {
                    const int s = ix + NB_DI[d] * DD_H + NB_DJ[d];
                    p = Pl[s]; du = Dl[s]; zu = El[s]; dx = Xl[li + NB_DI[d]]; dy = Yl[li + NB_DI[d]];
                });
#pragma unroll
            for (int q = 0; q < 4; q++) val[q] = q == k ? v : val[q];
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (fresh & (1u << k)) {
                Dl[idx[k]] = val[k]; Fl[idx[k]] = (uint16_t)r;
                open[k] = false;
                finished |= 1u << k;
            }
        if (!__syncthreads_or(fresh != 0)) break;
    }
    dd_visit_end(A, pass, V, s_done, s_open, n_open, finished, [&](int k, const CellSlot &) { return cell[k]; },
                 [&](int k, const CellSlot &) { return val[k]; });
}

// the value of an open cell whose in-neighbours are all final, from the planes (the level kernel's Finish)
struct UpFinish {
    __device__ __forceinline__ double operator()(const DistArgs &A, int32_t v, uint32_t cw) const
    {
        const int i = v / A.m;
        return du_gather(A, v, cw, i, v - i * A.m, A.kind != 0 ? A.elev[v] : 0.0,
            [&](int d, int32_t u, double &p, double &du, double &zu, double &dx, double &dy) {
                p = A.prop[u]; du = A.D[u]; zu = A.kind != 0 ? A.elev[u] : 0.0; dx = A.dX2[i + NB_DI[d]]; dy = A.dY2[i + NB_DI[d]];
            });
    }
};

}  // namespace

extern "C" int pydem_dist_up(pydem_tile *t, int kind, int stat, int edge_nan, double *out, double *ms, int64_t *levels, int64_t *n_unresolved)
{
    PYDEM_TRY(dist_check_tile(t, "pydem_dist_up"));
    if (kind < 0 || kind > 2 || stat < 0 || stat > 2) { pydem_set_error("pydem_dist_up: kind %d / stat %d out of range (0..2)", kind, stat); return -2; }
    PYDEM_TRY(dist_check_graph(t, "pydem_dist_up"));
    DistArgs A;
    PYDEM_TRY(dist_state(t, A, kind, stat));
    return dist_sweep<du_release>(t, "dist_up", DU_MIN_PER_VISIT, A, UpClassify{edge_nan}, UpFinish{}, k_du_recount,
        [&](dim3 grid, int32_t pass, int tiles_x, int tiles_y, int32_t *tile_state) {
            hipLaunchKernelGGL(k_du_tiles, grid, dim3(256), 0, t->stream, A, pass, tiles_x, tiles_y, tile_state);
        }, out, ms, levels, n_unresolved);
}
