// flowdist.h -- the engine of the seven sweeps over the tile's D-infinity flow graph: the reverse path statistic (flowdist.hip,
// pydem_dist_down), the forward one (flowdist_up.hip, pydem_dist_up), the reverse accumulation (flowacc_rev.hip,
// pydem_rev_accum), the forward accumulation (flowacc_fwd.hip, pydem_fwd_accum), the forward and the reverse labelling of the
// stream network (streamnet.hip, pydem_stream_network), and the accumulation along the receiver tree (flowacc_tree.hip,
// pydem_tree_accum).  A sweep supplies what differs -- which cells are final at the start (a Classify), the value of a cell
// whose neighbours are final (a Finish; in the tile passes, its round loop) and which
// side of the graph it waits for -- and takes the rest from here, where every rule is written once:
//
//   the encoding of an open cell in the result plane, the argument block, the counter words, the wave-aggregated queue append;
//   the accumulator of a path statistic with its fixed operand order, the edge cost;
//   a cell's block of a sorted pit list (dd_pit_block), its facet neighbours in cell order (dd_facet_sorted) and its out-edges
//   in the order every reverse sweep pulls them in (dd_for_out_edges), its in-edges in the order every forward sweep does
//   (dd_for_in_edges);
//   the frame of a tile visit: whether it runs, the staging of tile + halo under the stamp rule, the geometry of a thread's
//   four cells, the store after the rounds and the tile's three words (dd_visit_begin, dd_stage, dd_slot, dd_visit_end);
//   the init and the level kernel (k_flow_init, k_flow_level), the queue of a reverse sweep (dd_release, k_dd_recount) and of
//   a forward one (du_release, k_du_recount), the cells a forward sweep starts from (UpClassify);
//   the host's checks, uploads, state and schedule (dist_check_tile, dist_check_graph, dist_upload, dist_state, dist_schedule, dist_sweep).
//
// One call at a time owns the state (pydem_tile::dd_*): a call overwrites the others' device result.
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
// (DD_USER: a 64-bit word the schedule zeroes with the block and never reads, for what a call counts after its sweep --
// streamnet.hip: the -1 of the basins)
enum : int { DD_LO = 0, DD_HI = 1, DD_TAIL = 2, DD_LEVELS = 3, DD_NOPEN = 4 /* 64-bit: [4..5] */, DD_PASSDONE = 6 /* 64-bit: [6..7] */,
             DD_VISITS = 8, DD_USER = 10 /* 64-bit: [10..11] */, DD_WORDS = 16 };

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

// The block of a sorted pit list whose key is `c`, walked with `for (PitBlock b = dd_pit_block(keys, n, c); b.more(); b.e++)`;
// has = false (the cell's graph word carries no pit flag): the empty block, without the search.
struct PitBlock {
    const int32_t *keys;
    int64_t n, e;
    int32_t c;
    __device__ __forceinline__ bool more() const { return e < n && keys[e] == c; }
};
__device__ __forceinline__ PitBlock dd_pit_block(const int32_t *__restrict__ keys, int64_t n, int32_t c, bool has = true)
{
    return PitBlock{keys, n, has ? dd_lower_bound(keys, n, c) : n, c};
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

// ---- a cell's out-edges
// one regular out-edge: offset of the facet neighbour, weight, whether the graph has the edge
struct FacetEdge { int di, dj; double w; bool has; };
// the facet's two neighbours in ascending cell order (a: the lower cell); swapped: a is the facet's SECOND neighbour (weight 1 - p)
struct Facet { FacetEdge a, b; bool swapped; };

__device__ __forceinline__ Facet dd_facet_sorted(const DistArgs &A, uint32_t cw, double p)
{
    const int s = ci_section(cw);
    const int ai = fe1r(s), aj = fe1c(s), bi = fe2r(s), bj = fe2c(s);       // (once each: the compiler does not merge two calls)
    Facet f = {{ai, aj, p, (cw & CI_OUT1) != 0}, {bi, bj, 1 - p, (cw & CI_OUT2) != 0}, false};
    if (bi * A.m + bj < ai * A.m + aj) { const FacetEdge x = f.a; f.a = f.b; f.b = x; f.swapped = true; }
    return f;
}

// f(dst, di, dj, w) for every out-edge c -> dst = c + (di, dj) of weight w, in the order every reverse sweep pulls them in:
// ascending destination, a regular edge before a pit edge to the same cell.  cw: the graph word of c.
template <class F>
__device__ __forceinline__ void dd_for_out_edges(const DistArgs &A, int32_t c, uint32_t cw, F f)
{
    const int i = c / A.m, j = c - i * A.m;
    int nr = 0, rdi[2], rdj[2];                         // (one array per field: an array of structs indexed by ir would go to LDS)
    double rw[2];
    if (cw & (CI_OUT1 | CI_OUT2)) {
        const Facet ft = dd_facet_sorted(A, cw, A.prop[c]);
        if (ft.a.has) { rdi[nr] = ft.a.di; rdj[nr] = ft.a.dj; rw[nr] = ft.a.w; nr++; }
        if (ft.b.has) { rdi[nr] = ft.b.di; rdj[nr] = ft.b.dj; rw[nr] = ft.b.w; nr++; }
    }
    PitBlock b = dd_pit_block(A.pit_src, A.n_pit, c, (cw & CI_PIT_OUT) != 0);
    for (int ir = 0;;) {
        const bool hr = ir < nr, hp = b.more();
        if (!hr && !hp) break;
        const int32_t rd = hr ? c + rdi[ir] * A.m + rdj[ir] : 0;
        const int32_t pd = hp ? A.pit_dst[b.e] : 0;
        if (hr && (!hp || rd <= pd)) { f(rd, rdi[ir], rdj[ir], rw[ir]); ir++; }
        else { const int pi = pd / A.m; f(pd, pi - i, pd - pi * A.m - j, A.pit_w[b.e]); b.e++; }
    }
}

// ---- a cell's in-edges
// neighbour d (bit d of the graph word: NW N NE W E SW S SE, ascending cell order) has the cell as its FIRST facet neighbour
// (weight p of the SOURCE) when it is a cardinal one, as its second (weight 1 - p) when it is a diagonal one
__device__ __forceinline__ bool du_cardinal(int d) { return NB_DI[d] == 0 || NB_DJ[d] == 0; }

// reg(d, u) for every regular in-edge u -> c from neighbour d and pit(k) for every entry k of the pit in-list whose destination
// is c, in the order every forward sweep pulls them in: ascending source, a regular edge before a pit edge from the same
// source.  cw: the graph word of c.
template <class Reg, class Pit>
__device__ __forceinline__ void dd_for_in_edges(const DistArgs &A, int32_t c, uint32_t cw, Reg reg, Pit pit)
{
    PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c, (cw & CI_PIT_IN) != 0);
#pragma unroll
    for (int d = 0; d < 8; d++) {
        if (!(cw & (1u << d))) continue;
        const int32_t u = c + NB_DI[d] * A.m + NB_DJ[d];
        for (; b.more() && A.pin_src[b.e] < u; b.e++) pit(b.e);
        reg(d, u);
    }
    for (; b.more(); b.e++) pit(b.e);
}

// ---- the frame of a tile visit
// One workgroup of 256 threads visits one 32 x 32 tile in a pass: it stages values and final flags of tile + halo in LDS, runs
// rounds to the fixed point with one barrier each, then stores what it finished with the pass number as stamp.  The rules:
//
//   stamps    a cell outside the workgroup's hands (the halo, the far end of a pit edge) is final only if its stamp is from an
//             EARLIER pass (stamp < pass; 0: final from the start, DD_STAMP_OPEN: open).  A stamp of the current pass -- written by
//             whoever owns the cell, in this launch -- reads as open, so a tile never reads what another workgroup writes in
//             the same launch and the set a pass finishes is the same in every run.
//   rounds    a cell is ready in round r only on flags < r: its neighbours became final in an EARLIER round, so what a round
//             writes -- flags = r, values of cells nobody may read yet -- cannot change what the round reads.  At most 1024
//             rounds: every round but the last finishes a cell.  The round loops are the sweeps' own (the kernels).
//   results   leave once, after the rounds (a barrier waits for the stores in flight: one store per round made every round as
//             long as a trip to memory).
//   visits    from the second pass on a tile is visited while it has open cells and it or one of its 8 neighbours finished
//             something in the pass before.  Four words per tile behind the counter block say so: open cells after its last
//             visit; for each parity of the pass number the last pass of that parity in which it finished something (this pass
//             writes one word while the workgroups around read the other); cells finished by its visit of the current pass, -1
//             if it was skipped (summed by k_dd_pass_sum: a counter all tiles add to would serialise them).
struct TileVisit {
    bool run;                                           // false: skipped, the workgroup returns (before any barrier)
    int tile, i0, j0;                                   // the tile's index; row and column of the halo's first cell
    int32_t *tile_open, *prog_w, *tile_done;
};

__device__ __forceinline__ TileVisit dd_visit_begin(int32_t *tile_state, int32_t pass, int tiles_x, int tiles_y)
{
    const int ntiles = tiles_x * tiles_y;
    const int32_t *prog_r = tile_state + (1 + ((pass - 1) & 1)) * (int64_t)ntiles;
    const int tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    TileVisit V = {true, tile, ty * DD_T - 1, tx * DD_T - 1,
                   tile_state, tile_state + (1 + (pass & 1)) * (int64_t)ntiles, tile_state + 3 * (int64_t)ntiles};
    if (pass > 1) {                                     // (uniform per workgroup: everything read here is from earlier launches)
        bool visit = false;
        if (V.tile_open[tile] > 0)
            for (int a = -1; a <= 1; a++)
                for (int b = -1; b <= 1; b++) {
                    const int yy = ty + a, xx = tx + b;
                    if (yy >= 0 && yy < tiles_y && xx >= 0 && xx < tiles_x && prog_r[yy * tiles_x + xx] == pass - 1) visit = true;
                }
        if (!visit) {
            if (threadIdx.x == 0) V.tile_done[tile] = -1;
            V.run = false;
        }
    }
    return V;
}

// Values and flags of tile + halo: Dl = the value of a final cell, Fl = the round of the visit in which the cell became final
// (0: before it, DD_FL_OPEN: not yet).  What else the sweep wants of a slot it stages in two steps: load(c) for a cell c on the grid,
// next to the value's load, and store(t) for every slot t, next to the value's store.  (One callable after the stamp test put its
// loads behind the value's: three trips to memory per slot where the parent had two, 0.5 % of a forward sweep.)  Clears the
// visit's two counters; ends with the barrier after which the slots may be read.
template <class Load, class Store>
__device__ __forceinline__ void dd_stage(const DistArgs &A, int32_t pass, const TileVisit &V, double *Dl, uint16_t *Fl,
                                         int32_t &s_done, int32_t &s_open, Load load, Store store)
{
    const int32_t *stamp = A.queue;
    if (threadIdx.x == 0) { s_done = 0; s_open = 0; }
    for (int t = threadIdx.x; t < DD_H * DD_H; t += 256) {
        const int li = t / DD_H, lj = t - li * DD_H;
        const int gi = V.i0 + li, gj = V.j0 + lj;
        bool fin = false;
        double d = 0.0;
        if (gi >= 0 && gi < A.n && gj >= 0 && gj < A.m) {
            const int32_t c = gi * A.m + gj;
            fin = stamp[c] < pass;
            if (fin) d = A.D[c];
            load(c);
        }
        store(t);
        Dl[t] = d; Fl[t] = fin ? (uint16_t)0 : DD_FL_OPEN;
    }
    __syncthreads();
}
__device__ __forceinline__ void dd_stage(const DistArgs &A, int32_t pass, const TileVisit &V, double *Dl, uint16_t *Fl, int32_t &s_done, int32_t &s_open)
{
    dd_stage(A, pass, V, Dl, Fl, s_done, s_open, [](int32_t) {}, [](int) {});
}

// this thread's k-th cell (k = 0..3): row (threadIdx.x / 32) + 8 k of the tile, column threadIdx.x % 32; idx: its LDS slot
struct CellSlot { int gi, gj, idx; };
__device__ __forceinline__ CellSlot dd_slot(int k, const TileVisit &V)
{
    const int ti = (int)(threadIdx.x >> 5) + 8 * k, tj = (int)(threadIdx.x & 31);
    return CellSlot{V.i0 + 1 + ti, V.j0 + 1 + tj, (ti + 1) * DD_H + tj + 1};
}
__device__ __forceinline__ int32_t dd_slot_cell(const DistArgs &A, const CellSlot &s) { return s.gi * A.m + s.gj; }
// the cell is on the grid and was open when the visit began: one of those the visit may finish
__device__ __forceinline__ bool dd_slot_open(const DistArgs &A, const CellSlot &s, const uint16_t *Fl) { return s.gi < A.n && s.gj < A.m && Fl[s.idx] != 0; }

// the k-th of a thread's four per-cell values, selected, not branched on: a wavefront runs an evaluation as often as its busiest
// lane has ready cells in the round -- usually once -- not once per cell slot
#define DD_SEL(a, k) ((k) == 0 ? a[0] : (k) == 1 ? a[1] : (k) == 2 ? a[2] : a[3])

// After the rounds: value(k, s) of the cells in `finished` (bit k: the thread's k-th cell, s its slot) goes to cell(k, s) of the
// result plane with the pass as stamp; then the tile's words.  n_open: how many of the thread's cells were open when the visit
// began.  (The cell is the kernel's to hand out: one that needs it in its rounds keeps it in a register, and working it out
// again from the slot cost k_du_tiles three VGPRs; one that does not recomputes it, dd_slot_cell.)
template <class Cell, class Value>
__device__ __forceinline__ void dd_visit_end(const DistArgs &A, int32_t pass, const TileVisit &V, int32_t &s_done, int32_t &s_open,
                                             int n_open, unsigned finished, Cell cell, Value value)
{
    int32_t *stamp = A.queue;
    int n_done = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (finished & (1u << k)) {
            const CellSlot s = dd_slot(k, V);
            const int32_t c = cell(k, s);
            A.D[c] = value(k, s); stamp[c] = pass; n_done++;
        }
    if (n_open) atomicAdd(&s_open, n_open - n_done);
    if (n_done) atomicAdd(&s_done, n_done);
    __syncthreads();
    if (threadIdx.x == 0) {
        V.tile_open[V.tile] = s_open;
        if (s_done) V.prog_w[V.tile] = pass;
        V.tile_done[V.tile] = s_done;
    }
}

// ---- the two kernels every sweep has
// The cell pattern of a call.  classify(A, c, i, j, cw, value) says whether the cell c = (i, j) with graph word cw starts open;
// if not, `value` is its final value.  An open cell gets the open pattern and DD_STAMP_OPEN, a final one its value and stamp 0.
template <class Classify>
__global__ __launch_bounds__(256) void k_flow_init(DistArgs A, Classify classify)
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
            double v = 0.0;
            open = classify(A, c, i, j, A.cinfo[c], v);
            if (open) reinterpret_cast<uint2 *>(A.D)[c] = make_uint2(0u, DD_OPEN_HI);
            else A.D[c] = v;
            A.queue[c] = open ? DD_STAMP_OPEN : 0;
        }
        mine += open ? 1 : 0;
    }
    // one global atomic per workgroup (a word takes ~90 atomics per microsecond: one per wavefront and row was most of this kernel)
    if (mine) atomicAdd(&s_open, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_open) atomicAdd(n_open, (unsigned long long)s_open);
}

// One level of the queue: the lane finishes its cell of the window [DD_LO, DD_HI) -- finish(A, v, cw) is its value, all it reads
// is from earlier launches -- then release(A, v, cw) takes one off the counts that waited for it and appends those that reach
// zero.  The release runs in control flow that is uniform per wavefront: a lane without a cell passes cw = 0.
template <class Finish, void (*Release)(const DistArgs &, int32_t, uint32_t)>
__global__ __launch_bounds__(256) void k_flow_level(DistArgs A, Finish finish)
{
    const int64_t lo = A.ctr[DD_LO], hi = A.ctr[DD_HI];
    for (int64_t base = lo + (int64_t)blockIdx.x * blockDim.x; base < hi; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = base + threadIdx.x;
        int32_t v = 0;
        uint32_t cw = 0;
        if (k < hi) {
            v = A.queue[k];
            cw = A.cinfo[v];
            A.D[v] = finish(A, v, cw);
        }
        Release(A, v, cw);
    }
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

// ---- the queue of a REVERSE sweep (flowdist.hip, flowacc_rev.hip): it depends on the graph alone, not on what is accumulated
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
        for (PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, v); b.more(); b.e++) {
            const int32_t u = A.pin_src[b.e];
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
                    for (PitBlock b = dd_pit_block(A.pit_src, A.n_pit, c); b.more(); b.e++)
                        if (dd_is_open(A, A.pit_dst[b.e])) cnt++;
                *dd_count(A, c) = cnt;
                ready = cnt == 0;
            }
        }
        dd_push(A, ready, c);
    }
}

// ---- the queue of a FORWARD sweep (flowdist_up.hip, flowacc_fwd.hip) and which cells it starts from: they depend on the graph
// and the elevation alone, not on what is accumulated
// every open cell counts its open in-neighbours (all values are from earlier launches); those with none start the queue
__global__ __launch_bounds__(256) void k_du_recount(DistArgs A)
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
                int cnt = 0;
#pragma unroll
                for (int d = 0; d < 8; d++)
                    if ((cw & (1u << d)) && dd_is_open(A, c + NB_DI[d] * A.m + NB_DJ[d])) cnt++;
                if (cw & CI_PIT_IN)
                    for (PitBlock b = dd_pit_block(A.pin_dst, A.n_pit, c); b.more(); b.e++)
                        if (dd_is_open(A, A.pin_src[b.e])) cnt++;
                *dd_count(A, c) = cnt;
                ready = cnt == 0;
            }
        }
        dd_push(A, ready, c);
    }
}

// cell v is final: every open cell one of its out-edges leads to has one open in-edge less.  `cw` = graph word of v, 0 for a
// lane that holds no cell.  (A cell that was final from the start -- NaN by the edge rule -- holds a value, not a count.)
__device__ __forceinline__ void du_release(const DistArgs &A, int32_t v, uint32_t cw)
{
    const int s = ci_section(cw);
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int32_t u = v + (q ? fe2r(s) * A.m + fe2c(s) : fe1r(s) * A.m + fe1c(s));
        bool ready = false;
        if ((cw & (q ? CI_OUT2 : CI_OUT1)) && dd_is_open(A, u)) ready = atomicSub(dd_count(A, u), 1) == 1;
        dd_push(A, ready, u);
    }
    if (cw & CI_PIT_OUT) {
        for (PitBlock b = dd_pit_block(A.pit_src, A.n_pit, v); b.more(); b.e++) {
            const int32_t u = A.pit_dst[b.e];
            if (dd_is_open(A, u) && atomicSub(dd_count(A, u), 1) == 1) {
                const int64_t slot = atomicAdd(A.ctr + DD_TAIL, 1);
                if (slot < A.qcap) A.queue[slot] = u;
            }
        }
    }
}

// NaN by the elevation and the edge rule; 0 where nothing flows in; the others are open
struct UpClassify {
    int edge_nan;
    __device__ __forceinline__ bool operator()(const DistArgs &A, int32_t c, int i, int j, uint32_t cw, double &value) const
    {
        const double z = A.elev[c];
        bool nanv = z != z;
        if (edge_nan && !nanv) {
            nanv = i == 0 || i == A.n - 1 || j == 0 || j == A.m - 1;
            if (!nanv) {
#pragma unroll
                for (int d = 0; d < 8; d++) { const double zn = A.elev[c + NB_DI[d] * A.m + NB_DJ[d]]; nanv = nanv || zn != zn; }
            }
        }
        value = nanv ? dd_nan() : 0.0;
        return !nanv && (cw & (0xFFu | CI_PIT_IN));
    }
};

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

// What every entry point checks of its tile (`what`: the function's name); 0, or the error code with the message set.  In two
// steps, because the checks of the call's own arguments come between them: there is a tile and its device is current; the tile
// has a flow graph.
static int dist_check_tile(pydem_tile *t, const char *what)
{
    if (!t) { pydem_set_error("%s: no tile", what); return -2; }
    HIP_TRY(hipSetDevice(t->device));
    return 0;
}
static int dist_check_graph(pydem_tile *t, const char *what)
{
    if (!t->graph_valid || !t->cinfo || !t->prop || !t->have[PYDEM_PROPORTION] || !t->have[PYDEM_ELEV] || !t->spacing_set) {
        pydem_set_error("%s: no flow graph on this tile (pydem_uca / pydem_build_graph first)", what);
        return -3;
    }
    return 0;
}

// a plane of the call's own (a mask, a seed) on the device: allocated on first use, freed with the tile
template <class T>
static int dist_upload(pydem_tile *t, T **plane, const T *src)
{
    PYDEM_TRY(tile_alloc(t, plane, (size_t)t->NN));
    return tile_plane_copy(t, *plane, const_cast<T *>(src), (size_t)t->NN * sizeof(T), false);
}

// the state the calls share (allocated by the first call of any, freed with the tile) and the argument block over it.  The
// int32 plane (stamps, then the queue) means nothing between the end of a sweep and the next init, which rewrites every stamp:
// streamnet.hip stages its int32 downloads in it there.  A sweep that wants to read a stamp of the call before has to give
// that use a plane of its own first.
static int dist_state(pydem_tile *t, DistArgs &A, int kind, int stat)
{
    const int64_t ntiles = cdiv(t->m, DD_T) * cdiv(t->n, DD_T);
    t->dd_down_ready = false;           // whoever takes the state writes the result plane: pydem_dist_down sets it again at its end
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

// The schedule of a call, the same for every sweep: the counters, the cell pattern (`init`), tile passes while they pay
// (`tiles`), the queue for the rest (`recount`, then one `level` launch per level), NaN for what never became ready, the
// timing and the download.  The four arguments launch the sweep's kernels on the tile's stream; default_per_visit: the
// cells a tile visit has to finish on average for another pass to beat the queue (the switch point of the sweep).
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

// dist_schedule with the launches every sweep makes the same way: the init and the level kernel from the sweep's Classify,
// Finish and release, its recount kernel over the rows; tiles(grid, pass, tiles_x, tiles_y, tile_state) launches its tile pass.
template <void (*Release)(const DistArgs &, int32_t, uint32_t), class Classify, class Finish, class FTiles>
static int dist_sweep(pydem_tile *t, const char *what, int64_t default_per_visit, const DistArgs &A, Classify classify, Finish finish,
                      void (*recount)(DistArgs), FTiles tiles, double *out, double *ms, int64_t *levels, int64_t *n_unresolved)
{
    const dim3 rows = dist_row_grid(t);
    return dist_schedule(t, what, default_per_visit, out, ms, levels, n_unresolved,
        [&] { hipLaunchKernelGGL(k_flow_init<Classify>, rows, dim3(256), 0, t->stream, A, classify); },
        [&](int pass, int tiles_x, int tiles_y, int32_t *tile_state) { tiles(dim3((unsigned)(tiles_x * tiles_y)), (int32_t)pass, tiles_x, tiles_y, tile_state); },
        [&] { hipLaunchKernelGGL(recount, rows, dim3(256), 0, t->stream, A); },
        [&](int grid) { hipLaunchKernelGGL((k_flow_level<Finish, Release>), dim3(grid), dim3(256), 0, t->stream, A, finish); });
}
