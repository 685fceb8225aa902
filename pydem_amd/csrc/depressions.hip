// depressions.hip -- pydem_depressions: the depression inventory of the resident elevation.  No reference method.
//
// W is the classic fill (eps = 0) of z, relaxed in scratch by the first part of pydem_fill_depressions (fill_relax); the
// elevation is only read.  A depression is an 8-connected component of the raised cells (W > z); with eps = 0 a component has
// one level, its spill elevation (include/pydem_hip.h has the definition of every column).  Everything here is integers: cell
// indices, counts, order-preserving bit patterns of doubles under atomicMin, fixed-point sums under atomicAdd -- so every
// schedule gives the same bits, and the host twin (pydem_amd/conditioning.py: label_depressions) is compared with array_equal.
//
// Labelling: a union-find over the int32 plane `parent` of linear cell indices (-1: not raised).
//   k_dp_init     parent[c] = c on raised cells; the largest depth of the tile (the volume's quantum needs it).
//   k_dp_local    one workgroup per 32 x 32 block: minimum-label propagation with pointer jumping in LDS to the block's fixed
//                 point; parent = the smallest linear index of the cell's component inside the block.  PYDEM_DEPR_LOCAL=0
//                 skips it: every raised cell stays its own root.
//   k_dp_merge    unites across the block seams (right, down, both diagonals; the four-block corners are diagonal steps like any
//                 other) -- or across EVERY adjacency when the local step was skipped.  A union links the larger root to the
//                 smaller with atomicMin and goes on from the value it displaced when the root it read was stale.  parent[x] <= x
//                 always and only ever falls, so every loop is a descent of strictly decreasing indices; nothing waits for
//                 another workgroup.  Reads of parent are agent-scope relaxed atomic loads: a plain load may be served from this
//                 CU's L1 or this XCD's L2 and miss what an atomicMin of another XCD did.  A stale value would still be an
//                 ancestor (old links stay valid), but the retry could then spin on it.
//   k_dp_flatten  parent = root; the root of a component is its smallest linear index whatever the order of the unions, since
//                 the cell with that index can never be linked below itself.  Flags the roots for the scan.
// Numbering: hipcub exclusive scan of the root flags in place: rank of a root = depressions with a smaller first cell.  K is the
// last word of the scan, and one more when the last cell is a root (label_components).  k_dp_ids then turns the parent plane into
// the plane of ids 1..K (0 not raised, -1 no data) and stores each depression's level from its root cell.
// Statistics: k_dp_stats, one lane per cell.  Raised cells (dp_raised): the lanes of a wavefront that share a row reduce across the
// wavefront (wave_by_key of stage_kit.h) and their first lane issues the atomics -- one set per wavefront inside a large lake
// instead of 64.  Other finite cells look at their eight neighbours for the sill columns and drop duplicate rows in registers
// (dp_sills).  k_dp_bottom finds the smallest index among the cells at a depression's lowest z; k_dp_botelev copies that cell's
// elevation.
// The table is K rows of DT_COLS 64-bit words, column-major, in the conditioning arena; the host filters it, uploads the
// id -> kept id lookup, and k_dp_write produces the label plane.
#include "stage_kit.h"
#include <hipcub/hipcub.hpp>
#include <memory>

namespace {

constexpr int DP_B = 32;            // block edge of the local step (the fill's block)
constexpr int DP_T = 256;           // lanes per workgroup: 32 columns x 8 groups of 4 rows
constexpr int DP_R = DP_B * DP_B / DP_T;

// counter block, 64-bit words
enum { DPC_DEPTH = 0,   // bits of max (W - z)
       DPC_WORDS = 8 };

// table columns (64-bit words, column c of row k at tab[c * T + k]).  The first DT_SEAM_COLS, in this order, are the partial table
// of pydem_fill_seam_inventory: its ABI, mirrored by conditioning.SEAM_TABLE_COLS.  The table of pydem_depressions has the level
// too; the host reads it column by column (col() of stage_depressions), so the order is nobody's business there.
enum { DT_CELLS = 0, DT_R0, DT_R1, DT_C0, DT_C1,
       DT_ZMIN,         // order-preserving pattern of the lowest z (+0.0 for -0.0: they compare equal)
       DT_BOTTOM, DT_POUR, DT_NSILLS, DT_OPEN,
       DT_AREA, DT_VOLUME,      // fixed-point sums (int64 in two's complement; every term is >= 0)
       DT_BOTELEV,              // bits of a double, a plain store
       DT_SEAM_COLS,
       DT_SPILL = DT_SEAM_COLS, // the same
       DT_COLS };

__device__ inline int dp_ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int dp_find(const int32_t *parent, int x)
{
    for (;;) {
        const int p = dp_ld(parent + x);        // p <= x
        if (p == x) return x;
        x = p;
    }
}

// a > b after the swap; parent[a] = min(parent[a], b).  old == a: a was a root and now hangs under b.  Otherwise a had been linked
// below itself in the meantime: its former parent `old` (< a) and b still have to meet.
__device__ inline void dp_unite(int32_t *parent, int a, int b)
{
    for (;;) {
        a = dp_find(parent, a);
        b = dp_find(parent, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// doubles as unsigned words of the same order
__device__ inline u64 dp_key(double v)
{
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double dp_unkey(u64 k)
{
    const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

__global__ void __launch_bounds__(256)
k_dp_init(const double *__restrict__ z, const double *__restrict__ W, int32_t *__restrict__ parent, int64_t NN, u64 *ctr)
{
    double dmax = 0.0;
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = c0 + threadIdx.x;
        if (c >= NN) continue;
        const double w = W[c], v = z[c];
        const bool up = w > v;
        parent[c] = up ? (int32_t)c : -1;
        if (up && w - v > dmax) dmax = w - v;
    }
    dmax = wave_max(dmax);
    if ((threadIdx.x & 63) == 0 && dmax > 0.0) atomicMax(ctr + DPC_DEPTH, (u64)__double_as_longlong(dmax));
}

__global__ void __launch_bounds__(DP_T)
k_dp_local(int32_t *__restrict__ parent, int n, int m)
{
    __shared__ int s[DP_B * DP_B];      // local index of the smallest cell known in the component, -1: not raised
    const int tid = (int)threadIdx.x, tx = tid & (DP_B - 1), ty = tid >> 5;
    const int r0 = (int)blockIdx.y * DP_B, c0 = (int)blockIdx.x * DP_B;
    const int gc = c0 + tx;
    int any = 0;
#pragma unroll
    for (int k = 0; k < DP_R; k++) {
        const int lr = ty * DP_R + k, gr = r0 + lr;
        int v = -1;
        if (gr < n && gc < m && parent[(int64_t)gr * m + gc] >= 0) { v = lr * DP_B + tx; any = 1; }
        s[lr * DP_B + tx] = v;
    }
    if (!__syncthreads_or(any)) return;
    for (;;) {
        int nl[DP_R];
        bool changed = false;
#pragma unroll
        for (int k = 0; k < DP_R; k++) {
            const int lr = ty * DP_R + k;
            const int l = s[lr * DP_B + tx];
            int mn = l;
            if (l >= 0) {
#pragma unroll
                for (int dr = -1; dr <= 1; dr++)
#pragma unroll
                    for (int dq = -1; dq <= 1; dq++) {
                        const int rr = lr + dr, qq = tx + dq;
                        if ((dr | dq) == 0 || rr < 0 || rr >= DP_B || qq < 0 || qq >= DP_B) continue;
                        const int v = s[rr * DP_B + qq];
                        if (v >= 0 && v < mn) mn = v;
                    }
                // pointer jumping: the label of a label is a cell of the same component with an index no larger
                mn = min(mn, s[mn]);
                mn = min(mn, s[mn]);
                changed |= mn < l;
            }
            nl[k] = mn;
        }
        __syncthreads();                            // every lane has read
        if (changed) {
#pragma unroll
            for (int k = 0; k < DP_R; k++) s[(ty * DP_R + k) * DP_B + tx] = nl[k];
        }
        if (!__syncthreads_or(changed ? 1 : 0)) break;
    }
#pragma unroll
    for (int k = 0; k < DP_R; k++) {
        const int lr = ty * DP_R + k, gr = r0 + lr;
        const int l = s[lr * DP_B + tx];
        if (l >= 0) parent[(int64_t)gr * m + gc] = (int32_t)((int64_t)(r0 + (l >> 5)) * m + c0 + (l & (DP_B - 1)));   // (l >= 0: a cell of the tile)
    }
}

// the four forward neighbours of a cell: every adjacency once
__global__ void __launch_bounds__(256)
k_dp_merge(int32_t *parent, int n, int m, int all)
{
    const int64_t NN = (int64_t)n * m;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(c / m), q = (int)(c - (int64_t)r * m);
        const int lr = r & (DP_B - 1), lq = q & (DP_B - 1);
        if (!all && lr != DP_B - 1 && lq != DP_B - 1 && lq != 0) continue;       // no forward neighbour in another block
        if (dp_ld(parent + c) < 0) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int dr = k == 0 ? 0 : 1, dq = k == 0 ? 1 : k - 2;               // (0,+1) (1,-1) (1,0) (1,+1)
            const int rr = r + dr, qq = q + dq;
            if (rr >= n || qq < 0 || qq >= m) continue;
            if (!all && (rr >> 5) == (r >> 5) && (qq >> 5) == (q >> 5)) continue;
            const int64_t v = (int64_t)rr * m + qq;
            if (dp_ld(parent + v) < 0) continue;
            dp_unite(parent, (int)c, (int)v);
        }
    }
}

__global__ void __launch_bounds__(256)
k_dp_flatten(int32_t *parent, int32_t *__restrict__ rank, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        int flag = 0;
        if (dp_ld(parent + c) >= 0) {
            const int root = dp_find(parent, (int)c);       // (a store of this launch that the walk meets is a root already)
            parent[c] = root;
            flag = root == (int)c;
        }
        rank[c] = flag;
    }
}

// the first `cols` columns of a table of T rows
__global__ void __launch_bounds__(256)
k_dp_table_init(u64 *tab, int64_t T, int cols)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * cols) return;
    const int col = (int)(i / T);
    const bool is_min = col == DT_R0 || col == DT_C0 || col == DT_ZMIN || col == DT_BOTTOM || col == DT_POUR;
    tab[i] = is_min ? ~0ull : 0ull;
}

// parent (flattened) -> ids in place: a lane reads and writes its own word of the plane only; rank is read-only here
__global__ void __launch_bounds__(256)
k_dp_ids(int32_t *lab, const int32_t *__restrict__ rank, const double *__restrict__ W, u64 *tab, int64_t K, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int p = lab[c];
        const double w = W[c];
        int id;
        if (p >= 0) {
            id = rank[p] + 1;
            if (p == (int)c && id <= K) tab[(int64_t)DT_SPILL * K + id - 1] = (u64)__double_as_longlong(w);
        } else
            id = isnan(w) ? -1 : 0;
        lab[c] = id;
    }
}

// The statistics of a raised cell (up) of row `row` (1 .. T) at (r, q): elevation zc, surface wc, cell area a0.  The lanes of the
// wavefront that share the row publish one set of atomics into eight columns.  Reached by the whole wavefront.
__device__ __forceinline__ void dp_raised(bool up, int row, int r, int q, double zc, double wc, double a0, int sh_area, int sh_vol,
                                          u64 *tab, int64_t T)
{
    const int lane = (int)(threadIdx.x & 63);
    u64 zk = ~0ull, ai = 0, vi = 0;
    if (up) {
        zk = dp_key(zc + 0.0);
        ai = (u64)__double2ll_rn(ldexp(a0, sh_area));
        vi = (u64)__double2ll_rn(ldexp((wc - zc) * a0, sh_vol));
    }
    wave_by_key(up, row, [&](int lrow, int leader, u64 mask, bool mine, bool lone) {
        int rmin = r, rmax = r, qmin = q, qmax = q;
        u64 cnt = 1, k = zk, a = ai, v = vi;
        if (!lone) {                                        // more than one lane: reduce first (uniform branch)
            rmin = wave_min(mine ? r : 0x7fffffff);
            rmax = wave_max(mine ? r : -1);
            qmin = wave_min(mine ? q : 0x7fffffff);
            qmax = wave_max(mine ? q : -1);
            k = wave_min(mine ? zk : ~0ull);
            a = wave_add(mine ? ai : 0ull);
            v = wave_add(mine ? vi : 0ull);
            cnt = (u64)__popcll(mask);
        }
        if (lane == leader) {
            u64 *w = tab + (lrow - 1);
            atomicAdd(w + (int64_t)DT_CELLS * T, cnt);
            atomicMin(w + (int64_t)DT_R0 * T, (u64)rmin);
            atomicMax(w + (int64_t)DT_R1 * T, (u64)rmax);
            atomicMin(w + (int64_t)DT_C0 * T, (u64)qmin);
            atomicMax(w + (int64_t)DT_C1 * T, (u64)qmax);
            atomicMin(w + (int64_t)DT_ZMIN * T, k);
            atomicAdd(w + (int64_t)DT_AREA * T, a);
            atomicAdd(w + (int64_t)DT_VOLUME * T, v);
        }
    });
}

// neighbour j = 0 .. 7 of a cell, row by row
__device__ __forceinline__ void dp_neighbour(int j, int r, int q, int &rr, int &qq)
{
    rr = r + (j < 3 ? -1 : (j < 5 ? 0 : 1));
    qq = q + (j < 3 ? j - 1 : (j == 3 ? -1 : (j == 4 ? 1 : j - 6)));
}

// A sill cell c -- finite, not raised, beside a depression whose level is its elevation: rows[j] is the row of neighbour j where
// that neighbour is such a depression's cell, else 0.  Every distinct row gets the cell once (duplicates dropped in registers).
__device__ __forceinline__ void dp_sills(const int (&rows)[8], bool open, const uint8_t *__restrict__ outlets, int64_t c, u64 *tab, int64_t T)
{
    int found = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) found |= rows[j];
    if (!found) return;
    if (outlets && outlets[c] != 0) open = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        bool fresh = rows[j] > 0;
#pragma unroll
        for (int i = 0; i < j; i++) fresh = fresh && rows[i] != rows[j];
        if (fresh) {
            u64 *w = tab + (rows[j] - 1);
            atomicAdd(w + (int64_t)DT_NSILLS * T, 1ull);
            atomicMin(w + (int64_t)DT_POUR * T, (u64)c);
            if (open) atomicMax(w + (int64_t)DT_OPEN * T, 1ull);
        }
    }
}

// rows are the ids of the plane; a neighbour outside the tile is nothing (its cell is on the border: open)
__global__ void __launch_bounds__(256)
k_dp_stats(const int32_t *__restrict__ lab, const double *__restrict__ z, const double *__restrict__ W, const uint8_t *__restrict__ outlets,
           const double *__restrict__ dX2, const double *__restrict__ dY2, u64 *tab, int64_t K, int n, int m, int sh_area, int sh_vol)
{
    const int64_t NN = (int64_t)n * m;
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {     // (uniform per wavefront)
        const int64_t c = c0 + threadIdx.x;
        int id = 0, r = 0, q = 0;
        double zc = 0.0;
        if (c < NN) {
            id = lab[c];
            r = (int)(c / m);
            q = (int)(c - (int64_t)r * m);
            zc = z[c];
        }
        const bool up = id > 0 && id <= K;
        dp_raised(up, id, r, q, zc, up ? W[c] : 0.0, up ? dX2[r] * dY2[r] : 0.0, sh_area, sh_vol, tab, K);      // (row_area, as k_row_area)
        if (c < NN && id == 0) {
            int rows[8];
            bool open = r == 0 || r == n - 1 || q == 0 || q == m - 1;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                int rr, qq;
                dp_neighbour(j, r, q, rr, qq);
                rows[j] = 0;
                if (rr < 0 || rr >= n || qq < 0 || qq >= m) continue;
                const int64_t v = (int64_t)rr * m + qq;
                const int l = lab[v];
                if (l < 0) open = true;                         // beside no data
                else if (l > 0 && l <= K && W[v] == zc) rows[j] = l;
            }
            dp_sills(rows, open, outlets, c, tab, K);
        }
    }
}

__global__ void __launch_bounds__(256)
k_dp_bottom(const int32_t *__restrict__ lab, const double *__restrict__ z, u64 *tab, int64_t K, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int id = lab[c];
        if (id <= 0 || id > K) continue;
        if (z[c] == dp_unkey(tab[(int64_t)DT_ZMIN * K + id - 1])) atomicMin(tab + (int64_t)DT_BOTTOM * K + id - 1, (u64)c);
    }
}

__global__ void __launch_bounds__(256)
k_dp_botelev(const double *__restrict__ z, u64 *tab, int64_t T, int64_t NN)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= T) return;
    const u64 b = tab[(int64_t)DT_BOTTOM * T + k];
    if (b < (u64)NN) tab[(int64_t)DT_BOTELEV * T + k] = (u64)__double_as_longlong(z[b]);
}

__global__ void __launch_bounds__(256)
k_dp_write(const int32_t *__restrict__ lab, const int32_t *__restrict__ lut, int32_t *__restrict__ out, int64_t K, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int id = lab[c];
        out[c] = (id > 0 && id <= K) ? lut[id] : (id < 0 ? -1 : 0);
    }
}

// The labelling of the raised cells (W > z): parent <- each cell's root, the smallest linear index of its component (-1: not
// raised); out->rank <- the exclusive scan of the root flags; K components; depth_max the largest W - z.  rank, the counter block
// and the scan's scratch come from the lease.  ev_start is recorded where the device work begins; marks (may be null): marks[0],
// [1], [2] after init + local, merge, flatten.  Waits for the stream.
struct Labelling { int32_t *rank = nullptr; int64_t K = 0; double depth_max = 0.0; };
int label_components(pydem_tile *t, ArenaLease *lease, const char *who, const double *W, int32_t *parent, hipEvent_t ev_start,
                     hipEvent_t *marks, Labelling *out)
{
    const bool local = env_switch("PYDEM_DEPR_LOCAL", true);    // read per call: the tests switch it
    const int n = (int)t->n, m = (int)t->m;
    const int64_t NN = t->NN;
    int32_t *rank = (int32_t *)arena_take(lease, (size_t)NN * 4);
    u64 *ctr = (u64 *)arena_take(lease, DPC_WORDS * 8);
    size_t scan_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (int32_t *)nullptr, (int32_t *)nullptr, (int)NN, t->stream));
    void *scan_tmp = arena_take(lease, scan_bytes);
    if (!rank || !ctr || !scan_tmp) return -1;
    const int gfull = capped_grid(NN, GRID_FULL);
    HIP_TRY(hipEventRecord(ev_start, t->stream));
    HIP_TRY(hipMemsetAsync(ctr, 0, DPC_WORDS * 8, t->stream));
    hipLaunchKernelGGL(k_dp_init, dim3(capped_grid(NN, GRID_LOOP)), dim3(256), 0, t->stream, (const double *)t->elev, W, parent, NN, ctr);
    if (local) hipLaunchKernelGGL(k_dp_local, dim3((unsigned)cdiv(m, DP_B), (unsigned)cdiv(n, DP_B)), dim3(DP_T), 0, t->stream, parent, n, m);
    HIP_TRY(hipGetLastError());
    if (marks) HIP_TRY(hipEventRecord(marks[0], t->stream));
    hipLaunchKernelGGL(k_dp_merge, dim3(gfull), dim3(256), 0, t->stream, parent, n, m, local ? 0 : 1);
    HIP_TRY(hipGetLastError());
    if (marks) HIP_TRY(hipEventRecord(marks[1], t->stream));
    hipLaunchKernelGGL(k_dp_flatten, dim3(gfull), dim3(256), 0, t->stream, parent, rank, NN);
    HIP_TRY(hipGetLastError());
    if (marks) HIP_TRY(hipEventRecord(marks[2], t->stream));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, rank, rank, (int)NN, t->stream));
    // K and the largest depth.  The exclusive sum at the last cell leaves that cell out: it counts when it is its own root.  A seam
    // cell of a session may be raised, the tile's last cell included; in pydem_depressions the last cell is an open border cell
    // and never a root, so the rule gives the plain last word of the scan there.
    volatile u64 *h = (volatile u64 *)t->h_counters;
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr, 8, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync(t->h_counters + 2, rank + (NN - 1), 4, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync(t->h_counters + 3, parent + (NN - 1), 4, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    const int64_t K = (int64_t)t->h_counters[2] + ((int64_t)t->h_counters[3] == NN - 1 ? 1 : 0);
    if (K < 0 || K > NN) { pydem_set_error("%s: inconsistent count of depressions (%lld)", who, (long long)K); return -5; }
    out->rank = rank;
    out->K = K;
    out->depth_max = as_double(h[DPC_DEPTH]);
    return 0;
}

}  // namespace

int stage_depressions(pydem_tile *t, const uint8_t *outlets, double min_depth, int64_t min_cells, double min_volume, int32_t *label,
                      int64_t *n_found, int64_t *n_kept, double *quanta, int64_t *passes, double *ms)
{
    if (!(min_depth >= 0) || !(min_volume >= 0) || min_cells < 0) {
        pydem_set_error("pydem_depressions: min_depth, min_cells and min_volume must be >= 0 (got %g, %lld, %g)", min_depth, (long long)min_cells, min_volume);
        return -2;
    }
    if (!t->spacing_set) { pydem_set_error("pydem_depressions: call pydem_tile_set_spacing first"); return -3; }
    if (t->NN >= (int64_t)INT32_MAX) { pydem_set_error("pydem_depressions: %lld cells do not fit the int32 parent plane", (long long)t->NN); return -2; }
    const int n = (int)t->n, m = (int)t->m;
    const int64_t NN = t->NN;

    Events<9> ev;
    PYDEM_TRY(ev.create());
    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    FillRelax fr;
    double eps = 0.0;
    PYDEM_TRY(fill_relax(t, &lease, "pydem_depressions", &eps, outlets, ev.e[0], &fr));
    const double *W = fr.W;
    const double *z = t->elev;
    int32_t *parent = (int32_t *)arena_take(&lease, (size_t)NN * 4);
    if (!parent) return -1;
    Labelling lb;
    PYDEM_TRY(label_components(t, &lease, "pydem_depressions", W, parent, ev.e[1], &ev.e[2], &lb));    // (ev.e[1]: relaxation done)
    int32_t *rank = lb.rank;
    const int64_t K = lb.K;
    const double depth_max = lb.depth_max;
    const int gcells = capped_grid(NN, GRID_LOOP), gfull = capped_grid(NN, GRID_FULL);

    double amax = 0.0;
    for (int64_t r = 0; r < t->n; r++) { const double a = t->h_dX2[(size_t)r] * t->h_dY2[(size_t)r]; if (a > amax) amax = a; }
    int sh_area = 0, sh_vol = 0;
    double q_area = 0, q_vol = 0;
    fixed_point(NN, amax, &sh_area, &q_area);
    fixed_point(NN, depth_max * amax, &sh_vol, &q_vol);

    u64 *tab = nullptr;
    int32_t *lut = nullptr;
    if (K > 0) {
        tab = (u64 *)arena_take(&lease, (size_t)K * DT_COLS * 8);
        lut = (int32_t *)arena_take(&lease, (size_t)(K + 1) * 4);
        if (!tab || !lut) {
            pydem_set_error("pydem_depressions: no device memory for the table of %lld depressions (%lld bytes); nothing was returned",
                            (long long)K, (long long)(K * (DT_COLS * 8 + 4)));
            return -6;
        }
        hipLaunchKernelGGL(k_dp_table_init, dim3((unsigned)cdiv(K * DT_COLS, 256)), dim3(256), 0, t->stream, tab, K, (int)DT_COLS);
    }
    hipLaunchKernelGGL(k_dp_ids, dim3(gfull), dim3(256), 0, t->stream, parent, (const int32_t *)rank, W, tab, K, NN);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[5], t->stream));                // numbering done
    const int32_t *lab = parent;
    std::unique_ptr<u64[]> htab;             // (not a vector: no zero fill of 112 bytes per depression before the copy)
    if (K > 0) {
        hipLaunchKernelGGL(k_dp_stats, dim3(gcells), dim3(256), 0, t->stream, lab, z, W, (const uint8_t *)fr.outlets, (const double *)t->dX2,
                           (const double *)t->dY2, tab, K, n, m, sh_area, sh_vol);
        hipLaunchKernelGGL(k_dp_bottom, dim3(gfull), dim3(256), 0, t->stream, lab, z, tab, K, NN);
        hipLaunchKernelGGL(k_dp_botelev, dim3((unsigned)cdiv(K, 256)), dim3(256), 0, t->stream, z, tab, K, NN);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev.e[6], t->stream));                // statistics done
    if (K > 0) {
        htab.reset(new u64[(size_t)K * DT_COLS]);
        PYDEM_TRY(tile_plane_copy(t, tab, htab.get(), (size_t)K * DT_COLS * 8, true));
    }

    // the host's part: rows, filters, renumbering
    std::vector<pydem_depression> rows;
    std::vector<int32_t> hlut((size_t)K + 1, 0);
    rows.reserve((size_t)K);
    for (int64_t k = 0; k < K; k++) {
        auto col = [&](int c) { return htab[(size_t)c * (size_t)K + (size_t)k]; };
        pydem_depression d;
        d.cells = (int64_t)col(DT_CELLS);
        d.r0 = (int64_t)col(DT_R0); d.r1 = (int64_t)col(DT_R1); d.c0 = (int64_t)col(DT_C0); d.c1 = (int64_t)col(DT_C1);
        d.bottom = (int64_t)col(DT_BOTTOM);
        d.pour = (int64_t)col(DT_POUR);
        d.n_sills = (int64_t)col(DT_NSILLS);
        d.open_sill = (int64_t)col(DT_OPEN);
        d.spill_elev = as_double(col(DT_SPILL));
        d.bottom_elev = as_double(col(DT_BOTELEV));
        d.max_depth = d.spill_elev - d.bottom_elev;
        d.area = (double)(int64_t)col(DT_AREA) * q_area;
        d.volume = (double)(int64_t)col(DT_VOLUME) * q_vol;
        if (d.cells < 1 || d.bottom >= NN || d.pour >= NN || d.n_sills < 1) {
            pydem_set_error("pydem_depressions: depression %lld has %lld cells, %lld sills, bottom %lld, pour %lld", (long long)k + 1,
                            (long long)d.cells, (long long)d.n_sills, (long long)d.bottom, (long long)d.pour);
            return -5;
        }
        if (d.max_depth < min_depth || d.cells < min_cells || d.volume < min_volume) continue;
        rows.push_back(d);
        hlut[(size_t)k + 1] = (int32_t)rows.size();
    }
    if (label) {
        if (K > 0) PYDEM_TRY(tile_plane_copy(t, lut, hlut.data(), hlut.size() * 4, false));
        HIP_TRY(hipEventRecord(ev.e[8], t->stream));            // table on the host, filtered; lookup on the device
        hipLaunchKernelGGL(k_dp_write, dim3(gfull), dim3(256), 0, t->stream, lab, (const int32_t *)lut, rank, K, NN);
        HIP_TRY(hipGetLastError());
    } else
        HIP_TRY(hipEventRecord(ev.e[8], t->stream));
    HIP_TRY(hipEventRecord(ev.e[7], t->stream));                // label plane written
    HIP_TRY(hipEventSynchronize(ev.e[7]));
    if (label) PYDEM_TRY(tile_plane_copy(t, rank, label, (size_t)NN * 4, true));
    if (ms) {
        // whole call, relaxation, init + local, merge, flatten, numbering, statistics, table (download, host filter, lookup upload), label write
        static const int from[9] = {0, 0, 1, 2, 3, 4, 5, 6, 8}, to[9] = {7, 1, 2, 3, 4, 5, 6, 8, 7};
        for (int i = 0; i < 9; i++) PYDEM_TRY(ev.elapsed(from[i], to[i], &ms[i]));
    }
    if (n_found) *n_found = K;
    if (n_kept) *n_kept = (int64_t)rows.size();
    if (quanta) { quanta[0] = q_area; quanta[1] = q_vol; }
    if (passes) *passes = fr.passes;
    t->depr.swap(rows);
    return 0;
}

// ---- the inventory ACROSS tiles: the session calls pydem_fill_seam_label / _label_roots / _get_id_lines / _inventory / _labels
// (include/pydem_hip.h).  The session's W is the tile's window of the whole-mosaic classic fill; the tile labels its own
// components of W > z with the kernels above, the host joins them across the tiles, and the tile then reduces the cells it OWNS
// into a partial table whose rows are the mosaic's depressions it can meet.  A cell outside the window comes from the halo ring
// (2 m + 2 n + 4 cells: the row above over columns -1 .. m, the row below, the column left over rows 0 .. n-1, the column right).
// Integers only, as above: the host twin (conditioning.SeamFill) gives the same words.
namespace {

// parent (flattened) -> local ids in place, as k_dp_ids; a root stores its cell and its level
__global__ void __launch_bounds__(256)
k_ds_ids(int32_t *lab, const int32_t *__restrict__ rank, const double *__restrict__ W, int32_t *__restrict__ roots,
         double *__restrict__ levels, int64_t K, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int p = lab[c];
        const double w = W[c];
        int id;
        if (p >= 0) {
            id = rank[p] + 1;
            if (p == (int)c && id <= K) { roots[id - 1] = (int32_t)c; levels[id - 1] = w; }
        } else
            id = isnan(w) ? -1 : 0;
        lab[c] = id;
    }
}

// k_dp_stats on the cells the tile owns: rows through the lookup (several local ids may share a row), and a neighbour outside the
// window from the halo ring.  A sill's whole 3 x 3 is known here, so it is open exactly when a neighbour is no data or uncovered
// (-1), or when it is an outlet
__global__ void __launch_bounds__(256)
k_ds_stats(const int32_t *__restrict__ ids, const double *__restrict__ z, const double *__restrict__ W, const uint8_t *__restrict__ outlets,
           const uint8_t *__restrict__ owner, const int32_t *__restrict__ lut, const int32_t *__restrict__ halo_ids,
           const double *__restrict__ halo_W, const double *__restrict__ row_area, u64 *tab, int64_t T, int n, int m, int sh_area, int sh_vol)
{
    const int64_t NN = (int64_t)n * m;
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {     // (uniform per wavefront)
        const int64_t c = c0 + threadIdx.x;
        int l = -1, g = 0, r = 0, q = 0;
        bool own = false;
        double zc = 0.0;
        if (c < NN) {
            l = ids[c];
            own = owner[c] != 0;
            r = (int)(c / m);
            q = (int)(c - (int64_t)r * m);
            zc = z[c];
            if (l > 0) g = lut[l];
        }
        const bool up = own && g > 0;
        dp_raised(up, g, r, q, zc, up ? W[c] : 0.0, up ? row_area[r] : 0.0, sh_area, sh_vol, tab, T);
        if (c < NN && own && l == 0) {
            int rows[8];
            bool open = false;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                int rr, qq;
                dp_neighbour(j, r, q, rr, qq);
                rows[j] = 0;
                int gv;
                double wv = 0.0;
                if (rr >= 0 && rr < n && qq >= 0 && qq < m) {
                    const int64_t v = (int64_t)rr * m + qq;
                    const int lv = ids[v];
                    gv = lv < 0 ? -1 : (lv > 0 ? lut[lv] : 0);
                    if (gv > 0) wv = W[v];
                } else {
                    int h;
                    if (rr < 0) h = qq + 1;
                    else if (rr >= n) h = (m + 2) + qq + 1;
                    else if (qq < 0) h = 2 * (m + 2) + rr;
                    else h = 2 * (m + 2) + n + rr;
                    gv = halo_ids[h];
                    wv = halo_W[h];
                }
                if (gv < 0) open = true;
                else if (gv > 0 && wv == zc) rows[j] = gv;
            }
            dp_sills(rows, open, outlets, c, tab, T);
        }
    }
}

__global__ void __launch_bounds__(256)
k_ds_bottom(const int32_t *__restrict__ ids, const double *__restrict__ z, const uint8_t *__restrict__ owner, const int32_t *__restrict__ lut,
            u64 *tab, int64_t T, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int l = ids[c];
        if (l <= 0 || owner[c] == 0) continue;
        const int g = lut[l];
        if (g <= 0) continue;
        if (z[c] == dp_unkey(tab[(int64_t)DT_ZMIN * T + g - 1])) atomicMin(tab + (int64_t)DT_BOTTOM * T + g - 1, (u64)c);
    }
}

__global__ void __launch_bounds__(256)
k_ds_write(const int32_t *__restrict__ ids, const int32_t *__restrict__ lut, int32_t *__restrict__ out, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int l = ids[c];
        out[c] = l > 0 ? lut[l] : l;
    }
}

}  // namespace

int stage_fill_seam_label(pydem_tile *t, int64_t *n_local, double *max_depth, double *ms)
{
    const char *who = "pydem_fill_seam_label";
    if (!t->fs_open) { pydem_set_error("%s: no session is open on this tile (pydem_fill_seam_begin first)", who); return -2; }
    if (t->NN >= (int64_t)INT32_MAX) { pydem_set_error("%s: %lld cells do not fit the int32 id plane", who, (long long)t->NN); return -2; }
    const int64_t NN = t->NN;
    if (!t->fs_ids) PYDEM_TRY(tile_hold(t, (void **)&t->fs_ids, (size_t)NN * 4, true));
    t->fs_K = -1;
    t->fs_roots.clear();
    t->fs_levels.clear();

    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    int32_t *parent = t->fs_ids;
    const double *W = t->fs_W;
    Labelling lb;
    PYDEM_TRY(label_components(t, &lease, who, W, parent, t->ev[6], nullptr, &lb));
    const int32_t *rank = lb.rank;
    const int64_t K = lb.K;
    const double depth_max = lb.depth_max;
    if (!std::isfinite(depth_max)) {
        pydem_set_error("%s: cells of W are still +inf (no relaxation has reached them); nothing was labelled", who);
        return -5;
    }
    int32_t *roots = nullptr;
    double *levels = nullptr;
    if (K > 0) {
        roots = (int32_t *)arena_take(&lease, (size_t)K * 4);
        levels = (double *)arena_take(&lease, (size_t)K * 8);
        if (!roots || !levels) return -1;
    }
    hipLaunchKernelGGL(k_ds_ids, dim3(capped_grid(NN, GRID_FULL)), dim3(256), 0, t->stream, parent, (const int32_t *)rank, W, roots, levels, K, NN);
    HIP_TRY(hipGetLastError());
    PYDEM_TRY(stage_elapsed(t, ms));
    if (K > 0) {
        t->fs_roots.resize((size_t)K);
        t->fs_levels.resize((size_t)K);
        PYDEM_TRY(tile_plane_copy(t, roots, t->fs_roots.data(), (size_t)K * 4, true));
        PYDEM_TRY(tile_plane_copy(t, levels, t->fs_levels.data(), (size_t)K * 8, true));
    }
    t->fs_K = K;
    if (n_local) *n_local = K;
    if (max_depth) *max_depth = depth_max;
    return 0;
}

int stage_fill_seam_label_roots(pydem_tile *t, int64_t count, int32_t *roots, double *levels)
{
    const char *who = "pydem_fill_seam_label_roots";
    if (!t->fs_open || t->fs_K < 0) { pydem_set_error("%s: the open session has no labels (pydem_fill_seam_label first)", who); return -2; }
    if (count != t->fs_K || (count > 0 && (!roots || !levels))) {
        pydem_set_error("%s: %lld entries asked, pydem_fill_seam_label found %lld", who, (long long)count, (long long)t->fs_K);
        return -2;
    }
    if (count > 0) {
        memcpy(roots, t->fs_roots.data(), (size_t)count * 4);
        memcpy(levels, t->fs_levels.data(), (size_t)count * 8);
    }
    return 0;
}

int stage_fill_seam_get_id_lines(pydem_tile *t, int count, const int *axes, const int64_t *indices, void *const *dsts)
{
    const char *who = "pydem_fill_seam_get_id_lines";
    if (!t->fs_open || t->fs_K < 0) { pydem_set_error("%s: the open session has no labels (pydem_fill_seam_label first)", who); return -2; }
    return seam_get_lines(t, who, (const int32_t *)t->fs_ids, count, axes, indices, dsts);
}

int stage_fill_seam_inventory(pydem_tile *t, const int32_t *lut, int64_t T, const uint8_t *owner, const uint8_t *outlets,
                              const int32_t *halo_ids, const double *halo_W, const double *row_area, int sh_area, int sh_vol,
                              uint64_t *table, double *ms)
{
    const char *who = "pydem_fill_seam_inventory";
    if (!t->fs_open || t->fs_K < 0) { pydem_set_error("%s: the open session has no labels (pydem_fill_seam_label first)", who); return -2; }
    const int n = (int)t->n, m = (int)t->m;
    const int64_t NN = t->NN, K = t->fs_K;
    const size_t R = 2 * (size_t)m + 2 * (size_t)n + 4;
    if (!lut || !owner || !halo_ids || !halo_W || !row_area || (T > 0 && !table)) { pydem_set_error("%s: a NULL argument", who); return -2; }
    if (T < 0 || T >= (int64_t)INT32_MAX) { pydem_set_error("%s: %lld rows do not fit int32 ids", who, (long long)T); return -2; }
    // every index the kernels form from these is checked here: a row is 1 .. T
    for (int64_t k = 0; k <= K; k++)
        if (lut[k] < 0 || lut[k] > T) { pydem_set_error("%s: lookup entry %lld is %d, outside 0 .. %lld", who, (long long)k, lut[k], (long long)T); return -2; }
    for (size_t e = 0; e < R; e++)
        if (halo_ids[e] < -1 || halo_ids[e] > T) { pydem_set_error("%s: halo entry %zu is %d, outside -1 .. %lld", who, e, halo_ids[e], (long long)T); return -2; }
    if (ms) *ms = 0.0;
    if (T == 0) return 0;

    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    int32_t *d_lut = (int32_t *)arena_take(&lease, (size_t)(K + 1) * 4);
    uint8_t *d_owner = (uint8_t *)arena_take(&lease, (size_t)NN);
    uint8_t *d_out = outlets ? (uint8_t *)arena_take(&lease, (size_t)NN) : nullptr;
    int32_t *d_hid = (int32_t *)arena_take(&lease, R * 4);
    double *d_hW = (double *)arena_take(&lease, R * 8);
    double *d_ra = (double *)arena_take(&lease, (size_t)n * 8);
    u64 *tab = (u64 *)arena_take(&lease, (size_t)T * DT_SEAM_COLS * 8);
    if (!d_lut || !d_owner || (outlets && !d_out) || !d_hid || !d_hW || !d_ra || !tab) return -1;
    PYDEM_TRY(tile_plane_copy(t, d_lut, const_cast<int32_t *>(lut), (size_t)(K + 1) * 4, false));
    PYDEM_TRY(tile_plane_copy(t, d_owner, const_cast<uint8_t *>(owner), (size_t)NN, false));
    if (outlets) PYDEM_TRY(tile_plane_copy(t, d_out, const_cast<uint8_t *>(outlets), (size_t)NN, false));
    PYDEM_TRY(tile_plane_copy(t, d_hid, const_cast<int32_t *>(halo_ids), R * 4, false));
    PYDEM_TRY(tile_plane_copy(t, d_hW, const_cast<double *>(halo_W), R * 8, false));
    PYDEM_TRY(tile_plane_copy(t, d_ra, const_cast<double *>(row_area), (size_t)n * 8, false));

    const int gcells = capped_grid(NN, GRID_LOOP), gfull = capped_grid(NN, GRID_FULL);
    const double *z = t->elev;
    HIP_TRY(hipEventRecord(t->ev[6], t->stream));
    hipLaunchKernelGGL(k_dp_table_init, dim3((unsigned)cdiv(T * DT_SEAM_COLS, 256)), dim3(256), 0, t->stream, tab, T, (int)DT_SEAM_COLS);
    hipLaunchKernelGGL(k_ds_stats, dim3(gcells), dim3(256), 0, t->stream, (const int32_t *)t->fs_ids, z, (const double *)t->fs_W,
                       (const uint8_t *)d_out, (const uint8_t *)d_owner, (const int32_t *)d_lut, (const int32_t *)d_hid, (const double *)d_hW,
                       (const double *)d_ra, tab, T, n, m, sh_area, sh_vol);
    hipLaunchKernelGGL(k_ds_bottom, dim3(gfull), dim3(256), 0, t->stream, (const int32_t *)t->fs_ids, z, (const uint8_t *)d_owner,
                       (const int32_t *)d_lut, tab, T, NN);
    hipLaunchKernelGGL(k_dp_botelev, dim3((unsigned)cdiv(T, 256)), dim3(256), 0, t->stream, z, tab, T, NN);
    HIP_TRY(hipGetLastError());
    PYDEM_TRY(stage_elapsed(t, ms));
    PYDEM_TRY(tile_plane_copy(t, tab, table, (size_t)T * DT_SEAM_COLS * 8, true));
    return 0;
}

int stage_fill_seam_labels(pydem_tile *t, const int32_t *lut, int32_t *label, double *ms)
{
    const char *who = "pydem_fill_seam_labels";
    if (!t->fs_open || t->fs_K < 0) { pydem_set_error("%s: the open session has no labels (pydem_fill_seam_label first)", who); return -2; }
    if (!lut || !label) { pydem_set_error("%s: a NULL argument", who); return -2; }
    const int64_t NN = t->NN, K = t->fs_K;
    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    int32_t *d_lut = (int32_t *)arena_take(&lease, (size_t)(K + 1) * 4);
    int32_t *out = (int32_t *)arena_take(&lease, (size_t)NN * 4);
    if (!d_lut || !out) return -1;
    PYDEM_TRY(tile_plane_copy(t, d_lut, const_cast<int32_t *>(lut), (size_t)(K + 1) * 4, false));
    const int gfull = capped_grid(NN, GRID_FULL);
    HIP_TRY(hipEventRecord(t->ev[6], t->stream));
    hipLaunchKernelGGL(k_ds_write, dim3(gfull), dim3(256), 0, t->stream, (const int32_t *)t->fs_ids, (const int32_t *)d_lut, out, NN);
    HIP_TRY(hipGetLastError());
    PYDEM_TRY(stage_elapsed(t, ms));
    PYDEM_TRY(tile_plane_copy(t, out, label, (size_t)NN * 4, true));
    return 0;
}
