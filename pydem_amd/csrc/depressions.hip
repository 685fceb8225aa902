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
// last word of the scan: the last cell of the tile is a border cell, never raised.  k_dp_ids then turns the parent plane into the
// plane of ids 1..K (0 not raised, -1 no data) and stores each depression's level from its root cell.
// Statistics: k_dp_stats, one lane per cell.  Raised cells: the lanes of a wavefront that share an id reduce across the wavefront
// (xor shuffles) and their first lane issues the atomics -- one set per wavefront inside a large lake instead of 64.  Other
// finite cells look at their eight neighbours for the sill columns and drop duplicate ids in registers.  k_dp_bottom finds the
// smallest index among the cells at a depression's lowest z; k_dp_botelev copies that cell's elevation.
// The table is K rows of DT_COLS 64-bit words, column-major, in the conditioning arena; the host filters it, uploads the
// id -> kept id lookup, and k_dp_write produces the label plane.
#include "internal.h"
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <string.h>
#include <memory>

namespace {

constexpr int DP_B = 32;            // block edge of the local step (the fill's block)
constexpr int DP_T = 256;           // lanes per workgroup: 32 columns x 8 groups of 4 rows
constexpr int DP_R = DP_B * DP_B / DP_T;

// counter block, 64-bit words
enum { DPC_DEPTH = 0,   // bits of max (W - z)
       DPC_WORDS = 8 };

// table columns (64-bit words, column c of depression k at tab[c * K + k])
enum { DT_CELLS = 0, DT_R0, DT_R1, DT_C0, DT_C1,
       DT_ZMIN,         // order-preserving pattern of the lowest z (+0.0 for -0.0: they compare equal)
       DT_BOTTOM, DT_POUR, DT_NSILLS, DT_OPEN,
       DT_AREA, DT_VOLUME,      // fixed-point sums (int64 in two's complement; every term is >= 0)
       DT_SPILL, DT_BOTELEV,    // bits of doubles, plain stores
       DT_COLS };

typedef unsigned long long u64;

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
    for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(dmax, o); dmax = u > dmax ? u : dmax; }
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

__global__ void __launch_bounds__(256)
k_dp_table_init(u64 *tab, int64_t K)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K * DT_COLS) return;
    const int col = (int)(i / K);
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

__device__ inline int dp_wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ inline int dp_wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }
__device__ inline u64 dp_wave_min(u64 v) { for (int o = 32; o > 0; o >>= 1) { const u64 u = __shfl_xor(v, o); v = u < v ? u : v; } return v; }
__device__ inline u64 dp_wave_add(u64 v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }

__global__ void __launch_bounds__(256)
k_dp_stats(const int32_t *__restrict__ lab, const double *__restrict__ z, const double *__restrict__ W, const uint8_t *__restrict__ outlets,
           const double *__restrict__ dX2, const double *__restrict__ dY2, u64 *tab, int64_t K, int n, int m, int sh_area, int sh_vol)
{
    const int64_t NN = (int64_t)n * m;
    const int lane = (int)(threadIdx.x & 63);
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
        u64 zk = ~0ull, ai = 0, vi = 0;
        if (up) {
            const double a0 = dX2[r] * dY2[r];                  // row_area (k_row_area)
            zk = dp_key(zc + 0.0);
            ai = (u64)__double2ll_rn(ldexp(a0, sh_area));
            vi = (u64)__double2ll_rn(ldexp((W[c] - zc) * a0, sh_vol));
        }
        u64 todo = __ballot(up);
        while (todo) {                                          // (todo is the same in every lane)
            const int leader = __ffsll((long long)todo) - 1;
            const int lid = __shfl(id, leader);
            const bool mine = up && id == lid;
            const u64 mask = __ballot(mine);
            todo &= ~mask;
            int rmin = r, rmax = r, qmin = q, qmax = q;
            u64 cnt = 1, k = zk, a = ai, v = vi;
            if (mask != (1ull << leader)) {                     // more than one lane: reduce first (uniform branch)
                rmin = dp_wave_min(mine ? r : 0x7fffffff);
                rmax = dp_wave_max(mine ? r : -1);
                qmin = dp_wave_min(mine ? q : 0x7fffffff);
                qmax = dp_wave_max(mine ? q : -1);
                k = dp_wave_min(mine ? zk : ~0ull);
                a = dp_wave_add(mine ? ai : 0ull);
                v = dp_wave_add(mine ? vi : 0ull);
                cnt = (u64)__popcll(mask);
            }
            if (lane == leader) {
                u64 *row = tab + (lid - 1);
                atomicAdd(row + (int64_t)DT_CELLS * K, cnt);
                atomicMin(row + (int64_t)DT_R0 * K, (u64)rmin);
                atomicMax(row + (int64_t)DT_R1 * K, (u64)rmax);
                atomicMin(row + (int64_t)DT_C0 * K, (u64)qmin);
                atomicMax(row + (int64_t)DT_C1 * K, (u64)qmax);
                atomicMin(row + (int64_t)DT_ZMIN * K, k);
                atomicAdd(row + (int64_t)DT_AREA * K, a);
                atomicAdd(row + (int64_t)DT_VOLUME * K, v);
            }
        }
        // sills: a finite cell that is not raised, beside a depression whose level is this cell's elevation
        if (c < NN && id == 0) {
            int ids[8];
            bool open = r == 0 || r == n - 1 || q == 0 || q == m - 1;
            int found = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int dr = j < 3 ? -1 : (j < 5 ? 0 : 1);
                const int dq = j < 3 ? j - 1 : (j == 3 ? -1 : (j == 4 ? 1 : j - 6));
                const int rr = r + dr, qq = q + dq;
                ids[j] = 0;
                if (rr < 0 || rr >= n || qq < 0 || qq >= m) continue;
                const int64_t v = (int64_t)rr * m + qq;
                const int l = lab[v];
                if (l < 0) open = true;                         // beside no data
                else if (l > 0 && l <= K && W[v] == zc) { ids[j] = l; found = 1; }
            }
            if (found) {
                if (outlets && outlets[c] != 0) open = true;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    bool fresh = ids[j] > 0;
#pragma unroll
                    for (int i = 0; i < j; i++) fresh = fresh && ids[i] != ids[j];
                    if (fresh) {
                        u64 *row = tab + (ids[j] - 1);
                        atomicAdd(row + (int64_t)DT_NSILLS * K, 1ull);
                        atomicMin(row + (int64_t)DT_POUR * K, (u64)c);
                        if (open) atomicMax(row + (int64_t)DT_OPEN * K, 1ull);
                    }
                }
            }
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
k_dp_botelev(const double *__restrict__ z, u64 *tab, int64_t K, int64_t NN)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const u64 b = tab[(int64_t)DT_BOTTOM * K + k];
    if (b < (u64)NN) tab[(int64_t)DT_BOTELEV * K + k] = (u64)__double_as_longlong(z[b]);
}

__global__ void __launch_bounds__(256)
k_dp_write(const int32_t *__restrict__ lab, const int32_t *__restrict__ lut, int32_t *__restrict__ out, int64_t K, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int id = lab[c];
        out[c] = (id > 0 && id <= K) ? lut[id] : (id < 0 ? -1 : 0);
    }
}

double as_double(u64 b)
{
    double d;
    ::memcpy(&d, &b, 8);
    return d;
}

struct Events {
    hipEvent_t e[10] = {};
    int n = 0;
    ~Events() { for (int i = 0; i < n; i++) (void)hipEventDestroy(e[i]); }
};

// fraction bits and exponent of the fixed-point sums: B = min(40, 62 - ceil(log2(max(cells, 2)))), E from frexp of the largest term
void fixed_point(int64_t cells, double largest, int *shift, double *quantum)
{
    int lg = 0;
    const uint64_t x = (uint64_t)(cells < 2 ? 2 : cells) - 1;
    while (lg < 64 && (x >> lg)) lg++;                  // ceil(log2(x + 1))
    const int B = 62 - lg < 40 ? 62 - lg : 40;
    int E = 0;
    (void)frexp(largest, &E);
    *shift = B - E;
    *quantum = ldexp(1.0, E - B);
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
    const char *e = getenv("PYDEM_DEPR_LOCAL");                 // read per call: the tests switch it
    const bool local = !(e && *e && atoi(e) == 0);
    const int n = (int)t->n, m = (int)t->m;
    const int64_t NN = t->NN;

    Events ev;
    for (; ev.n < 9; ev.n++) HIP_TRY(hipEventCreate(&ev.e[ev.n]));
    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    FillRelax fr;
    double eps = 0.0;
    PYDEM_TRY(fill_relax(t, &lease, "pydem_depressions", &eps, outlets, ev.e[0], &fr));
    const double *W = fr.W;
    const double *z = t->elev;
    int32_t *parent = (int32_t *)arena_take(&lease, (size_t)NN * 4);
    int32_t *rank = (int32_t *)arena_take(&lease, (size_t)NN * 4);
    u64 *ctr = (u64 *)arena_take(&lease, DPC_WORDS * 8);
    size_t scan_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (int32_t *)nullptr, (int32_t *)nullptr, (int)NN, t->stream));
    void *scan_tmp = arena_take(&lease, scan_bytes);
    if (!parent || !rank || !ctr || !scan_tmp) return -1;

    const int gcells = (int)(cdiv(NN, 256) < 8192 ? cdiv(NN, 256) : 8192);
    const int gfull = (int)(cdiv(NN, 256) < (1 << 20) ? cdiv(NN, 256) : (1 << 20));
    HIP_TRY(hipEventRecord(ev.e[1], t->stream));                // relaxation done
    HIP_TRY(hipMemsetAsync(ctr, 0, DPC_WORDS * 8, t->stream));
    hipLaunchKernelGGL(k_dp_init, dim3(gcells), dim3(256), 0, t->stream, z, W, parent, NN, ctr);
    if (local) hipLaunchKernelGGL(k_dp_local, dim3((unsigned)cdiv(m, DP_B), (unsigned)cdiv(n, DP_B)), dim3(DP_T), 0, t->stream, parent, n, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[2], t->stream));
    hipLaunchKernelGGL(k_dp_merge, dim3(gfull), dim3(256), 0, t->stream, parent, n, m, local ? 0 : 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[3], t->stream));
    hipLaunchKernelGGL(k_dp_flatten, dim3(gfull), dim3(256), 0, t->stream, parent, rank, NN);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[4], t->stream));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, rank, rank, (int)NN, t->stream));
    // K and the largest depth
    volatile u64 *h = (volatile u64 *)t->h_counters;
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr, 8, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync(t->h_counters + 2, rank + (NN - 1), 4, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    const double depth_max = as_double(h[DPC_DEPTH]);
    const int64_t K = (int64_t)t->h_counters[2];        // (the last cell lies on the border: it is no root, so the exclusive sum there is the total)
    if (K < 0 || K > NN) { pydem_set_error("pydem_depressions: inconsistent count of depressions (%lld)", (long long)K); return -5; }

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
        hipLaunchKernelGGL(k_dp_table_init, dim3((unsigned)cdiv(K * DT_COLS, 256)), dim3(256), 0, t->stream, tab, K);
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
        for (int i = 0; i < 9; i++) {
            float el = 0.f;
            HIP_TRY(hipEventElapsedTime(&el, ev.e[from[i]], ev.e[to[i]]));
            ms[i] = (double)el;
        }
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

// the partial table: S_COLS columns of n_rows 64-bit words, column-major
enum { S_CELLS = 0, S_R0, S_R1, S_C0, S_C1, S_ZMIN, S_BOTTOM, S_POUR, S_NSILLS, S_OPEN, S_AREA, S_VOLUME, S_BOTELEV, S_COLS };

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

__global__ void __launch_bounds__(256)
k_ds_gather(const int32_t *__restrict__ src, int64_t pitch, int64_t cnt, int32_t *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i * pitch];
}

__global__ void __launch_bounds__(256)
k_ds_table_init(u64 *tab, int64_t T)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * S_COLS) return;
    const int col = (int)(i / T);
    const bool is_min = col == S_R0 || col == S_C0 || col == S_ZMIN || col == S_BOTTOM || col == S_POUR;
    tab[i] = is_min ? ~0ull : 0ull;
}

// k_dp_stats on the cells the tile owns, with rows through the lookup (several local ids may share a row) and the halo ring
__global__ void __launch_bounds__(256)
k_ds_stats(const int32_t *__restrict__ ids, const double *__restrict__ z, const double *__restrict__ W, const uint8_t *__restrict__ outlets,
           const uint8_t *__restrict__ owner, const int32_t *__restrict__ lut, const int32_t *__restrict__ halo_ids,
           const double *__restrict__ halo_W, const double *__restrict__ row_area, u64 *tab, int64_t T, int n, int m, int sh_area, int sh_vol)
{
    const int64_t NN = (int64_t)n * m;
    const int lane = (int)(threadIdx.x & 63);
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
        u64 zk = ~0ull, ai = 0, vi = 0;
        if (up) {
            const double a0 = row_area[r];
            zk = dp_key(zc + 0.0);
            ai = (u64)__double2ll_rn(ldexp(a0, sh_area));
            vi = (u64)__double2ll_rn(ldexp((W[c] - zc) * a0, sh_vol));
        }
        u64 todo = __ballot(up);
        while (todo) {                                          // (todo is the same in every lane)
            const int leader = __ffsll((long long)todo) - 1;
            const int lid = __shfl(g, leader);
            const bool mine = up && g == lid;
            const u64 mask = __ballot(mine);
            todo &= ~mask;
            int rmin = r, rmax = r, qmin = q, qmax = q;
            u64 cnt = 1, k = zk, a = ai, v = vi;
            if (mask != (1ull << leader)) {                     // more than one lane: reduce first (uniform branch)
                rmin = dp_wave_min(mine ? r : 0x7fffffff);
                rmax = dp_wave_max(mine ? r : -1);
                qmin = dp_wave_min(mine ? q : 0x7fffffff);
                qmax = dp_wave_max(mine ? q : -1);
                k = dp_wave_min(mine ? zk : ~0ull);
                a = dp_wave_add(mine ? ai : 0ull);
                v = dp_wave_add(mine ? vi : 0ull);
                cnt = (u64)__popcll(mask);
            }
            if (lane == leader) {
                u64 *row = tab + (lid - 1);
                atomicAdd(row + (int64_t)S_CELLS * T, cnt);
                atomicMin(row + (int64_t)S_R0 * T, (u64)rmin);
                atomicMax(row + (int64_t)S_R1 * T, (u64)rmax);
                atomicMin(row + (int64_t)S_C0 * T, (u64)qmin);
                atomicMax(row + (int64_t)S_C1 * T, (u64)qmax);
                atomicMin(row + (int64_t)S_ZMIN * T, k);
                atomicAdd(row + (int64_t)S_AREA * T, a);
                atomicAdd(row + (int64_t)S_VOLUME * T, v);
            }
        }
        // sills: an owned finite cell that is not raised, beside a depression whose level is this cell's elevation; its whole 3 x 3
        // is known here, so it is open exactly when a neighbour is no data or uncovered (-1), or when it is an outlet
        if (c < NN && own && l == 0) {
            int gs[8];
            bool open = false;
            int found = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int dr = j < 3 ? -1 : (j < 5 ? 0 : 1);
                const int dq = j < 3 ? j - 1 : (j == 3 ? -1 : (j == 4 ? 1 : j - 6));
                const int rr = r + dr, qq = q + dq;
                gs[j] = 0;
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
                else if (gv > 0 && wv == zc) { gs[j] = gv; found = 1; }
            }
            if (found) {
                if (outlets && outlets[c] != 0) open = true;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    bool fresh = gs[j] > 0;
#pragma unroll
                    for (int i = 0; i < j; i++) fresh = fresh && gs[i] != gs[j];
                    if (fresh) {
                        u64 *row = tab + (gs[j] - 1);
                        atomicAdd(row + (int64_t)S_NSILLS * T, 1ull);
                        atomicMin(row + (int64_t)S_POUR * T, (u64)c);
                        if (open) atomicMax(row + (int64_t)S_OPEN * T, 1ull);
                    }
                }
            }
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
        if (z[c] == dp_unkey(tab[(int64_t)S_ZMIN * T + g - 1])) atomicMin(tab + (int64_t)S_BOTTOM * T + g - 1, (u64)c);
    }
}

__global__ void __launch_bounds__(256)
k_ds_botelev(const double *__restrict__ z, u64 *tab, int64_t T, int64_t NN)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= T) return;
    const u64 b = tab[(int64_t)S_BOTTOM * T + k];
    if (b < (u64)NN) tab[(int64_t)S_BOTELEV * T + k] = (u64)__double_as_longlong(z[b]);
}

__global__ void __launch_bounds__(256)
k_ds_write(const int32_t *__restrict__ ids, const int32_t *__restrict__ lut, int32_t *__restrict__ out, int64_t NN)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < NN; c += (int64_t)gridDim.x * blockDim.x) {
        const int l = ids[c];
        out[c] = l > 0 ? lut[l] : l;
    }
}

int seam_elapsed(pydem_tile *t, double *ms)
{
    HIP_TRY(hipEventRecord(t->ev[7], t->stream));
    HIP_TRY(hipEventSynchronize(t->ev[7]));
    float el = 0.f;
    HIP_TRY(hipEventElapsedTime(&el, t->ev[6], t->ev[7]));
    if (ms) *ms = (double)el;
    return 0;
}

}  // namespace

int stage_fill_seam_label(pydem_tile *t, int64_t *n_local, double *max_depth, double *ms)
{
    const char *who = "pydem_fill_seam_label";
    if (!t->fs_open) { pydem_set_error("%s: no session is open on this tile (pydem_fill_seam_begin first)", who); return -2; }
    if (t->NN >= (int64_t)INT32_MAX) { pydem_set_error("%s: %lld cells do not fit the int32 id plane", who, (long long)t->NN); return -2; }
    const char *e = getenv("PYDEM_DEPR_LOCAL");                 // read per call: the tests switch it
    const bool local = !(e && *e && atoi(e) == 0);
    const int n = (int)t->n, m = (int)t->m;
    const int64_t NN = t->NN;
    if (!t->fs_ids) PYDEM_TRY(tile_hold(t, (void **)&t->fs_ids, (size_t)NN * 4, true));
    t->fs_K = -1;
    t->fs_roots.clear();
    t->fs_levels.clear();

    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    int32_t *parent = t->fs_ids;
    int32_t *rank = (int32_t *)arena_take(&lease, (size_t)NN * 4);
    u64 *ctr = (u64 *)arena_take(&lease, DPC_WORDS * 8);
    size_t scan_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (int32_t *)nullptr, (int32_t *)nullptr, (int)NN, t->stream));
    void *scan_tmp = arena_take(&lease, scan_bytes);
    if (!rank || !ctr || !scan_tmp) return -1;
    const double *W = t->fs_W;
    const double *z = t->elev;
    const int gcells = (int)(cdiv(NN, 256) < 8192 ? cdiv(NN, 256) : 8192);
    const int gfull = (int)(cdiv(NN, 256) < (1 << 20) ? cdiv(NN, 256) : (1 << 20));
    HIP_TRY(hipEventRecord(t->ev[6], t->stream));
    HIP_TRY(hipMemsetAsync(ctr, 0, DPC_WORDS * 8, t->stream));
    hipLaunchKernelGGL(k_dp_init, dim3(gcells), dim3(256), 0, t->stream, z, W, parent, NN, ctr);
    if (local) hipLaunchKernelGGL(k_dp_local, dim3((unsigned)cdiv(m, DP_B), (unsigned)cdiv(n, DP_B)), dim3(DP_T), 0, t->stream, parent, n, m);
    hipLaunchKernelGGL(k_dp_merge, dim3(gfull), dim3(256), 0, t->stream, parent, n, m, local ? 0 : 1);
    hipLaunchKernelGGL(k_dp_flatten, dim3(gfull), dim3(256), 0, t->stream, parent, rank, NN);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, rank, rank, (int)NN, t->stream));
    // K and the largest depth.  A seam cell may be raised, the tile's last cell included: it counts when it is its own root
    volatile u64 *h = (volatile u64 *)t->h_counters;
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr, 8, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync(t->h_counters + 2, rank + (NN - 1), 4, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipMemcpyAsync(t->h_counters + 3, parent + (NN - 1), 4, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    const double depth_max = as_double(h[DPC_DEPTH]);
    const int64_t K = (int64_t)t->h_counters[2] + ((int64_t)t->h_counters[3] == NN - 1 ? 1 : 0);
    if (K < 0 || K > NN) { pydem_set_error("%s: inconsistent count of depressions (%lld)", who, (long long)K); return -5; }
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
    hipLaunchKernelGGL(k_ds_ids, dim3(gfull), dim3(256), 0, t->stream, parent, (const int32_t *)rank, W, roots, levels, K, NN);
    HIP_TRY(hipGetLastError());
    PYDEM_TRY(seam_elapsed(t, ms));
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
    if (count <= 0) return 0;
    const size_t Lmax = (size_t)(t->n > t->m ? t->n : t->m);
    int ncols = 0;
    for (int k = 0; k < count; k++) {
        const int64_t lim = axes[k] == 0 ? t->n : t->m;
        if ((axes[k] != 0 && axes[k] != 1) || indices[k] < -lim || indices[k] >= lim) { pydem_set_error("%s: line index out of range", who); return -2; }
        if (axes[k] == 1) ncols++;
    }
    ArenaLease lease;
    int32_t *stage = nullptr;
    if (ncols) {
        PYDEM_TRY(arena_acquire(t->device, &lease));
        stage = (int32_t *)arena_take(&lease, (size_t)ncols * (size_t)t->n * 4);
        if (!stage) return -1;
    }
    void *pin_v = nullptr;
    PYDEM_TRY(tile_pinned(t, (size_t)count * Lmax * 4, &pin_v));
    char *pin = (char *)pin_v;
    int col = 0;
    for (int k = 0; k < count; k++) {
        const int64_t lim = axes[k] == 0 ? t->n : t->m;
        const int64_t index = indices[k] < 0 ? indices[k] + lim : indices[k];
        if (axes[k] == 0) {
            HIP_TRY(hipMemcpyAsync(pin + (size_t)k * Lmax * 4, t->fs_ids + (size_t)index * t->m, (size_t)t->m * 4, hipMemcpyDeviceToHost, t->stream));
        } else {
            int32_t *dst = stage + (size_t)col++ * (size_t)t->n;
            const int g = (int)(cdiv(t->n, 256) < 64 ? cdiv(t->n, 256) : 64);
            hipLaunchKernelGGL(k_ds_gather, dim3(g), dim3(256), 0, t->stream, (const int32_t *)(t->fs_ids + index), t->m, t->n, dst);
            HIP_TRY(hipMemcpyAsync(pin + (size_t)k * Lmax * 4, dst, (size_t)t->n * 4, hipMemcpyDeviceToHost, t->stream));
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    for (int k = 0; k < count; k++) memcpy(dsts[k], pin + (size_t)k * Lmax * 4, (size_t)(axes[k] == 0 ? t->m : t->n) * 4);
    return 0;
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
    u64 *tab = (u64 *)arena_take(&lease, (size_t)T * S_COLS * 8);
    if (!d_lut || !d_owner || (outlets && !d_out) || !d_hid || !d_hW || !d_ra || !tab) return -1;
    PYDEM_TRY(tile_plane_copy(t, d_lut, const_cast<int32_t *>(lut), (size_t)(K + 1) * 4, false));
    PYDEM_TRY(tile_plane_copy(t, d_owner, const_cast<uint8_t *>(owner), (size_t)NN, false));
    if (outlets) PYDEM_TRY(tile_plane_copy(t, d_out, const_cast<uint8_t *>(outlets), (size_t)NN, false));
    PYDEM_TRY(tile_plane_copy(t, d_hid, const_cast<int32_t *>(halo_ids), R * 4, false));
    PYDEM_TRY(tile_plane_copy(t, d_hW, const_cast<double *>(halo_W), R * 8, false));
    PYDEM_TRY(tile_plane_copy(t, d_ra, const_cast<double *>(row_area), (size_t)n * 8, false));

    const int gcells = (int)(cdiv(NN, 256) < 8192 ? cdiv(NN, 256) : 8192);
    const int gfull = (int)(cdiv(NN, 256) < (1 << 20) ? cdiv(NN, 256) : (1 << 20));
    const double *z = t->elev;
    HIP_TRY(hipEventRecord(t->ev[6], t->stream));
    hipLaunchKernelGGL(k_ds_table_init, dim3((unsigned)cdiv(T * S_COLS, 256)), dim3(256), 0, t->stream, tab, T);
    hipLaunchKernelGGL(k_ds_stats, dim3(gcells), dim3(256), 0, t->stream, (const int32_t *)t->fs_ids, z, (const double *)t->fs_W,
                       (const uint8_t *)d_out, (const uint8_t *)d_owner, (const int32_t *)d_lut, (const int32_t *)d_hid, (const double *)d_hW,
                       (const double *)d_ra, tab, T, n, m, sh_area, sh_vol);
    hipLaunchKernelGGL(k_ds_bottom, dim3(gfull), dim3(256), 0, t->stream, (const int32_t *)t->fs_ids, z, (const uint8_t *)d_owner,
                       (const int32_t *)d_lut, tab, T, NN);
    hipLaunchKernelGGL(k_ds_botelev, dim3((unsigned)cdiv(T, 256)), dim3(256), 0, t->stream, z, tab, T, NN);
    HIP_TRY(hipGetLastError());
    PYDEM_TRY(seam_elapsed(t, ms));
    PYDEM_TRY(tile_plane_copy(t, tab, table, (size_t)T * S_COLS * 8, true));
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
    const int gfull = (int)(cdiv(NN, 256) < (1 << 20) ? cdiv(NN, 256) : (1 << 20));
    HIP_TRY(hipEventRecord(t->ev[6], t->stream));
    hipLaunchKernelGGL(k_ds_write, dim3(gfull), dim3(256), 0, t->stream, (const int32_t *)t->fs_ids, (const int32_t *)d_lut, out, NN);
    HIP_TRY(hipGetLastError());
    PYDEM_TRY(seam_elapsed(t, ms));
    PYDEM_TRY(tile_plane_copy(t, out, label, (size_t)NN * 4, true));
    return 0;
}
