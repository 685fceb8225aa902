// cyutils.hip -- the reference's ONLY native boundary, kept callable as it is:
//   pydem/cyfuncs/cyutils.pyx:35-46   drain_connections(arr, ids, indptr, indices, set_to)
//   pydem/cyfuncs/cyutils.pyx:78-116  drain_area(area, done, ids, col_indptr, col_indices, col_data,
//                                                row_indptr, row_indices, n_rows, n_cols,
//                                                edge_todo, edge_todo_no_mask, skip_edge)
// over a GENERIC sparse graph in scipy CSC/CSR form (the DEMProcessor path above never builds that
// matrix; this shim exists so code written against the Cython module keeps working).  Semantics follow
// the Cython loops (:49-72, :119-187) round for round: level-synchronous PUSH, `done` marked before a
// round's pushes, a target that is already done and lies on the tile edge is skipped, a target becomes
// part of the next frontier when all its CSR upstream cells are done, and the loop ends when the
// frontier repeats itself (normally: is empty).  Differences: frontiers are lists (the Cython code
// rescans all N cells four times per round).
// What is guaranteed: area, done, the taints and the final ids are those of the Cython loops bit for bit,
// and bit-identical run to run, on every input on which those loops end (they do not end on every
// input, and then neither does this).  How:
//  * The Cython loop walks the frontier in ascending id and every push reads the CURRENT value of its
//    source.  As long as no accepted target of a round is itself in the round's frontier, no push reads a
//    value written in its round, and only the order of the additions into one target shows: the round
//    collects its targets, then every target PULLS over its CSR row from the sources that are in the
//    frontier -- ascending source id, a source's entries in column order -- without floating-point
//    atomics.  This needs CSR rows of sorted, unique source ids; the Python wrapper brings them to that
//    form (the reference uses the CSR only as a set).
//  * A round in which an accepted target IS in the running frontier (cells that drain into each other
//    and were seeded together, a chain seeded along its length: what the reference's re-seed after a
//    stall does on level ground) is run in the Cython order on the host: k_cy_targets raises a flag that
//    rides on the target counter's readback, the state comes down, one plain C++ loop walks the sorted
//    frontier, and the state goes back up (cy_ordered_round).
#include "internal.h"
#include <string.h>
#include <algorithm>

namespace {

__device__ __forceinline__ bool cy_on_edge(int64_t id, int64_t n_rows, int64_t n_cols)   // cyutils.pyx:207-226
{
    return id < n_cols || id >= n_cols * n_rows - n_cols || id % n_cols == 0 || id % n_cols == n_cols - 1;
}

__global__ void k_cy_mark_done(const int32_t *__restrict__ front, int32_t nf, uint8_t *done, int32_t *mark, int32_t tag)
{
    for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nf; q += gridDim.x * blockDim.x) {
        if (done) done[front[q]] = 1;      // :138-140
        mark[front[q]] = tag - 1;          // members of the current frontier (to recognise a repeating frontier)
    }
}

// a list slot for every lane that is active here, ONE atomic per wavefront: the list counters are single addresses, and
// one returning atomic per pushed node serialises in the L2 (~10 ns each)
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

// phase 1 of a round: the distinct targets of the frontier (cyutils.pyx:155-161), and whether one of them is a member of it
__global__ void k_cy_targets(const int32_t *__restrict__ front, int32_t nf, const uint8_t *__restrict__ done,
                             const int32_t *__restrict__ col_indptr, const int32_t *__restrict__ col_indices, int64_t n_rows,
                             int64_t n_cols, int skip_edge, int32_t *tmark, int32_t tag, int32_t *targets, int32_t *n_targets,
                             const int32_t *__restrict__ mark, int32_t *in_front)
{
    for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nf; q += gridDim.x * blockDim.x) {
        const int32_t i = front[q];
        for (int32_t j = col_indptr[i]; j < col_indptr[i + 1]; j++) {
            const int32_t row = col_indices[j];
            if ((skip_edge || done[row]) && cy_on_edge(row, n_rows, n_cols)) continue;          // :159-161
            if (mark[row] == tag - 1) *in_front = 1;      // a target inside the running frontier: the round needs the Cython order
            if (atomicExch(&tmark[row], tag) != tag) targets[agg_slot(n_targets)] = row;
        }
    }
}

// phase 2: every target adds what the frontier sends it, in ascending source order (:163-168), then checks
// whether all of its upstream cells are done (:173-179)
__global__ void k_cy_pull(const int32_t *__restrict__ targets, int32_t nt, double *area, const uint8_t *__restrict__ done,
                          const int32_t *__restrict__ col_indptr, const int32_t *__restrict__ col_indices,
                          const double *__restrict__ col_data, const int32_t *__restrict__ row_indptr,
                          const int32_t *__restrict__ row_indices, double *edge_todo, double *edge_todo_nm,
                          int32_t *mark, int32_t tag, int32_t *next, int32_t *n_next, int32_t *n_repeat)
{
    for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nt; q += gridDim.x * blockDim.x) {
        const int32_t row = targets[q];
        double a = area[row];
        double t = edge_todo ? edge_todo[row] : 0.0, tn = edge_todo_nm ? edge_todo_nm[row] : 0.0;
        bool wait = false;
        for (int32_t k = row_indptr[row]; k < row_indptr[row + 1]; k++) {
            const int32_t src = row_indices[k];
            if (mark[src] == tag - 1) {                      // a member of this round's frontier: its push, :163
                for (int32_t j = col_indptr[src]; j < col_indptr[src + 1]; j++) {
                    if (col_indices[j] != row) continue;
                    const double w = col_data[j];
                    a += area[src] * w;
                    if (edge_todo) t += edge_todo[src] * w;
                    if (edge_todo_nm) tn += edge_todo_nm[src] * w;
                }
            }
            if (!done[src]) wait = true;
        }
        area[row] = a;
        if (edge_todo) edge_todo[row] = t;
        if (edge_todo_nm) edge_todo_nm[row] = tn;
        if (!wait) {
            const int32_t old = atomicExch(&mark[row], tag);
            if (old != tag) {
                next[agg_slot(n_next)] = row;
                if (old == tag - 1) atomicAdd(n_repeat, 1);                                      // was in the previous frontier too
            }
        }
    }
}

__global__ void k_cy_flood(const int32_t *__restrict__ front, int32_t nf, int32_t *arr, const int32_t *__restrict__ indptr,
                           const int32_t *__restrict__ indices, int32_t set_to, int32_t *mark, int32_t tag, int32_t *next,
                           int32_t *n_next, int32_t *n_repeat)
{
    for (int32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nf; q += gridDim.x * blockDim.x) {
        const int32_t i = front[q];
        for (int32_t j = indptr[i]; j < indptr[i + 1]; j++) {
            const int32_t row = indices[j];
            if (atomicExch(&arr[row], set_to) != set_to) {                                       // :69-70
                const int32_t old = atomicExch(&mark[row], tag);
                if (old != tag) { next[agg_slot(n_next)] = row; if (old == tag - 1) atomicAdd(n_repeat, 1); }
            }
        }
    }
}

int front_from_mask(const uint8_t *mask, int64_t n, std::vector<int32_t> &out)
{
    out.clear();
    for (int64_t i = 0; i < n; i++) if (mask[i]) out.push_back((int32_t)i);
    return 0;
}

// One round in the Cython order (:151-185) on host copies of the state: the frontier in ascending id, every push reading the
// current value of its source.  `stamp` (N entries, zero before the call's first ordered round) plays the part of the device
// marks: tag - 1 for the members of the running frontier, tag for those of the next.
void cy_ordered_round(std::vector<int32_t> &front, double *area, const uint8_t *done, const int32_t *col_indptr,
                      const int32_t *col_indices, const double *col_data, const int32_t *row_indptr, const int32_t *row_indices,
                      int64_t n_rows, int64_t n_cols, double *edge_todo, double *edge_todo_nm, int skip_edge,
                      std::vector<int32_t> &stamp, int32_t tag, std::vector<int32_t> &next, int32_t *n_repeat)
{
    std::sort(front.begin(), front.end());
    for (int32_t i : front) stamp[(size_t)i] = tag - 1;
    next.clear();
    *n_repeat = 0;
    for (int32_t i : front)
        for (int32_t j = col_indptr[i]; j < col_indptr[i + 1]; j++) {
            const int64_t row = col_indices[j];
            const double w = col_data[j];
            if ((skip_edge || done[row]) && (row < n_cols || row >= n_cols * n_rows - n_cols || row % n_cols == 0 ||
                                             row % n_cols == n_cols - 1)) continue;                 // :159-161
            area[row] += area[i] * w;                                                                // :163
            if (edge_todo) edge_todo[row] += edge_todo[i] * w;
            if (edge_todo_nm) edge_todo_nm[row] += edge_todo_nm[i] * w;
            bool wait = false;
            for (int32_t k = row_indptr[row]; k < row_indptr[row + 1] && !wait; k++) wait = !done[row_indices[k]];   // :173-179
            if (wait || stamp[(size_t)row] == tag) continue;
            if (stamp[(size_t)row] == tag - 1) ++*n_repeat;
            stamp[(size_t)row] = tag;
            next.push_back((int32_t)row);
        }
}

}  // namespace

extern "C" {

int pydem_drain_area(double *area, uint8_t *done, uint8_t *ids, const int32_t *col_indptr, const int32_t *col_indices,
                     const double *col_data, const int32_t *row_indptr, const int32_t *row_indices, int64_t n_rows,
                     int64_t n_cols, double *edge_todo, double *edge_todo_no_mask, int skip_edge, int device)
{
    HIP_TRY(hipSetDevice(device));
    const int64_t N = n_rows * n_cols;
    if (N >= INT32_MAX) { pydem_set_error("graph too large for int32 ids"); return -2; }
    const int64_t nnz = col_indptr[N];
    const int64_t nnz_r = row_indptr[N];      // rows of unique sources: fewer entries than the CSC where it lists an edge twice
    DevTemp d_area, d_done, d_cp, d_ci, d_cd, d_rp, d_ri, d_et, d_etn, d_mark, d_q0, d_q1, d_cnt, d_tmark, d_targets;
    PYDEM_TRY(d_area.alloc(N * 8)); PYDEM_TRY(d_done.alloc(N)); PYDEM_TRY(d_cp.alloc((N + 1) * 4)); PYDEM_TRY(d_ci.alloc(nnz * 4));
    PYDEM_TRY(d_cd.alloc(nnz * 8)); PYDEM_TRY(d_rp.alloc((N + 1) * 4)); PYDEM_TRY(d_ri.alloc(nnz_r * 4));
    PYDEM_TRY(d_mark.alloc(N * 4)); PYDEM_TRY(d_q0.alloc(N * 4)); PYDEM_TRY(d_q1.alloc(N * 4)); PYDEM_TRY(d_cnt.alloc(16));
    PYDEM_TRY(d_tmark.alloc(N * 4)); PYDEM_TRY(d_targets.alloc(N * 4));
    if (edge_todo) PYDEM_TRY(d_et.alloc(N * 8));
    if (edge_todo_no_mask) PYDEM_TRY(d_etn.alloc(N * 8));
    HIP_TRY(hipMemcpy(d_area.p, area, N * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_done.p, done, N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_cp.p, col_indptr, (N + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ci.p, col_indices, nnz * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_cd.p, col_data, nnz * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_rp.p, row_indptr, (N + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ri.p, row_indices, nnz_r * 4, hipMemcpyHostToDevice));
    if (edge_todo) HIP_TRY(hipMemcpy(d_et.p, edge_todo, N * 8, hipMemcpyHostToDevice));
    if (edge_todo_no_mask) HIP_TRY(hipMemcpy(d_etn.p, edge_todo_no_mask, N * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_mark.p, 0, N * 4));
    HIP_TRY(hipMemset(d_tmark.p, 0, N * 4));
    std::vector<int32_t> front;
    front_from_mask(ids, N, front);
    int32_t nf = (int32_t)front.size();
    HIP_TRY(hipMemcpy(d_q0.p, front.data(), (size_t)nf * 4, hipMemcpyHostToDevice));
    int32_t *q[2] = {d_q0.as<int32_t>(), d_q1.as<int32_t>()};
    int32_t tag = 2;      // marks: tag of the round in which a cell entered a frontier
    int cur = 0;
    // (the initial frontier carries tag 1 so that "same frontier again" can be recognised in round 1)
    std::vector<int32_t> stamp, next;      // host side of an ordered round
    for (int64_t r = 0;; r++) {
        int32_t n_next = 0, n_rep = 0;
        if (nf > 0) {
            const int g = (int)(cdiv(nf, 256) < 2048 ? cdiv(nf, 256) : 2048);
            hipLaunchKernelGGL(k_cy_mark_done, dim3(g), dim3(256), 0, 0, q[cur], nf, d_done.as<uint8_t>(), d_mark.as<int32_t>(), tag);
            HIP_TRY(hipMemset(d_cnt.p, 0, 16));
            hipLaunchKernelGGL(k_cy_targets, dim3(g), dim3(256), 0, 0, q[cur], nf, d_done.as<uint8_t>(), d_cp.as<int32_t>(), d_ci.as<int32_t>(),
                               n_rows, n_cols, skip_edge, d_tmark.as<int32_t>(), tag, d_targets.as<int32_t>(), d_cnt.as<int32_t>() + 2,
                               d_mark.as<int32_t>(), d_cnt.as<int32_t>() + 3);
            int32_t tc[2] = {0, 0};       // targets, and whether one of them is in the running frontier
            HIP_TRY(hipMemcpy(tc, d_cnt.as<int32_t>() + 2, 8, hipMemcpyDeviceToHost));
            const int32_t nt = tc[0];
            if (tc[1]) {
                // the Cython order, on the host, in the caller's arrays (they take the results at the end anyway)
                HIP_TRY(hipMemcpy(area, d_area.p, N * 8, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(done, d_done.p, N, hipMemcpyDeviceToHost));
                if (edge_todo) HIP_TRY(hipMemcpy(edge_todo, d_et.p, N * 8, hipMemcpyDeviceToHost));
                if (edge_todo_no_mask) HIP_TRY(hipMemcpy(edge_todo_no_mask, d_etn.p, N * 8, hipMemcpyDeviceToHost));
                front.resize((size_t)nf);
                HIP_TRY(hipMemcpy(front.data(), q[cur], (size_t)nf * 4, hipMemcpyDeviceToHost));
                if (stamp.empty()) stamp.assign((size_t)N, 0);
                cy_ordered_round(front, area, done, col_indptr, col_indices, col_data, row_indptr, row_indices, n_rows, n_cols,
                                 edge_todo, edge_todo_no_mask, skip_edge, stamp, tag, next, &n_rep);
                n_next = (int32_t)next.size();
                HIP_TRY(hipMemcpy(d_area.p, area, N * 8, hipMemcpyHostToDevice));
                if (edge_todo) HIP_TRY(hipMemcpy(d_et.p, edge_todo, N * 8, hipMemcpyHostToDevice));
                if (edge_todo_no_mask) HIP_TRY(hipMemcpy(d_etn.p, edge_todo_no_mask, N * 8, hipMemcpyHostToDevice));
                if (n_next > 0) HIP_TRY(hipMemcpy(q[1 - cur], next.data(), (size_t)n_next * 4, hipMemcpyHostToDevice));
            } else {
                if (nt > 0) {
                    const int gt = (int)(cdiv(nt, 256) < 2048 ? cdiv(nt, 256) : 2048);
                    hipLaunchKernelGGL(k_cy_pull, dim3(gt), dim3(256), 0, 0, d_targets.as<int32_t>(), nt, d_area.as<double>(), d_done.as<uint8_t>(),
                                       d_cp.as<int32_t>(), d_ci.as<int32_t>(), d_cd.as<double>(), d_rp.as<int32_t>(), d_ri.as<int32_t>(),
                                       edge_todo ? d_et.as<double>() : nullptr, edge_todo_no_mask ? d_etn.as<double>() : nullptr,
                                       d_mark.as<int32_t>(), tag, q[1 - cur], d_cnt.as<int32_t>(), d_cnt.as<int32_t>() + 1);
                }
                HIP_TRY(hipGetLastError());
                int32_t h[2];
                HIP_TRY(hipMemcpy(h, d_cnt.p, 8, hipMemcpyDeviceToHost));
                n_next = h[0]; n_rep = h[1];
            }
        }
        // keep_going = (ids != ids_old)  (:187): stop when the new frontier equals the old one
        const bool same = (n_next == nf) && (n_rep == n_next);
        cur = 1 - cur; nf = n_next; tag++;
        if (same) break;
        if (r > (1ll << 31)) { pydem_set_error("drain_area did not terminate"); return -5; }
    }
    HIP_TRY(hipMemcpy(area, d_area.p, N * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(done, d_done.p, N, hipMemcpyDeviceToHost));
    if (edge_todo) HIP_TRY(hipMemcpy(edge_todo, d_et.p, N * 8, hipMemcpyDeviceToHost));
    if (edge_todo_no_mask) HIP_TRY(hipMemcpy(edge_todo_no_mask, d_etn.p, N * 8, hipMemcpyDeviceToHost));
    // final frontier back into ids (callers overwrite it, dem_processing.py:962)
    memset(ids, 0, (size_t)N);
    if (nf > 0) {
        front.resize((size_t)nf);
        HIP_TRY(hipMemcpy(front.data(), q[cur], (size_t)nf * 4, hipMemcpyDeviceToHost));
        for (int32_t v : front) ids[v] = 1;
    }
    return 0;
}

int pydem_drain_connections(uint8_t *arr, uint8_t *ids, const int32_t *indptr, const int32_t *indices, int64_t n,
                            uint8_t set_to, int device)
{
    HIP_TRY(hipSetDevice(device));
    if (n >= INT32_MAX) { pydem_set_error("graph too large for int32 ids"); return -2; }
    const int64_t nnz = indptr[n];
    DevTemp d_arr, d_p, d_i, d_mark, d_q0, d_q1, d_cnt;
    PYDEM_TRY(d_arr.alloc(n * 4)); PYDEM_TRY(d_p.alloc((n + 1) * 4)); PYDEM_TRY(d_i.alloc(nnz * 4)); PYDEM_TRY(d_mark.alloc(n * 4));
    PYDEM_TRY(d_q0.alloc(n * 4)); PYDEM_TRY(d_q1.alloc(n * 4)); PYDEM_TRY(d_cnt.alloc(16));
    std::vector<int32_t> a32((size_t)n);
    for (int64_t k = 0; k < n; k++) a32[(size_t)k] = arr[k];
    HIP_TRY(hipMemcpy(d_arr.p, a32.data(), n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_p.p, indptr, (n + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_i.p, indices, nnz * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_mark.p, 0, n * 4));
    std::vector<int32_t> front;
    front_from_mask(ids, n, front);
    int32_t nf = (int32_t)front.size();
    HIP_TRY(hipMemcpy(d_q0.p, front.data(), (size_t)nf * 4, hipMemcpyHostToDevice));
    int32_t *q[2] = {d_q0.as<int32_t>(), d_q1.as<int32_t>()};
    int32_t tag = 2;
    int cur = 0;
    for (;;) {
        HIP_TRY(hipMemset(d_cnt.p, 0, 16));
        if (nf > 0) {
            const int g = (int)(cdiv(nf, 256) < 2048 ? cdiv(nf, 256) : 2048);
            hipLaunchKernelGGL(k_cy_mark_done, dim3(g), dim3(256), 0, 0, q[cur], nf, (uint8_t *)nullptr, d_mark.as<int32_t>(), tag);
            hipLaunchKernelGGL(k_cy_flood, dim3(g), dim3(256), 0, 0, q[cur], nf, d_arr.as<int32_t>(), d_p.as<int32_t>(),
                               d_i.as<int32_t>(), (int32_t)set_to, d_mark.as<int32_t>(), tag, q[1 - cur], d_cnt.as<int32_t>(),
                               d_cnt.as<int32_t>() + 1);
            HIP_TRY(hipGetLastError());
        }
        int32_t h[2];
        HIP_TRY(hipMemcpy(h, d_cnt.p, 8, hipMemcpyDeviceToHost));
        const bool same = (h[0] == nf) && (h[1] == h[0]);
        cur = 1 - cur; nf = h[0]; tag++;
        if (same) break;
    }
    HIP_TRY(hipMemcpy(a32.data(), d_arr.p, n * 4, hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < n; k++) arr[k] = (uint8_t)a32[(size_t)k];
    memset(ids, 0, (size_t)n);
    return 0;
}

}  // extern "C"
