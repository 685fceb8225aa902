// stage_kit.h -- what the stand-alone stages beside the step share: terrain.hip, horizon.hip, hand_table.hip, depressions.hip and
// fill_depressions.hip.  Device side: the 64-lane reductions, the walk over the
// distinct keys of a wavefront, the slotted counter.  Host side: the event set, the fixed-point format
// of the integer sums, the capped grid, the PYDEM_* switches, the lines of a held plane.  Everything has internal linkage: a
// kernel of this header is a kernel of every unit that launches it.
#pragma once
#include "internal.h"
#include "line_gather.h"
#include <math.h>
#include <string.h>

namespace {

typedef unsigned long long u64;

// ---- device: reductions over the 64 lanes (xor butterfly: every lane ends with the result) ----
__device__ __forceinline__ u64 wave_add(u64 v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ u64 wave_min(u64 v) { for (int o = 32; o > 0; o >>= 1) { const u64 u = __shfl_xor(v, o); v = u < v ? u : v; } return v; }
__device__ __forceinline__ u64 wave_max(u64 v) { for (int o = 32; o > 0; o >>= 1) { const u64 u = __shfl_xor(v, o); v = u > v ? u : v; } return v; }
__device__ __forceinline__ int wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ int wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ double wave_max(double v) { for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(v, o); v = u > v ? u : v; } return v; }

// The walk over the distinct keys of a wavefront's active lanes, in the order of their first lanes: f(key, leader, mask, mine,
// lone) once per key, by all 64 lanes together -- leader: the first lane that holds the key; mask: the lanes that hold it; mine:
// this lane is one of them; lone: the leader is the only one.  Every argument but `mine` is the same in every lane, so a branch
// on `lone` is uniform and f may reduce across the wavefront (mine ? term : neutral) under it; the leader then issues ONE set of
// integer atomics per key and wavefront instead of one per lane, and a lone lane publishes its own terms without the shuffles.
// The call must be reached by the whole wavefront (a loop over cells that is uniform per wavefront).
template <typename Key, typename F>
__device__ __forceinline__ void wave_by_key(bool act, Key key, F f)
{
    u64 todo = __ballot(act);
    while (todo) {                                          // (todo is the same in every lane)
        const int leader = __ffsll((long long)todo) - 1;
        const Key lkey = __shfl(key, leader);
        const bool mine = act && key == lkey;
        const u64 mask = __ballot(mine);
        todo &= ~mask;
        f(lkey, leader, mask, mine, mask == (1ull << leader));
    }
}

// The slotted counter: SLOTS words 128 bytes apart take the atomics (a million additions to ONE address cost 7 ms on the 16384^2
// tile, more than the arithmetic of a 15 x 15 window), and k_slot_total adds them into the word SLOT_TOTAL.  Integers: any order
// gives the same count.  The block is SLOT_BYTES, zeroed by the caller.
constexpr int SLOTS = 64, SLOT_WORDS = 16, SLOT_TOTAL = 8, SLOT_BYTES = SLOTS * SLOT_WORDS * 8;

// one 64-bit atomic per wavefront; `slot`: any number that spreads the wavefronts (uniform per wavefront)
__device__ __forceinline__ void slot_count_wave(u64 *ctr, u64 mine, int slot)
{
    mine = wave_add(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(ctr + (slot & (SLOTS - 1)) * SLOT_WORDS, mine);
}

// Per workgroup: slot_count_begin() in the kernel's first lines zeroes the workgroup's LDS word (8 bytes of a kernel that counts);
// slot_count, reached by the whole workgroup behind at least one barrier of the kernel's after that, takes each wavefront's count
// (wave_add) with an integer LDS atomic and issues one global atomic.  (Zeroing the word inside slot_count behind a barrier of its
// own, or handing the word over as a pointer, costs k_hz two VGPRs, and the former 0.4 % of its time:
// profiles/stage_kit_resources.txt.)
__shared__ u64 slot_s_count;
__device__ __forceinline__ void slot_count_begin() { if (threadIdx.x == 0) slot_s_count = 0; }
__device__ __forceinline__ void slot_count(u64 *ctr, u64 wave_total)
{
    if ((threadIdx.x & 63) == 0 && wave_total) atomicAdd(&slot_s_count, wave_total);
    __syncthreads();
    if (threadIdx.x == 0 && slot_s_count) atomicAdd(ctr + (blockIdx.x & (SLOTS - 1)) * SLOT_WORDS, slot_s_count);
}

template <typename Word = u64>      // (a template only so that a unit that does not count carries no copy of the kernel)
__global__ void __launch_bounds__(64) k_slot_total(Word *ctr)
{
    const Word sum = wave_add(ctr[(int)threadIdx.x * SLOT_WORDS]);
    if (threadIdx.x == 0) ctr[SLOT_TOTAL] = sum;
}

// ---- host ----
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    int n = 0;
    ~Events() { for (int i = 0; i < n; i++) (void)hipEventDestroy(e[i]); }
    int create() { for (; n < N; n++) HIP_TRY(hipEventCreate(&e[n])); return 0; }
    int elapsed(int i, int j, double *ms) const
    {
        float f = 0.f;
        HIP_TRY(hipEventElapsedTime(&f, e[i], e[j]));
        *ms = (double)f;
        return 0;
    }
};

// the device time of a call that recorded t->ev[6] where its device work began: records t->ev[7] and waits for it
inline int stage_elapsed(pydem_tile *t, double *ms)
{
    HIP_TRY(hipEventRecord(t->ev[7], t->stream));
    HIP_TRY(hipEventSynchronize(t->ev[7]));
    float el = 0.f;
    HIP_TRY(hipEventElapsedTime(&el, t->ev[6], t->ev[7]));
    if (ms) *ms = (double)el;
    return 0;
}

inline double as_double(u64 b)
{
    double d;
    ::memcpy(&d, &b, 8);
    return d;
}

// fraction bits and exponent of a fixed-point sum: B = min(40, 62 - ceil(log2(max(cells, 2)))), E from frexp of the largest term
// (the host twin is conditioning.fixed_point)
inline void fixed_point(int64_t cells, double largest, int *shift, double *quantum)
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

// workgroups of 256 lanes for `cells` cells, `cap` at most: GRID_LOOP for the kernels that carry a reduction through a
// grid-stride loop, GRID_FULL for the plain per-cell ones
constexpr int GRID_LOOP = 8192, GRID_FULL = 1 << 20;
inline int capped_grid(int64_t cells, int cap) { return (int)(cdiv(cells, 256) < cap ? cdiv(cells, 256) : cap); }

// A PYDEM_* variable: its integer, `dflt` when it is unset or empty.  Nothing is cached here: a switch that is read once per
// process is held in a static of its unit (include/pydem_hip.h says which is which; the tests switch the others mid-process).
inline int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}
inline bool env_switch(const char *name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; }

// `count` lines of the held plane `plane` of T (axis 0: row, 1: column; a negative index counts from the end) into dsts: one
// stream, one wait.  Columns are gathered into scratch of the conditioning arena, everything lands in the tile's pinned staging.
template <typename T>
int seam_get_lines(pydem_tile *t, const char *who, const T *plane, int count, const int *axes, const int64_t *indices, void *const *dsts)
{
    if (count <= 0) return 0;
    const size_t Lmax = (size_t)(t->n > t->m ? t->n : t->m);
    int ncols = 0;
    for (int k = 0; k < count; k++) {
        const int64_t lim = axes[k] == 0 ? t->n : t->m;
        if ((axes[k] != 0 && axes[k] != 1) || indices[k] < -lim || indices[k] >= lim) { pydem_set_error("%s: line index out of range", who); return -2; }
        if (axes[k] == 1) ncols++;
    }
    ArenaLease lease;
    T *stage = nullptr;
    if (ncols) {
        PYDEM_TRY(arena_acquire(t->device, &lease));
        stage = (T *)arena_take(&lease, (size_t)ncols * (size_t)t->n * sizeof(T));
        if (!stage) return -1;
    }
    void *pin_v = nullptr;
    PYDEM_TRY(tile_pinned(t, (size_t)count * Lmax * sizeof(T), &pin_v));
    T *pin = (T *)pin_v;
    int col = 0;
    for (int k = 0; k < count; k++) {
        const int64_t lim = axes[k] == 0 ? t->n : t->m;
        const int64_t index = indices[k] < 0 ? indices[k] + lim : indices[k];
        if (axes[k] == 0) {
            HIP_TRY(hipMemcpyAsync(pin + (size_t)k * Lmax, plane + (size_t)index * t->m, (size_t)t->m * sizeof(T), hipMemcpyDeviceToHost, t->stream));
        } else {
            T *dst = stage + (size_t)col++ * (size_t)t->n;
            hipLaunchKernelGGL(k_line_gather<T>, dim3(capped_grid(t->n, 64)), dim3(256), 0, t->stream, plane + index, t->m, t->n, dst);
            HIP_TRY(hipMemcpyAsync(pin + (size_t)k * Lmax, dst, (size_t)t->n * sizeof(T), hipMemcpyDeviceToHost, t->stream));
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    for (int k = 0; k < count; k++) memcpy(dsts[k], pin + (size_t)k * Lmax, (size_t)(axes[k] == 0 ? t->m : t->n) * sizeof(T));
    return 0;
}

}  // namespace
