// hand_table.hip -- pydem_hand_table: per zone and per water stage, the cells, the flooded area, the area-weighted HAND and the
// wetted bed area of a HAND plane (the "hydraulic property table" of the HAND workflows).  No reference method; the definition of
// every word is in include/pydem_hip.h.
//
// One pass over two planes (zone, HAND; the slope comes from the resident PYDEM_MAG) with integer atomics, as k_dp_stats of
// depressions.hip: a cell's three terms are turned into fixed point (llrint(ldexp(p, shift))) and added to 64-bit words, so the
// sums do not depend on the order of the additions and every schedule gives the same bits.  The host twin
// (pydem_amd/hydraulics.py: hand_table_ref) is compared with array_equal.
//   k_ht_max   the largest term of each of the three sums over the counted cells (the shifts need them) and the largest zone,
//              with atomicMax on the bit patterns of the magnitudes -- non-negative doubles order like their words.
//   k_ht_sum   one lane per cell.  The stages sit in LDS and a binary search gives the bin; the key of a counted cell is
//              (zone - 1) * S + bin, that of a NaN / above-the-top cell K * S + (zone - 1) * 2 + {0, 1}.  A wavefront walks its
//              distinct keys (wave_by_key of stage_kit.h); the lanes of one key reduce with xor shuffles and their first lane
//              issues the atomics -- one set per wavefront inside a large catchment instead of 64.  A lone lane skips the
//              reduction.  PYDEM_HANDTAB_LOCAL=0 (read once per process): no reduction, every lane issues its own atomics.
// The table ([K, S, 4] words, then [K, 2]) and the uploaded planes are leased from the conditioning arena: nothing stays with
// the tile.
#include "stage_kit.h"

namespace {

constexpr int HT_MAX_STAGES = 1024;
// counter block, 64-bit words: bits of max p_a, max |p_m|, max p_b; the largest zone id met (0: none above 0)
enum { HTC_A = 0, HTC_M, HTC_B, HTC_ZONE, HTC_WORDS };

// the three terms of a cell of row area a, HAND h and slope mg (a non-finite slope counts as 0)
__device__ inline void ht_terms(double a, double h, double mg, double &pm, double &pb)
{
    pm = a * h;
    pb = isfinite(mg) ? a * __dsqrt_rn(1.0 + mg * mg) : a;
}

// what a cell is: 0 skipped (zone < 1 or > K), 1 counted, 2 NaN, 3 above the top stage
__device__ inline int ht_class(int z, int64_t K, double h, double top)
{
    if (z < 1 || (int64_t)z > K) return 0;
    if (isnan(h)) return 2;
    return h > top ? 3 : 1;
}

__global__ void __launch_bounds__(256)
k_ht_max(const int32_t *__restrict__ zone, const double *__restrict__ hand, const double *__restrict__ mag, const double *__restrict__ dX2,
         const double *__restrict__ dY2, int64_t K, double top, int64_t NN, int m, u64 *ctr)
{
    u64 ma = 0, mm = 0, mb = 0, mz = 0;
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = c0 + threadIdx.x;
        if (c >= NN) continue;
        const int z = zone[c];
        if (z > 0 && (u64)z > mz) mz = (u64)z;
        const double h = hand[c];
        if (ht_class(z, K, h, top) != 1) continue;
        const int64_t r = c / m;
        const double a = dX2[r] * dY2[r];
        double pm, pb;
        ht_terms(a, h, mag[c], pm, pb);
        const u64 ka = (u64)__double_as_longlong(fabs(a)), km = (u64)__double_as_longlong(fabs(pm)), kb = (u64)__double_as_longlong(fabs(pb));
        ma = ka > ma ? ka : ma;
        mm = km > mm ? km : mm;
        mb = kb > mb ? kb : mb;
    }
    ma = wave_max(ma); mm = wave_max(mm); mb = wave_max(mb); mz = wave_max(mz);
    if ((threadIdx.x & 63) == 0) {
        if (ma) atomicMax(ctr + HTC_A, ma);
        if (mm) atomicMax(ctr + HTC_M, mm);
        if (mb) atomicMax(ctr + HTC_B, mb);
        if (mz) atomicMax(ctr + HTC_ZONE, mz);
    }
}

// tab: [K * S] rows of four words (cells, area, area x HAND, bed area), then [K] rows of two (NaN cells, cells above the top)
__global__ void __launch_bounds__(256)
k_ht_sum(const int32_t *__restrict__ zone, const double *__restrict__ hand, const double *__restrict__ mag, const double *__restrict__ dX2,
         const double *__restrict__ dY2, const double *__restrict__ stages, int S, int64_t K, int64_t NN, int m, int sh_a, int sh_m,
         int sh_b, int local, u64 *tab)
{
    __shared__ double st[HT_MAX_STAGES];
    for (int i = (int)threadIdx.x; i < S; i += (int)blockDim.x) st[i] = stages[i];
    __syncthreads();
    const double top = st[S - 1];
    const int64_t KS = K * (int64_t)S;
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {     // (uniform per wavefront)
        const int64_t c = c0 + threadIdx.x;
        int cls = 0;
        int64_t key = -1;
        u64 ai = 0, mi = 0, bi = 0;
        if (c < NN) {
            const int z = zone[c];
            const double h = hand[c];
            cls = ht_class(z, K, h, top);
            if (cls == 1) {
                int lo = 0, cnt = S;                            // stages below h: the first index with st[i] >= h
                while (cnt > 0) {
                    const int half = cnt >> 1;
                    if (st[lo + half] < h) { lo += half + 1; cnt -= half + 1; } else cnt = half;
                }
                key = (int64_t)(z - 1) * S + lo;                // (h <= top: lo <= S - 1)
                const int64_t r = c / m;
                const double a = dX2[r] * dY2[r];
                double pm, pb;
                ht_terms(a, h, mag[c], pm, pb);
                ai = (u64)__double2ll_rn(ldexp(a, sh_a));
                mi = (u64)__double2ll_rn(ldexp(pm, sh_m));      // signed: two's complement
                bi = (u64)__double2ll_rn(ldexp(pb, sh_b));
            } else if (cls >= 2)
                key = KS + (int64_t)(z - 1) * 2 + (cls - 2);
        }
        const bool act = cls != 0;
        if (!local) {
            if (cls == 1) {
                u64 *row = tab + key * 4;
                atomicAdd(row, 1ull); atomicAdd(row + 1, ai); atomicAdd(row + 2, mi); atomicAdd(row + 3, bi);
            } else if (act)
                atomicAdd(tab + KS * 4 + (key - KS), 1ull);
            continue;
        }
        wave_by_key(act, key, [&](int64_t lkey, int leader, u64 mask, bool mine, bool lone) {
            const u64 cnt = (u64)__popcll(mask);
            if (lkey >= KS) {                                   // a NaN / above word: the count alone (uniform branch)
                if (lane == leader) atomicAdd(tab + KS * 4 + (lkey - KS), cnt);
                return;
            }
            u64 a = ai, v = mi, b = bi;
            if (!lone) {                                        // more than one lane: reduce first (uniform branch)
                a = wave_add(mine ? ai : 0ull);
                v = wave_add(mine ? mi : 0ull);
                b = wave_add(mine ? bi : 0ull);
            }
            if (lane == leader) {
                u64 *row = tab + lkey * 4;
                atomicAdd(row, cnt); atomicAdd(row + 1, a); atomicAdd(row + 2, v); atomicAdd(row + 3, b);
            }
        });
    }
}

bool local_reduction()
{
    static const bool on = env_switch("PYDEM_HANDTAB_LOCAL", true);      // (read once per process)
    return on;
}

}  // namespace

int stage_hand_table(pydem_tile *t, const int32_t *zone, const double *hand, const double *stages, int64_t S, int64_t K, int64_t *table,
                     int64_t *skipped, double *quanta, double *ms)
{
    const char *who = "pydem_hand_table";
    if (!zone || !stages || (K > 0 && (!table || !skipped))) { pydem_set_error("%s: a NULL argument", who); return -2; }
    if (K < 0 || K > (int64_t)INT32_MAX) { pydem_set_error("%s: %lld zones (0 .. 2^31 - 1 allowed)", who, (long long)K); return -2; }
    if (S < 1 || S > HT_MAX_STAGES) { pydem_set_error("%s: %lld stages (1 .. %d allowed)", who, (long long)S, HT_MAX_STAGES); return -2; }
    for (int64_t j = 0; j < S; j++)
        if (!std::isfinite(stages[j]) || (j > 0 && !(stages[j] > stages[j - 1]))) {
            pydem_set_error("%s: the stages must be finite and strictly ascending (stage %lld is %g)", who, (long long)j, stages[j]);
            return -2;
        }
    if (!t->spacing_set) { pydem_set_error("%s: call pydem_tile_set_spacing first", who); return -3; }
    if (!t->mag || !t->have[PYDEM_MAG]) { pydem_set_error("%s: required input field %d is missing", who, (int)PYDEM_MAG); return -3; }
    if (!hand && (!t->dd_down_ready || !t->dd_out)) {
        pydem_set_error("%s: no HAND plane was passed and the tile holds no finished pydem_dist_down result (another sweep, or a "
                        "change of the surface, has followed the last one)", who);
        return -3;
    }
    const int64_t NN = t->NN;
    const int m = (int)t->m;
    const size_t tab_words = (size_t)K * (size_t)S * 4 + (size_t)K * 2;

    Events<4> ev;
    PYDEM_TRY(ev.create());
    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    // everything the call needs, before any kernel runs
    u64 *tab = nullptr;
    if (K > 0) {
        const size_t before = lease.want;
        tab = (u64 *)arena_take(&lease, tab_words * 8);
        if (!tab) {
            lease.want = before;                // (a table that cannot be had does not size the arena of the next lease)
            pydem_set_error("%s: no device memory for the table of %lld zones x %lld stages (%zu bytes); nothing was returned", who,
                            (long long)K, (long long)S, tab_words * 8);
            return -6;
        }
    }
    int32_t *d_zone = (int32_t *)arena_take(&lease, (size_t)NN * 4);
    double *d_hand = hand ? (double *)arena_take(&lease, (size_t)NN * 8) : t->dd_out;
    double *d_stages = (double *)arena_take(&lease, (size_t)S * 8);
    u64 *ctr = (u64 *)arena_take(&lease, HTC_WORDS * 8);
    if (!d_zone || !d_hand || !d_stages || !ctr) return -1;
    PYDEM_TRY(tile_plane_copy(t, d_zone, const_cast<int32_t *>(zone), (size_t)NN * 4, false));
    if (hand) PYDEM_TRY(tile_plane_copy(t, d_hand, const_cast<double *>(hand), (size_t)NN * 8, false));
    PYDEM_TRY(tile_plane_copy(t, d_stages, const_cast<double *>(stages), (size_t)S * 8, false));

    const int gcells = capped_grid(NN, GRID_LOOP);
    HIP_TRY(hipMemsetAsync(ctr, 0, HTC_WORDS * 8, t->stream));
    HIP_TRY(hipEventRecord(ev.e[0], t->stream));
    hipLaunchKernelGGL(k_ht_max, dim3(gcells), dim3(256), 0, t->stream, (const int32_t *)d_zone, (const double *)d_hand, (const double *)t->mag,
                       (const double *)t->dX2, (const double *)t->dY2, K, stages[S - 1], NN, m, ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], t->stream));
    volatile u64 *h = (volatile u64 *)t->h_counters;
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr, HTC_WORDS * 8, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    if ((int64_t)h[HTC_ZONE] > K) {
        pydem_set_error("%s: the zone plane holds the id %lld, above the %lld zones of the call", who, (long long)h[HTC_ZONE], (long long)K);
        return -2;
    }
    const double largest[3] = {as_double(h[HTC_A]), as_double(h[HTC_M]), as_double(h[HTC_B])};
    int sh[3];
    double q[3];
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(largest[k])) {
            pydem_set_error("%s: a term of the sums is not finite (-inf in the HAND plane, a slope or a spacing out of range)", who);
            return -2;
        }
        fixed_point(NN, largest[k], &sh[k], &q[k]);
    }
    HIP_TRY(hipEventRecord(ev.e[2], t->stream));
    if (K > 0) {
        HIP_TRY(hipMemsetAsync(tab, 0, tab_words * 8, t->stream));
        hipLaunchKernelGGL(k_ht_sum, dim3(gcells), dim3(256), 0, t->stream, (const int32_t *)d_zone, (const double *)d_hand, (const double *)t->mag,
                           (const double *)t->dX2, (const double *)t->dY2, (const double *)d_stages, (int)S, K, NN, m, sh[0], sh[1], sh[2],
                           local_reduction() ? 1 : 0, tab);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev.e[3], t->stream));
    HIP_TRY(hipEventSynchronize(ev.e[3]));
    if (K > 0) {
        PYDEM_TRY(tile_plane_copy(t, tab, table, (size_t)K * (size_t)S * 4 * 8, true));
        PYDEM_TRY(tile_plane_copy(t, tab + (size_t)K * (size_t)S * 4, skipped, (size_t)K * 2 * 8, true));
    }
    if (quanta) for (int k = 0; k < 3; k++) quanta[k] = q[k];
    if (ms) {
        PYDEM_TRY(ev.elapsed(0, 1, &ms[1]));
        PYDEM_TRY(ev.elapsed(2, 3, &ms[2]));
        ms[0] = ms[1] + ms[2];
    }
    return 0;
}
