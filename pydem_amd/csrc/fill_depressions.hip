// fill_depressions.hip -- pydem_fill_depressions: depression filling (PitRemove / Planchon-Darboux / priority-flood + eps) on the
// resident elevation.  No reference method.
//
// The filled surface W is the GREATEST solution of
//     W[c] = z[c]                                                  on open cells (border, beside no-data, caller's outlets)
//     W[c] = max(z[c], min over the finite 8-neighbours v of (W[v] + eps))     elsewhere
// (include/pydem_hip.h).  The right-hand side is monotone in W -- also in floating point: x <= y gives fl(x + eps) <= fl(y + eps)
// -- so relaxing downward from W0 (+inf on the closed cells) in ANY order keeps every value at or above the greatest solution
// and never raises one; what the relaxation stops at is a solution, hence that one, bit for bit.  For the same reason the
// minimum of the eight sums is the sum of the minimum and eps: one add per cell update instead of eight.  A sum is never
// -0.0, and max keeps z unless the sum is strictly greater, so signed zeros have one outcome too.
//
// Schedule: 32 x 32 blocks, one workgroup each.  A visit loads the block's W with a one-cell halo into LDS, iterates there to
// the block's fixed point for that halo and writes the cells that fell back.  The blocks of one launch share a colour,
// (block_row & 1) * 2 + (block_col & 1): their halos lie in blocks of the three other colours, so no workgroup of a launch
// reads a word that another one of the same launch writes.  A block is visited only while its flag word is set: every flag is
// set at the start, a visit clears its own, and a block whose rim cells fell sets the flags of the neighbours that read that
// rim (plain stores of 1, read by later launches only).  A pass is the four launches; a block that changed anything stores
// the pass number into one counter word, which the host reads through the pinned mirror every few passes.
//
// LDS: 34 x 34 doubles, row pitch 34 (9248 bytes).  Lane l of a wavefront reads column (l & 31) + dx of row 4 * (l >> 5) + dy:
// the 32 lanes that ds_read_b64 serves together read 32 consecutive doubles, 256 contiguous bytes, all 64 banks once -- at
// any pitch, so the tile is not padded.  9.2 KB and 256 threads per workgroup: the LDS admits 17 workgroups per CU, the wave
// slots fewer: 70 VGPRs give 7 wavefronts per SIMD, so registers bound the occupancy, not LDS (profiles/fill_depressions_cost.txt).
//
// The seam session (pydem_fill_seam_*, at the end of this file) is the same relaxation on a W that stays with the tile between
// calls, for the fill ACROSS tiles: border cells that other tiles hold too are not open by position but capped by the other
// tiles' values, W = max(z, min(cap, min (W[v] + eps))).  Still monotone, in W and in the caps, so W at a fixed point is a valid
// start when caps fall.  Its visit is a second instantiation of the same body (SEAM): the lane's four caps in registers, one fmin
// more per update, 82 VGPRs and 5 wavefronts per SIMD (profiles/fill_mosaic_cost.txt); the plain one compiles the cap out.
#include "stage_kit.h"

namespace {

constexpr int FD_B = 32;            // block edge
constexpr int FD_P = FD_B + 2;      // LDS tile edge and row pitch (one-cell halo)
constexpr int FD_T = 256;           // lanes per workgroup: 32 columns x 8 groups of 4 rows
constexpr int FD_R = FD_B * FD_B / FD_T;    // rows per lane (4)

// counter block, 64-bit words
enum { FD_AMAX = 0,     // bits of max |z| over the finite cells (non-negative doubles order like their bit patterns)
       FD_INF = 1,      // != 0: z holds +-inf
       FD_STAMP = 2,    // number of the last pass in which a block changed
       FD_RAISED = 3,   // cells with W > z
       FD_DEPTH = 4,    // bits of max (W - z)
       FD_LOWERED = 5,  // seam session: cells whose W is lower than the snapshot of the call's start
       FD_LEFT = 6,     // seam session: cells of W that are still +inf
       FD_WORDS = 8 };

// W0 = z on open cells, +inf on the other finite cells, NaN kept; max |z| and the +-inf test into the counter block
// SEAM (the session): a border cell marked in `seam` (top m, bottom m, left n, right n bytes) is not open by position
template <bool SEAM>
__global__ void __launch_bounds__(256)
k_fd_init(const double *__restrict__ z, const uint8_t *__restrict__ outlets, double *__restrict__ W, int n, int m,
          unsigned long long *ctr, const uint8_t *__restrict__ seam)
{
    const int64_t NN = (int64_t)n * m;
    double amax = 0.0;
    int inf = 0;
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = c0 + threadIdx.x;
        if (c >= NN) continue;
        const double v = z[c];
        if (isnan(v)) { W[c] = v; continue; }
        if (isinf(v)) inf = 1;
        else if (fabs(v) > amax) amax = fabs(v);
        const int r = (int)(c / m), q = (int)(c - (int64_t)r * m);
        bool border = r == 0 || r == n - 1 || q == 0 || q == m - 1;
        if (SEAM && border &&
            ((r == 0 && seam[q]) || (r == n - 1 && seam[m + q]) || (q == 0 && seam[2 * m + r]) || (q == m - 1 && seam[2 * m + n + r])))
            border = false;
        bool open = border || (outlets && outlets[c] != 0);
        if (!open) {
#pragma unroll
            for (int dr = -1; dr <= 1; dr++)
#pragma unroll
                for (int dq = -1; dq <= 1; dq++) {
                    if ((dr | dq) == 0) continue;
                    if (SEAM && (r + dr < 0 || r + dr >= n || q + dq < 0 || q + dq >= m)) continue;     // (a seam cell lies on the border)
                    if (isnan(z[c + (int64_t)dr * m + dq])) open = true;
                }
        }
        W[c] = open ? v : (double)INFINITY;
    }
    amax = wave_max(amax);
    const unsigned long long any_inf = __ballot(inf != 0);
    if ((threadIdx.x & 63) == 0) {
        if (amax > 0.0) atomicMax(ctr + FD_AMAX, (unsigned long long)__double_as_longlong(amax));
        if (any_inf) ctr[FD_INF] = 1ull;
    }
}

// One visit of the blocks of one colour.  LOCAL: iterate in LDS to the block's fixed point for the halo it loaded; otherwise one
// relaxation step (PYDEM_FILL_LOCAL=0: the result must not depend on the schedule).
// SEAM (the session): a lane whose cell lies on a border line holds that line's cap in a register (+inf otherwise; caps: top m,
// bottom m, left n, right n doubles, never NaN), and the candidate is max(z, min(cap, lo + eps)): one fmin more per update.
template <bool LOCAL, bool SEAM>
__device__ __forceinline__ void
fd_relax_visit(const double *__restrict__ z, double *__restrict__ W, int32_t *__restrict__ flags, int n, int m, int nbr, int nbc,
               int colour, double eps, unsigned long long stamp, unsigned long long *ctr, const double *__restrict__ caps)
{
    __shared__ double s[FD_P * FD_P];
    __shared__ unsigned s_rim;
    const int bc = 2 * (int)blockIdx.x + (colour & 1), br = 2 * (int)blockIdx.y + (colour >> 1);
    if (br >= nbr || bc >= nbc) return;
    const int b = br * nbc + bc;
    if (flags[b] == 0) return;          // (nothing writes this word during the launch: the visit stores it at its end)
    const int tid = (int)threadIdx.x, tx = tid & (FD_B - 1), ty = tid >> 5;
    const int r0 = br * FD_B, c0 = bc * FD_B;
    if (tid == 0) s_rim = 0u;
    for (int i = tid; i < FD_P * FD_P; i += FD_T) {
        const int lr = i / FD_P, lc = i - lr * FD_P;
        const int gr = r0 - 1 + lr, gc = c0 - 1 + lc;
        double v = (double)INFINITY;                // outside the tile and no-data: never the minimum
        if (gr >= 0 && gr < n && gc >= 0 && gc < m) { v = W[(int64_t)gr * m + gc]; if (isnan(v)) v = (double)INFINITY; }
        s[i] = v;
    }
    // the lane's cells: column tx, rows 4 ty .. 4 ty + 3 of the block; their z stays in registers (+inf where there is no
    // cell to relax: such a cell can never fall)
    double zz[FD_R], w0[FD_R];
    const int gc = c0 + tx;
#pragma unroll
    for (int k = 0; k < FD_R; k++) {
        const int gr = r0 + ty * FD_R + k;
        double v = (double)INFINITY;
        if (gr < n && gc < m) { v = z[(int64_t)gr * m + gc]; if (isnan(v)) v = (double)INFINITY; }
        zz[k] = v;
    }
    double cp[FD_R];
    if (SEAM) {
#pragma unroll
        for (int k = 0; k < FD_R; k++) {
            const int gr = r0 + ty * FD_R + k;
            double v = (double)INFINITY;
            if (gr < n && gc < m) {
                if (gr == 0) v = fmin(v, caps[gc]);
                if (gr == n - 1) v = fmin(v, caps[m + gc]);
                if (gc == 0) v = fmin(v, caps[2 * m + gr]);
                if (gc == m - 1) v = fmin(v, caps[2 * m + n + gr]);
            }
            cp[k] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FD_R; k++) w0[k] = s[(ty * FD_R + k + 1) * FD_P + tx + 1];
    int ever = 0;
    for (;;) {
        double a[FD_R + 2][3];
#pragma unroll
        for (int j = 0; j < FD_R + 2; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) a[j][i] = s[(ty * FD_R + j) * FD_P + tx + i];
        bool changed = false;
        // down the lane's four rows, then up again: a value that falls is seen by the lane's next cell at once
#pragma unroll
        for (int kk = 0; kk < 2 * FD_R - 1; kk++) {
            const int k = kk < FD_R ? kk : 2 * FD_R - 2 - kk;
            double lo = fmin(fmin(a[k][0], a[k][1]), a[k][2]);
            lo = fmin(lo, fmin(a[k + 1][0], a[k + 1][2]));
            lo = fmin(lo, fmin(fmin(a[k + 2][0], a[k + 2][1]), a[k + 2][2]));
            double sum = lo + eps;
            if (SEAM) sum = fmin(sum, cp[k]);
            const double cand = sum > zz[k] ? sum : zz[k];
            if (cand < a[k + 1][1]) { a[k + 1][1] = cand; changed = true; }
        }
        __syncthreads();                            // every lane has read its window
        if (changed) {
#pragma unroll
            for (int k = 0; k < FD_R; k++) s[(ty * FD_R + k + 1) * FD_P + tx + 1] = a[k + 1][1];
        }
        const int any = __syncthreads_or(changed ? 1 : 0);
        ever |= any;
        if (!LOCAL || !any) break;
    }
    if (!ever) {
        if (tid == 0) flags[b] = 0;
        return;
    }
    // write back what fell; which rims did
    unsigned rim = 0u;
#pragma unroll
    for (int k = 0; k < FD_R; k++) {
        const int lr = ty * FD_R + k, gr = r0 + lr;
        const double v = s[(lr + 1) * FD_P + tx + 1];
        if (v < w0[k]) {                            // (only cells of the tile can fall)
            W[(int64_t)gr * m + gc] = v;
            if (lr == 0) rim |= 1u | (tx == 0 ? 16u : 0u) | (tx == FD_B - 1 ? 32u : 0u);
            if (lr == FD_B - 1) rim |= 2u | (tx == 0 ? 64u : 0u) | (tx == FD_B - 1 ? 128u : 0u);
            if (tx == 0) rim |= 4u;
            if (tx == FD_B - 1) rim |= 8u;
        }
    }
    if (rim) atomicOr(&s_rim, rim);
    __syncthreads();
    if (tid < 8) {
        // bit: 0 N, 1 S, 2 W, 3 E, 4 NW, 5 NE, 6 SW, 7 SE
        const int dr = (tid == 0 || tid == 4 || tid == 5) ? -1 : ((tid == 1 || tid == 6 || tid == 7) ? 1 : 0);
        const int dq = (tid == 2 || tid == 4 || tid == 6) ? -1 : ((tid == 3 || tid == 5 || tid == 7) ? 1 : 0);
        const int rr = br + dr, qq = bc + dq;
        if (((s_rim >> tid) & 1u) && rr >= 0 && rr < nbr && qq >= 0 && qq < nbc) flags[rr * nbc + qq] = 1;
    } else if (tid == 64) {
        flags[b] = LOCAL ? 0 : 1;                   // one step is not the fixed point: the block comes back
        ctr[FD_STAMP] = stamp;
    }
}

template <bool LOCAL>
__global__ void __launch_bounds__(FD_T)
k_fd_relax(const double *__restrict__ z, double *__restrict__ W, int32_t *__restrict__ flags, int n, int m, int nbr, int nbc,
           int colour, double eps, unsigned long long stamp, unsigned long long *ctr)
{
    fd_relax_visit<LOCAL, false>(z, W, flags, n, m, nbr, nbc, colour, eps, stamp, ctr, nullptr);
}

template <bool LOCAL>
__global__ void __launch_bounds__(FD_T)
k_fd_relax_seam(const double *__restrict__ z, double *__restrict__ W, int32_t *__restrict__ flags, int n, int m, int nbr, int nbc,
                int colour, double eps, unsigned long long stamp, unsigned long long *ctr, const double *__restrict__ caps)
{
    fd_relax_visit<LOCAL, true>(z, W, flags, n, m, nbr, nbc, colour, eps, stamp, ctr, caps);
}

// the session's caps: an incoming entry below the held one replaces it and flags the rim block of its cell
__global__ void __launch_bounds__(256)
k_fs_caps(double *__restrict__ caps, const double *__restrict__ incoming, int32_t *__restrict__ flags, int n, int m, int nbr, int nbc)
{
    const int L = 2 * m + 2 * n;
    for (int e = (int)(blockIdx.x * blockDim.x + threadIdx.x); e < L; e += (int)(gridDim.x * blockDim.x)) {
        const double v = incoming[e];
        if (!(v < caps[e])) continue;
        caps[e] = v;
        int br, bc;
        if (e < m) { br = 0; bc = e / FD_B; }
        else if (e < 2 * m) { br = nbr - 1; bc = (e - m) / FD_B; }
        else if (e < 2 * m + n) { br = (e - 2 * m) / FD_B; bc = 0; }
        else { br = (e - 2 * m - n) / FD_B; bc = nbc - 1; }
        flags[br * nbc + bc] = 1;
    }
}

// cells of W below `before` (null: cells of W that are +inf) into ctr[word]
__global__ void __launch_bounds__(256)
k_fs_count(const double *__restrict__ W, const double *__restrict__ before, int64_t NN, unsigned long long *ctr, int word)
{
    unsigned long long cnt = 0;
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {     // (uniform per wavefront)
        const int64_t c = c0 + threadIdx.x;
        bool hit = false;
        if (c < NN) hit = before ? W[c] < before[c] : W[c] == (double)INFINITY;
        cnt += (unsigned long long)__popcll(__ballot(hit));
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(ctr + word, cnt);
}

// depth = W - z (into the W plane), raised cells, maximum depth, elev = W
__global__ void __launch_bounds__(256)
k_fd_final(double *__restrict__ z, double *__restrict__ W, int64_t NN, unsigned long long *ctr)
{
    double dmax = 0.0;
    unsigned long long cnt = 0;
    for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x; c0 < NN; c0 += (int64_t)gridDim.x * blockDim.x) {     // (uniform per wavefront)
        const int64_t c = c0 + threadIdx.x;
        bool up = false;
        if (c < NN) {
            const double w = W[c], v = z[c];
            const double d = w - v;
            W[c] = d;
            up = w > v;
            if (up) { z[c] = w; if (d > dmax) dmax = d; }
        }
        cnt += (unsigned long long)__popcll(__ballot(up));
    }
    dmax = wave_max(dmax);
    if ((threadIdx.x & 63) == 0) {
        if (cnt) atomicAdd(ctr + FD_RAISED, cnt);
        if (dmax > 0.0) atomicMax(ctr + FD_DEPTH, (unsigned long long)__double_as_longlong(dmax));
    }
}

// read per call: the tests switch them
struct FillEnv { int max_passes = 0, every = 0; bool local = true; };
int fill_env(const char *who, FillEnv *e)
{
    e->max_passes = env_int("PYDEM_FILL_MAX_PASSES", 100000);
    if (e->max_passes < 1) { pydem_set_error("%s: PYDEM_FILL_MAX_PASSES must be >= 1", who); return -2; }
    e->local = env_switch("PYDEM_FILL_LOCAL", true);
    e->every = env_int("PYDEM_FILL_CHECK_EVERY", 4);         // passes between two looks at the counter (the result does not depend on it)
    if (e->every < 1) e->every = 1;
    return 0;
}

int fill_look(pydem_tile *t, unsigned long long *ctr)
{
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr, FD_WORDS * 8, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

// the pass loop: bounded by max_passes.  caps: the cap lines of a seam session (null: the plain fill).  *passes: the passes that
// changed something and the one that found nothing to do.  -5 at the bound.
int fill_passes(pydem_tile *t, const FillEnv &env, double *W, int32_t *flags, unsigned long long *ctr, const double *caps, double eps,
                int64_t *run_out, int64_t *passes)
{
    const int n = (int)t->n, m = (int)t->m;
    const int nbr = (int)cdiv(n, FD_B), nbc = (int)cdiv(m, FD_B);
    volatile unsigned long long *h = (volatile unsigned long long *)t->h_counters;     // (64 int32: room for the block)
    const double *z = (const double *)t->elev;
    int64_t run = 0, stamp = 0;
    bool converged = false;
    while (run < env.max_passes) {
        const int64_t stop = run + env.every < env.max_passes ? run + env.every : env.max_passes;
        for (; run < stop; run++) {
            for (int colour = 0; colour < 4; colour++) {
                const int gx = (int)cdiv(nbc - (colour & 1), 2), gy = (int)cdiv(nbr - (colour >> 1), 2);
                if (gx < 1 || gy < 1) continue;
                const dim3 grid(gx, gy), block(FD_T);
                const unsigned long long st = (unsigned long long)(run + 1);
                if (caps) {
                    if (env.local)
                        hipLaunchKernelGGL(k_fd_relax_seam<true>, grid, block, 0, t->stream, z, W, flags, n, m, nbr, nbc, colour, eps, st, ctr, caps);
                    else
                        hipLaunchKernelGGL(k_fd_relax_seam<false>, grid, block, 0, t->stream, z, W, flags, n, m, nbr, nbc, colour, eps, st, ctr, caps);
                } else if (env.local)
                    hipLaunchKernelGGL(k_fd_relax<true>, grid, block, 0, t->stream, z, W, flags, n, m, nbr, nbc, colour, eps, st, ctr);
                else
                    hipLaunchKernelGGL(k_fd_relax<false>, grid, block, 0, t->stream, z, W, flags, n, m, nbr, nbc, colour, eps, st, ctr);
            }
        }
        HIP_TRY(hipGetLastError());
        PYDEM_TRY(fill_look(t, ctr));
        stamp = (int64_t)h[FD_STAMP];
        if (stamp < run) { converged = true; break; }       // the last pass enqueued changed nothing
    }
    *run_out = run;
    *passes = stamp + 1;
    return converged ? 0 : -5;
}

}  // namespace

// The first part of the fill, shared with pydem_depressions (depressions.hip): W relaxed to its fixed point in scratch of the
// caller's lease; the elevation is not touched.  `who` names the entry point in the messages; ev_start (may be null) is recorded
// where the device work begins.
int fill_relax(pydem_tile *t, ArenaLease *lease, const char *who, double *epsilon, const uint8_t *outlets, hipEvent_t ev_start, FillRelax *out)
{
    const double eps_in = *epsilon;
    if (!std::isfinite(eps_in)) { pydem_set_error("%s: epsilon must be finite (got %g)", who, eps_in); return -2; }
    FillEnv env;
    PYDEM_TRY(fill_env(who, &env));
    const int n = (int)t->n, m = (int)t->m;
    const int nbr = (int)cdiv(n, FD_B), nbc = (int)cdiv(m, FD_B);
    const int64_t nb = (int64_t)nbr * nbc;

    double *W = (double *)arena_take(lease, (size_t)t->NN * 8);
    int32_t *flags = (int32_t *)arena_take(lease, (size_t)nb * 4);
    unsigned long long *ctr = (unsigned long long *)arena_take(lease, FD_WORDS * 8);
    uint8_t *d_out = outlets ? (uint8_t *)arena_take(lease, (size_t)t->NN) : nullptr;
    if (!W || !flags || !ctr || (outlets && !d_out)) return -1;
    if (outlets) PYDEM_TRY(tile_plane_copy(t, d_out, const_cast<uint8_t *>(outlets), (size_t)t->NN, false));

    volatile unsigned long long *h = (volatile unsigned long long *)t->h_counters;     // (64 int32: room for the block)
    auto look = [&]() -> int { return fill_look(t, ctr); };
    const int gcells = capped_grid(t->NN, GRID_LOOP);

    if (ev_start) HIP_TRY(hipEventRecord(ev_start, t->stream));
    HIP_TRY(hipMemsetAsync(ctr, 0, FD_WORDS * 8, t->stream));
    hipLaunchKernelGGL(k_fd_init<false>, dim3(gcells), dim3(256), 0, t->stream, (const double *)t->elev, (const uint8_t *)d_out, W, n, m, ctr,
                       (const uint8_t *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)flags, 1, (size_t)nb, t->stream));
    PYDEM_TRY(look());
    if (h[FD_INF]) { pydem_set_error("%s: the elevation holds +-inf", who); return -2; }
    const double amax = as_double(h[FD_AMAX]);
    double eps = eps_in;
    if (eps < 0) {
        // automatic: 2^-32 of the smallest power of two >= max |z|
        int e = 1;
        if (amax > 0) { const double f = frexp(amax, &e); if (f == 0.5) e -= 1; } else e = 0;
        eps = ldexp(1.0, e - 32);
        if (!(eps > 0) || !std::isfinite(eps)) { pydem_set_error("%s: no automatic epsilon for max |z| = %g", who, amax); return -2; }
    }
    if (eps > 0 && amax + eps == amax) {
        pydem_set_error("%s: epsilon %g is not representable at the surface's magnitude (max |z| = %g)", who, eps, amax);
        return -2;
    }

    int64_t run = 0, passes = 0;
    const int rc = fill_passes(t, env, W, flags, ctr, nullptr, eps, &run, &passes);
    if (rc == -5) {
        pydem_set_error("%s: not converged after %lld passes (PYDEM_FILL_MAX_PASSES); the elevation is unchanged", who, (long long)run);
        return -5;
    }
    PYDEM_TRY(rc);
    *epsilon = eps;
    out->W = W; out->ctr = ctr; out->outlets = d_out; out->passes = passes;
    return 0;
}

// pydem_fill_depressions: the relaxation, then depth, counts and elev = W
int stage_fill_depressions(pydem_tile *t, double *epsilon, const uint8_t *outlets, double *depth, int64_t *n_raised, double *max_depth,
                           int64_t *passes, double *ms)
{
    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    FillRelax fr;
    PYDEM_TRY(fill_relax(t, &lease, "pydem_fill_depressions", epsilon, outlets, t->ev[6], &fr));
    double *W = fr.W;
    unsigned long long *ctr = fr.ctr;
    volatile unsigned long long *h = (volatile unsigned long long *)t->h_counters;
    const double eps = *epsilon;
    const int gcells = capped_grid(t->NN, GRID_LOOP);
    hipLaunchKernelGGL(k_fd_final, dim3(gcells), dim3(256), 0, t->stream, t->elev, W, t->NN, ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr, FD_WORDS * 8, hipMemcpyDeviceToHost, t->stream));
    PYDEM_TRY(stage_elapsed(t, ms));
    if (passes) *passes = fr.passes;
    if (n_raised) *n_raised = (int64_t)h[FD_RAISED];
    if (max_depth) *max_depth = as_double(h[FD_DEPTH]);
    if (eps > 0) { t->elev_f32 = false; t->elev_dtype = PYDEM_F64; }      // (eps == 0: every value of W is a value of z)
    if (depth) PYDEM_TRY(tile_plane_copy(t, W, depth, (size_t)t->NN * 8, true));
    return 0;
}

// ---- the seam session: pydem_fill_seam_begin / _relax / _get_lines / _end (include/pydem_hip.h) ----
// W, the block flags and the cap lines stay with the tile between the calls (tile_hold: pydem_tile_device_bytes counts them); what
// a single call needs besides -- the outlets mask and the seam bytes of the init, the incoming caps and the snapshot of W that
// *n_lowered is counted against, the staging of gathered columns -- comes from the conditioning arena for that call.  The
// counter block is the tile's own (t->counters: 64 int32, zeroed by every call that reads it).
static void fill_seam_drop(pydem_tile *t)
{
    (void)hipStreamSynchronize(t->stream);      // (the planes go to the next tile: nothing may still write them)
    tile_drop(t, (void **)&t->fs_W);
    tile_drop(t, (void **)&t->fs_flags);
    tile_drop(t, (void **)&t->fs_caps);
    tile_drop(t, (void **)&t->fs_ids);          // (the id plane of pydem_fill_seam_label, where one is held)
    t->fs_K = -1;
    t->fs_roots.clear();
    t->fs_levels.clear();
    t->fs_caps_h.clear();
    t->fs_open = false;
}

int stage_fill_seam_begin(pydem_tile *t, const uint8_t *outlets, const uint8_t *const seam[4], double *amax_out)
{
    const char *who = "pydem_fill_seam_begin";
    if (t->fs_open) { pydem_set_error("%s: a session is open on this tile (pydem_fill_seam_end first)", who); return -2; }
    const int n = (int)t->n, m = (int)t->m;
    const int nbr = (int)cdiv(n, FD_B), nbc = (int)cdiv(m, FD_B);
    const int64_t nb = (int64_t)nbr * nbc;
    const size_t L = 2 * (size_t)m + 2 * (size_t)n;
    int rc = tile_hold(t, (void **)&t->fs_W, (size_t)t->NN * 8, true);
    if (rc == 0) rc = tile_hold(t, (void **)&t->fs_flags, (size_t)nb * 4, true);
    if (rc == 0) rc = tile_hold(t, (void **)&t->fs_caps, L * 8, true);
    if (rc != 0) { fill_seam_drop(t); return rc; }
    auto run = [&]() -> int {
        ArenaLease lease;
        PYDEM_TRY(arena_acquire(t->device, &lease));
        uint8_t *d_out = outlets ? (uint8_t *)arena_take(&lease, (size_t)t->NN) : nullptr;
        uint8_t *d_seam = (uint8_t *)arena_take(&lease, L);
        if (!d_seam || (outlets && !d_out)) return -1;
        if (outlets) PYDEM_TRY(tile_plane_copy(t, d_out, const_cast<uint8_t *>(outlets), (size_t)t->NN, false));
        // pinned staging: the cap lines (+inf), then the seam bytes
        void *pin = nullptr;
        PYDEM_TRY(tile_pinned(t, L * 8 + L, &pin));
        double *pc = (double *)pin;
        uint8_t *ps = (uint8_t *)pin + L * 8;
        for (size_t e = 0; e < L; e++) pc[e] = (double)INFINITY;
        const size_t off[4] = {0, (size_t)m, 2 * (size_t)m, 2 * (size_t)m + (size_t)n}, len[4] = {(size_t)m, (size_t)m, (size_t)n, (size_t)n};
        for (int k = 0; k < 4; k++) {
            if (seam[k]) for (size_t e = 0; e < len[k]; e++) ps[off[k] + e] = seam[k][e] != 0;
            else memset(ps + off[k], 0, len[k]);
        }
        unsigned long long *ctr = (unsigned long long *)t->counters;
        volatile unsigned long long *h = (volatile unsigned long long *)t->h_counters;
        const int gcells = capped_grid(t->NN, GRID_LOOP);
        HIP_TRY(hipMemcpyAsync(t->fs_caps, pc, L * 8, hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipMemcpyAsync(d_seam, ps, L, hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipMemsetAsync(ctr, 0, FD_WORDS * 8, t->stream));
        hipLaunchKernelGGL(k_fd_init<true>, dim3(gcells), dim3(256), 0, t->stream, (const double *)t->elev, (const uint8_t *)d_out, t->fs_W, n, m,
                           ctr, (const uint8_t *)d_seam);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)t->fs_flags, 1, (size_t)nb, t->stream));
        PYDEM_TRY(fill_look(t, ctr));
        if (h[FD_INF]) { pydem_set_error("%s: the elevation holds +-inf", who); return -2; }
        t->fs_amax = as_double(h[FD_AMAX]);
        return 0;
    };
    rc = run();
    if (rc != 0) { fill_seam_drop(t); return rc; }
    t->fs_caps_h.assign(L, (double)INFINITY);
    t->fs_eps = -1.0;
    t->fs_open = true;
    if (amax_out) *amax_out = t->fs_amax;
    return 0;
}

int stage_fill_seam_relax(pydem_tile *t, double eps, const double *const caps[4], int64_t *n_lowered, int64_t *passes_out, double *ms)
{
    const char *who = "pydem_fill_seam_relax";
    if (!t->fs_open) { pydem_set_error("%s: no session is open on this tile (pydem_fill_seam_begin first)", who); return -2; }
    if (!std::isfinite(eps) || eps < 0) { pydem_set_error("%s: epsilon must be finite and >= 0 (got %g)", who, eps); return -2; }
    if (t->fs_eps >= 0 && eps != t->fs_eps) { pydem_set_error("%s: epsilon %g, the session began with %g", who, eps, t->fs_eps); return -2; }
    if (eps > 0 && t->fs_amax + eps == t->fs_amax) {
        pydem_set_error("%s: epsilon %g is not representable at the surface's magnitude (max |z| = %g)", who, eps, t->fs_amax);
        return -2;
    }
    FillEnv env;
    PYDEM_TRY(fill_env(who, &env));
    const int n = (int)t->n, m = (int)t->m;
    const int nbr = (int)cdiv(n, FD_B), nbc = (int)cdiv(m, FD_B);
    const size_t L = 2 * (size_t)m + 2 * (size_t)n;
    const size_t off[4] = {0, (size_t)m, 2 * (size_t)m, 2 * (size_t)m + (size_t)n}, len[4] = {(size_t)m, (size_t)m, (size_t)n, (size_t)n};
    // caps may only fall (NaN counts as +inf): checked before anything changes
    for (int k = 0; k < 4; k++) {
        if (!caps[k]) continue;
        for (size_t e = 0; e < len[k]; e++) {
            const double v = std::isnan(caps[k][e]) ? (double)INFINITY : caps[k][e];
            if (v > t->fs_caps_h[off[k] + e]) {
                pydem_set_error("%s: cap line %d, entry %zu: %g is above the cap the session holds (%g); caps may only fall", who, k, e, v,
                                t->fs_caps_h[off[k] + e]);
                return -2;
            }
        }
    }
    ArenaLease lease;
    PYDEM_TRY(arena_acquire(t->device, &lease));
    double *incoming = (double *)arena_take(&lease, L * 8);
    double *before = (double *)arena_take(&lease, (size_t)t->NN * 8);
    if (!incoming || !before) return -1;
    void *pin = nullptr;
    PYDEM_TRY(tile_pinned(t, L * 8, &pin));
    double *pc = (double *)pin;
    memcpy(pc, t->fs_caps_h.data(), L * 8);
    for (int k = 0; k < 4; k++) {
        if (!caps[k]) continue;
        for (size_t e = 0; e < len[k]; e++) pc[off[k] + e] = std::isnan(caps[k][e]) ? (double)INFINITY : caps[k][e];
    }
    unsigned long long *ctr = (unsigned long long *)t->counters;
    volatile unsigned long long *h = (volatile unsigned long long *)t->h_counters;
    const int gcells = capped_grid(t->NN, GRID_LOOP);
    const int gcaps = capped_grid((int64_t)L, 64);
    HIP_TRY(hipEventRecord(t->ev[6], t->stream));
    HIP_TRY(hipMemsetAsync(ctr, 0, FD_WORDS * 8, t->stream));
    HIP_TRY(hipMemcpyAsync(incoming, pc, L * 8, hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(before, t->fs_W, (size_t)t->NN * 8, hipMemcpyDeviceToDevice, t->stream));
    hipLaunchKernelGGL(k_fs_caps, dim3(gcaps), dim3(256), 0, t->stream, t->fs_caps, (const double *)incoming, t->fs_flags, n, m, nbr, nbc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));       // (the pinned staging is the tile's: the next call may rewrite it)
    memcpy(t->fs_caps_h.data(), pc, L * 8);
    t->fs_eps = eps;
    int64_t run = 0, passes = 0;
    const int rc = fill_passes(t, env, t->fs_W, t->fs_flags, ctr, t->fs_caps, eps, &run, &passes);
    if (rc == -5) {
        pydem_set_error("%s: not converged after %lld passes (PYDEM_FILL_MAX_PASSES); the session stays open, the elevation is unchanged", who,
                        (long long)run);
        return -5;
    }
    PYDEM_TRY(rc);
    hipLaunchKernelGGL(k_fs_count, dim3(gcells), dim3(256), 0, t->stream, (const double *)t->fs_W, (const double *)before, t->NN, ctr, (int)FD_LOWERED);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr, FD_WORDS * 8, hipMemcpyDeviceToHost, t->stream));
    PYDEM_TRY(stage_elapsed(t, ms));
    if (passes_out) *passes_out = passes;
    if (n_lowered) *n_lowered = (int64_t)h[FD_LOWERED];
    return 0;
}

int stage_fill_seam_get_lines(pydem_tile *t, int count, const int *axes, const int64_t *indices, void *const *dsts)
{
    const char *who = "pydem_fill_seam_get_lines";
    if (!t->fs_open) { pydem_set_error("%s: no session is open on this tile", who); return -2; }
    return seam_get_lines(t, who, (const double *)t->fs_W, count, axes, indices, dsts);
}

int stage_fill_seam_end(pydem_tile *t, int commit, double *depth, int64_t *n_raised, double *max_depth)
{
    const char *who = "pydem_fill_seam_end";
    if (!t->fs_open) { pydem_set_error("%s: no session is open on this tile", who); return -2; }
    if (!commit) { fill_seam_drop(t); return 0; }
    unsigned long long *ctr = (unsigned long long *)t->counters;
    volatile unsigned long long *h = (volatile unsigned long long *)t->h_counters;
    const int gcells = capped_grid(t->NN, GRID_LOOP);
    HIP_TRY(hipMemsetAsync(ctr, 0, FD_WORDS * 8, t->stream));
    hipLaunchKernelGGL(k_fs_count, dim3(gcells), dim3(256), 0, t->stream, (const double *)t->fs_W, (const double *)nullptr, t->NN, ctr, (int)FD_LEFT);
    HIP_TRY(hipGetLastError());
    PYDEM_TRY(fill_look(t, ctr));
    if (h[FD_LEFT]) {
        pydem_set_error("%s: %llu cells of W are still +inf (no relaxation has reached them); the session stays open, the elevation is unchanged",
                        who, (unsigned long long)h[FD_LEFT]);
        return -5;
    }
    hipLaunchKernelGGL(k_fd_final, dim3(gcells), dim3(256), 0, t->stream, t->elev, t->fs_W, t->NN, ctr);
    HIP_TRY(hipGetLastError());
    PYDEM_TRY(fill_look(t, ctr));
    if (n_raised) *n_raised = (int64_t)h[FD_RAISED];
    if (max_depth) *max_depth = as_double(h[FD_DEPTH]);
    if (t->fs_eps > 0) { t->elev_f32 = false; t->elev_dtype = PYDEM_F64; }      // (eps == 0: every value of W is a value of z)
    int rc = 0;
    if (depth) rc = tile_plane_copy(t, t->fs_W, depth, (size_t)t->NN * 8, true);
    fill_seam_drop(t);
    return rc;
}
