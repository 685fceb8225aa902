// terrain.hip -- pydem_terrain_attributes: gradient, aspect, curvatures and hillshade of the resident elevation from a least-squares
// quadratic over a (2k+1)^2 window (Evans 1980 at k = 1, Wood 1996 above).  No reference method; include/pydem_hip.h states the
// definition and this file keeps its operand order, so that the numpy twin (pydem_amd/terrain.py: terrain_attributes_ref) can be
// held to it bit for bit:
//   row moments      R0_j = sum Z, R1_j = sum (double)i * Z, R2_j = sum (double)(i*i) * Z      each from 0.0, ascending i
//   window moments   M00 = sum R0_j, M10 = sum R1_j, M20 = sum R2_j, M01 = sum j * R0_j, M02 = sum (j*j) * R0_j, M11 = sum j * R1_j
//                                                                                              each from 0.0, ascending j
//   ta_finish        the fit, the ground units and the nine planes, one lane per cell
// Two kernels make the moments:
//   k_ta_march       k = 1.  One lane per column, 62 output columns per wavefront (lanes 0 and 63 are halo), rows marched in
//                    registers as k_stencil_march does: a row is loaded once, its neighbours come over DPP wave shifts, and the
//                    three row moments of the last three rows stay in registers.
//   k_ta_window<K>   k = 1..7 (k = 1 only under PYDEM_TA_GENERIC=1).  A workgroup of four wavefronts owns 64 columns x (30 - 2K) rows.
//                    It stages the 30 x (64 + 2K) block with its halo in LDS (cells outside the tile as NaN: their windows come out
//                    undefined by themselves), forms R0 / R1 / R2 once per staged row (horizontal pass, a wavefront per row, a lane
//                    per column: consecutive 8-byte words) and combines them vertically, one lane per cell.
//                    LDS: 30 rows x ((64 + 2K) staged + 3 x 64 moment) doubles = 240 (256 + 2K) bytes: 61 920 at K = 1, 64 800 at
//                    K = 7, under the 65 536 bytes of a static allocation, so that two workgroups share a CU's 160 KiB.  K = 7 is
//                    the last half width at which more than half of the staged rows are output rows (16 of 30); K = 8 would
//                    still fit (65 280 bytes, 14 of 30), K = 9 does not (65 760).  The interface stops at 7.
// A cell is DEFINED when its window lies inside the tile and M00 is not NaN (a NaN elevation in the window); every requested
// plane is NaN elsewhere.  *n_defined: every lane counts its defined cells into the slotted counter of stage_kit.h, one 64-bit
// integer atomic per wavefront (k_ta_march) or per workgroup (k_ta_window).  No floating-point atomics.  The planes and the
// counter block are one block of the tile's (tile_mem.h), grown to the largest request.
#include "stage_kit.h"

namespace {

constexpr int TA_SR = 30;           // staged rows of k_ta_window
constexpr int TA_COLS = 64;         // its output columns
constexpr int TA_MARCH_ROWS = 64;   // output rows per wavefront of k_ta_march

struct TaOuts { double *p[PYDEM_TA_COUNT]; };
// the exact integers of the fit (S2, N, D1, D2, D11), the sun (Le, Ln, Lu) and the vertical exaggeration
struct TaConst { double S2, N, D1, D2, D11, Le, Ln, Lu, zf; };

__device__ __forceinline__ double ta_lane_prev(double x)    // value held by lane-1 (column j-1): DPP wave_shr:1
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ta_lane_next(double x)    // value held by lane+1 (column j+1): DPP wave_shl:1
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// the planes of cell `cell` from its six window moments; returns whether the cell is defined
__device__ __forceinline__ bool ta_finish(double M00, double M10, double M20, double M01, double M02, double M11, bool inside, double gx,
                                          double gy, const TaConst &k, const TaOuts &o, size_t cell)
{
    const bool def = inside && !isnan(M00);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // the fit in index units
    const double d = M10 / k.D1;
    const double e = M01 / k.D1;
    const double cxy = M11 / k.D11;
    const double h = (k.S2 * M00) / k.N;
    const double a = (M20 - h) / k.D2;
    const double b = (M02 - h) / k.D2;
    // ground units: x east, y north (decreasing row)
    const double p = d / gx;
    const double q = -(e / gy);
    if (o.p[PYDEM_TA_DZDX]) o.p[PYDEM_TA_DZDX][cell] = def ? p : nan;
    if (o.p[PYDEM_TA_DZDY]) o.p[PYDEM_TA_DZDY][cell] = def ? q : nan;
    const double g2 = p * p + q * q;
    const bool flat = g2 == 0.0;
    if (o.p[PYDEM_TA_GRADIENT]) o.p[PYDEM_TA_GRADIENT][cell] = def ? __dsqrt_rn(g2) : nan;
    if (o.p[PYDEM_TA_ASPECT]) {
        double v = -1.0;
        if (!flat) {
            v = atan2(-p, -q);
            if (v < 0.0) v = v + 6.283185307179586;
        }
        o.p[PYDEM_TA_ASPECT][cell] = def ? v : nan;
    }
    if (o.p[PYDEM_TA_PROFILE] || o.p[PYDEM_TA_PLAN] || o.p[PYDEM_TA_TANGENTIAL] || o.p[PYDEM_TA_MEAN]) {
        const double r = (2.0 * a) / (gx * gx);
        const double t = (2.0 * b) / (gy * gy);
        const double s = -(cxy / (gx * gy));
        const double w = 1.0 + g2;
        const double pq2 = 2.0 * (p * q);
        const double sw = __dsqrt_rn(w);
        if (o.p[PYDEM_TA_PROFILE]) {
            const double A = ((p * p) * r + pq2 * s) + (q * q) * t;
            const double v = flat ? 0.0 : -A / (g2 * (w * sw));
            o.p[PYDEM_TA_PROFILE][cell] = def ? v : nan;
        }
        if (o.p[PYDEM_TA_PLAN] || o.p[PYDEM_TA_TANGENTIAL]) {
            const double B = ((q * q) * r - pq2 * s) + (p * p) * t;
            if (o.p[PYDEM_TA_PLAN]) {
                const double v = flat ? 0.0 : -B / (g2 * __dsqrt_rn(g2));
                o.p[PYDEM_TA_PLAN][cell] = def ? v : nan;
            }
            if (o.p[PYDEM_TA_TANGENTIAL]) {
                const double v = flat ? 0.0 : -B / (g2 * sw);
                o.p[PYDEM_TA_TANGENTIAL][cell] = def ? v : nan;
            }
        }
        if (o.p[PYDEM_TA_MEAN]) {
            const double C = ((1.0 + q * q) * r - pq2 * s) + (1.0 + p * p) * t;
            o.p[PYDEM_TA_MEAN][cell] = def ? -C / (2.0 * (w * sw)) : nan;
        }
    }
    if (o.p[PYDEM_TA_HILLSHADE]) {
        const double zp = k.zf * p, zq = k.zf * q;
        const double v = ((k.Lu - zp * k.Le) - zq * k.Ln) / __dsqrt_rn(1.0 + (zp * zp + zq * zq));
        o.p[PYDEM_TA_HILLSHADE][cell] = def ? (v > 0.0 ? v : 0.0) : nan;
    }
    return def;
}

// k = 1.  Wavefront w: strip = w % strips (62 columns), chunk = w / strips (TA_MARCH_ROWS output rows).  Rows and columns off the
// tile are read clamped and never used: a cell whose window leaves the tile is not `inside`.
__global__ void __launch_bounds__(256)
k_ta_march(const double *__restrict__ elev, int n, int m, const double *__restrict__ dX2, const double *__restrict__ dY2, int strips,
           int chunks, TaConst k, TaOuts o, u64 *ctr)
{
    const int lane = (int)(threadIdx.x & 63);
    const int wid = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int chunk = wid / strips, strip = wid - chunk * strips;
    if (chunk >= chunks) return;                                    // (uniform per wavefront; no barrier below)
    const int j = strip * 62 + lane - 1;                            // this lane's column (lanes 0 and 63: halo)
    const bool writes = lane >= 1 && lane <= 62 && j < m;
    const bool col_in = j >= 1 && j <= m - 2;
    const double *col = elev + (j < 0 ? 0 : (j < m ? j : m - 1));
    const int i0 = chunk * TA_MARCH_ROWS;
    const int i1 = i0 + TA_MARCH_ROWS < n ? i0 + TA_MARCH_ROWS : n;
    // the row moments of rows i - 1 (a), i (b), i + 1 (c)
#define TA_ROW(z, R0, R1, R2)                                                                  \
    {                                                                                          \
        const double zl_ = ta_lane_prev(z), zr_ = ta_lane_next(z);                             \
        R0 = ((0.0 + zl_) + z) + zr_;                                                          \
        R1 = ((0.0 + -1.0 * zl_) + 0.0 * z) + 1.0 * zr_;                                       \
        R2 = ((0.0 + 1.0 * zl_) + 0.0 * z) + 1.0 * zr_;                                        \
    }
    double a0, a1, a2, b0, b1, b2, c0, c1, c2;
    {
        const double za = col[(size_t)(i0 > 0 ? i0 - 1 : 0) * m], zb = col[(size_t)i0 * m];
        TA_ROW(za, a0, a1, a2)
        TA_ROW(zb, b0, b1, b2)
    }
    double zn = col[(size_t)(i0 + 1 < n ? i0 + 1 : n - 1) * m];
    u64 mine = 0;
    for (int i = i0; i < i1; i++) {
        const double zc = zn;
        zn = col[(size_t)(i + 2 < n ? i + 2 : n - 1) * m];          // the row after the next one, a row ahead of its use
        TA_ROW(zc, c0, c1, c2)
        const double M00 = ((0.0 + a0) + b0) + c0;
        const double M10 = ((0.0 + a1) + b1) + c1;
        const double M20 = ((0.0 + a2) + b2) + c2;
        const double M01 = ((0.0 + -1.0 * a0) + 0.0 * b0) + 1.0 * c0;
        const double M02 = ((0.0 + 1.0 * a0) + 0.0 * b0) + 1.0 * c0;
        const double M11 = ((0.0 + -1.0 * a1) + 0.0 * b1) + 1.0 * c1;
        if (writes) {
            const bool inside = col_in && i >= 1 && i <= n - 2;
            mine += ta_finish(M00, M10, M20, M01, M02, M11, inside, dX2[i], dY2[i], k, o, (size_t)i * m + j) ? 1u : 0u;
        }
        a0 = b0; a1 = b1; a2 = b2; b0 = c0; b1 = c1; b2 = c2;
    }
#undef TA_ROW
    slot_count_wave(ctr, mine, wid);
}

template <int K>
__global__ void __launch_bounds__(256)
k_ta_window(const double *__restrict__ elev, int n, int m, const double *__restrict__ dX2, const double *__restrict__ dY2, int blocks_x,
            TaConst k, TaOuts o, u64 *ctr)
{
    constexpr int SC = TA_COLS + 2 * K, TR = TA_SR - 2 * K;
    __shared__ double s_z[TA_SR][SC];
    __shared__ double s_r[3][TA_SR][TA_COLS];
    slot_count_begin();                                             // (the barriers below come before the count)
    const int by = (int)(blockIdx.x / (unsigned)blocks_x), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)blocks_x);
    const int r0 = by * TR, c0 = bx * TA_COLS;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // the block with its halo; a cell off the tile is NaN
    for (int idx = (int)threadIdx.x; idx < TA_SR * SC; idx += 256) {
        const int rr = idx / SC, cc = idx - rr * SC;
        const int gr = r0 - K + rr, gc = c0 - K + cc;
        s_z[rr][cc] = (gr >= 0 && gr < n && gc >= 0 && gc < m) ? elev[(size_t)gr * m + gc] : nan;
    }
    __syncthreads();
    // horizontal pass: the three row moments of every staged row
    for (int idx = (int)threadIdx.x; idx < TA_SR * TA_COLS; idx += 256) {
        const int rr = idx >> 6, cc = idx & 63;
        double R0 = 0.0, R1 = 0.0, R2 = 0.0;
#pragma unroll
        for (int i = -K; i <= K; i++) {
            const double z = s_z[rr][cc + K + i];
            R0 = R0 + z;
            R1 = R1 + (double)i * z;
            R2 = R2 + (double)(i * i) * z;
        }
        s_r[0][rr][cc] = R0; s_r[1][rr][cc] = R1; s_r[2][rr][cc] = R2;
    }
    __syncthreads();
    // vertical pass: one lane finishes a cell
    u64 mine = 0;
    for (int idx = (int)threadIdx.x; idx < TR * TA_COLS; idx += 256) {
        const int orow = idx >> 6, cc = idx & 63;
        const int gr = r0 + orow, gc = c0 + cc;
        double M00 = 0.0, M10 = 0.0, M20 = 0.0, M01 = 0.0, M02 = 0.0, M11 = 0.0;
#pragma unroll
        for (int j = -K; j <= K; j++) {
            const double R0 = s_r[0][orow + K + j][cc], R1 = s_r[1][orow + K + j][cc], R2 = s_r[2][orow + K + j][cc];
            M00 = M00 + R0;
            M10 = M10 + R1;
            M20 = M20 + R2;
            M01 = M01 + (double)j * R0;
            M02 = M02 + (double)(j * j) * R0;
            M11 = M11 + (double)j * R1;
        }
        if (gr < n && gc < m)
            mine += ta_finish(M00, M10, M20, M01, M02, M11, true, dX2[gr], dY2[gr], k, o, (size_t)gr * m + gc) ? 1u : 0u;
    }
    slot_count(ctr, wave_add(mine));
}

template <int K>
void launch_window(pydem_tile *t, const TaConst &k, const TaOuts &o, u64 *ctr)
{
    const int64_t bx = cdiv(t->m, TA_COLS), by = cdiv(t->n, TA_SR - 2 * K);
    hipLaunchKernelGGL((k_ta_window<K>), dim3((unsigned)(bx * by)), dim3(256), 0, t->stream, (const double *)t->elev, (int)t->n, (int)t->m,
                       (const double *)t->dX2, (const double *)t->dY2, (int)bx, k, o, ctr);
}

}  // namespace

int stage_terrain_attributes(pydem_tile *t, int half_width, const double *light, double z_factor, double *const *outs, double *ms,
                             int64_t *n_defined)
{
    const char *who = "pydem_terrain_attributes";
    if (half_width < 1 || half_width > 7) { pydem_set_error("%s: half_width %d (1 .. 7 allowed)", who, half_width); return -2; }
    int wanted = 0;
    if (outs) for (int a = 0; a < PYDEM_TA_COUNT; a++) wanted += outs[a] ? 1 : 0;
    if (!wanted) { pydem_set_error("%s: no plane was asked for", who); return -2; }
    if (outs[PYDEM_TA_HILLSHADE] && !light) { pydem_set_error("%s: a hillshade needs the light vector", who); return -2; }
    if (!(std::isfinite(z_factor) && z_factor > 0)) { pydem_set_error("%s: z_factor must be finite and > 0 (got %g)", who, z_factor); return -2; }
    if (!t->spacing_set) { pydem_set_error("%s: call pydem_tile_set_spacing first", who); return -3; }
    if (!t->elev || !t->have[PYDEM_ELEV]) { pydem_set_error("%s: required input field %d is missing", who, (int)PYDEM_ELEV); return -3; }

    const int64_t NN = t->NN;
    const double kk = (double)half_width, N = 2.0 * kk + 1.0;
    TaConst k;
    k.N = N;
    k.S2 = kk * (kk + 1.0) * N / 3.0;                                               // (exact: integers far below 2^53)
    const double S4 = kk * (kk + 1.0) * N * (3.0 * kk * kk + 3.0 * kk - 1.0) / 15.0;
    k.D1 = N * k.S2;
    k.D2 = N * S4 - k.S2 * k.S2;
    k.D11 = k.S2 * k.S2;
    k.Le = light ? light[0] : 0.0; k.Ln = light ? light[1] : 0.0; k.Lu = light ? light[2] : 0.0;
    k.zf = z_factor;

    // one block: the counter block (8192 bytes), then the requested planes
    const size_t need = SLOT_BYTES + (size_t)wanted * (size_t)NN * 8;
    PYDEM_TRY(tile_reserve(t, &t->ta_mem, &t->ta_bytes, need, need, false));
    u64 *ctr = (u64 *)t->ta_mem;
    TaOuts o;
    {
        double *next = (double *)((char *)t->ta_mem + SLOT_BYTES);
        for (int a = 0; a < PYDEM_TA_COUNT; a++) {
            o.p[a] = outs[a] ? next : nullptr;
            if (outs[a]) next += NN;
        }
    }
    Events<2> ev;
    PYDEM_TRY(ev.create());
    HIP_TRY(hipMemsetAsync(ctr, 0, SLOT_BYTES, t->stream));
    HIP_TRY(hipEventRecord(ev.e[0], t->stream));
    if (half_width == 1 && !env_switch("PYDEM_TA_GENERIC", false)) {     // (read per call: the tests switch it) k = 1 through k_ta_window too
        const int64_t strips = cdiv(t->m, 62), chunks = cdiv(t->n, TA_MARCH_ROWS);
        hipLaunchKernelGGL(k_ta_march, dim3((unsigned)cdiv(strips * chunks, 4)), dim3(256), 0, t->stream, (const double *)t->elev, (int)t->n,
                           (int)t->m, (const double *)t->dX2, (const double *)t->dY2, (int)strips, (int)chunks, k, o, ctr);
    } else {
        switch (half_width) {
            case 1: launch_window<1>(t, k, o, ctr); break;
            case 2: launch_window<2>(t, k, o, ctr); break;
            case 3: launch_window<3>(t, k, o, ctr); break;
            case 4: launch_window<4>(t, k, o, ctr); break;
            case 5: launch_window<5>(t, k, o, ctr); break;
            case 6: launch_window<6>(t, k, o, ctr); break;
            default: launch_window<7>(t, k, o, ctr); break;
        }
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_slot_total<>, dim3(1), dim3(64), 0, t->stream, ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], t->stream));
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr + SLOT_TOTAL, 8, hipMemcpyDeviceToHost, t->stream));      // (the pinned mirror: scratch of every stage)
    HIP_TRY(hipStreamSynchronize(t->stream));
    const u64 count = *(volatile u64 *)t->h_counters;
    for (int a = 0; a < PYDEM_TA_COUNT; a++)
        if (outs[a]) PYDEM_TRY(tile_plane_copy(t, o.p[a], outs[a], (size_t)NN * 8, true));
    if (n_defined) *n_defined = (int64_t)count;
    if (ms) PYDEM_TRY(ev.elapsed(0, 1, ms));
    return 0;
}
