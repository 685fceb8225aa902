// stencil.hip -- K1: Tarboton D-infinity slope magnitude + direction (3x3 stencil, 8 facets).
//
// Replaces _tarboton_slopes_directions (reference pydem/dem_processing.py:1753-1903) with its
// helpers _get_d1_d2 (:1905-1938) and _calc_direction (:1942-1991).  The reference makes 8
// full-array numpy passes (one per facet) plus 4 edge and 4 corner passes; here one kernel
// handles every interior cell and a second O(perimeter) kernel applies the edge/corner rules.
// The default interior kernel is k_stencil_march: one lane per column, rows marched in registers
// band by band, the neighbours' quotients through DPP wavefront shifts, facet states as mask algebra
// on the scalar unit; k_stencil_interior -- all 8 facets per cell from an LDS
// halo tile -- is the first version, kept as PYDEM_STENCIL=tile (5.3 ms against 3.0 ms at 16384^2).
//
// Bounded by HBM: algorithmic traffic 24 B/cell (read elev 8, write mag 8 + direction 8), plus
// 1 B/cell for the flat0 mask consumed by the flats stage.  No MFMA: there is no contraction.
// Compiled with -ffp-contract=off: the facet arithmetic must round exactly like numpy's
// separate multiply/add ufuncs or exact ties on integer DEMs break differently.
#include "internal.h"
#include <float.h>
#include <stdlib.h>
#include <string.h>

#define PI_D 3.141592653589793

namespace {

constexpr int TX = 64;    // tile columns (one wavefront wide: 512 B rows)
constexpr int TY = 32;    // tile rows
constexpr int RPT = 8;    // rows marched per thread (256 threads = 64 x 4)
constexpr int LW = TX + 2;

// winner bookkeeping across the 8 facets: `rad2 > mag` with strict '>' so the first facet wins
// exact ties (dem_processing.py:1986-1989)
struct Best {
    double rad2;   // best squared magnitude so far (-1 = none)
    double s1, s2; // slopes of the winning facet (for the final atan2)
    double theta;  // table angle of the winning facet
    int k;         // winning facet
    int kind;      // 1: r = 0 (cardinal), 2: r = theta (diagonal), 3: r = atan2(s2, s1)
    int tie;       // kind 3 with s2 * d1 == s1 * d2 exactly: atan2(s2, s1) IS theta (see STATES in march_band)
};

// One facet of _calc_direction (:1958-1989).  s1, s2, sd are the three slopes; d1, d2 the
// spacings (only used to decide r > theta by cross-multiplication instead of an arctangent:
// for s1 > 0, s2 > 0: atan2(s2, s1) > atan2(d2, d1)  <=>  s2*d1 > s1*d2; when the two
// products agree to within a few ulps the comparison is re-done with atan2 exactly as the
// reference does, so exact ties (s1 == s2, d1 == d2 on integer DEMs) resolve identically).
__device__ __forceinline__ void facet(double s1, double s2, double sd, double d1, double d2,
                                      double theta, int k, Best &b)
{
    const double s1_2 = s1 * s1;
    const bool s1le = s1 <= 0, s2le = s2 <= 0, s1gt = s1 > 0, s2gt = s2 > 0;
    double rad2 = s1_2 + s2 * s2;
    int kind = 3;
    bool rgt = false, tie = false;
    if (s1gt && s2gt) {
        const double a = s2 * d1, c = s1 * d2;
        rgt = a > c;
        tie = a == c;                                                   // slopes in the exact ratio of the spacings: r == theta, not greater
        if (!tie && fabs(a - c) <= 8.0 * DBL_EPSILON * fmax(a, c)) rgt = atan2(s2, s1) > theta;
    }
    if ((s1le && s2gt) || rgt) { rad2 = sd * sd; kind = 2; }           // I1 :1973-1976
    if (s1gt && s2le) { rad2 = s1_2; kind = 1; }                       // I2 :1978-1981 (r < 0 implies s2 < 0)
    if (s1le && (s2le || (s2gt && sd <= 0))) rad2 = -1.0;              // I3 :1983-1984
    if (rad2 > b.rad2) {                                               // I4 :1986-1989
        b.rad2 = rad2; b.s1 = s1; b.s2 = s2; b.theta = theta; b.k = k; b.kind = kind; b.tie = (kind == 3 && tie) ? 1 : 0;
    }
}

// atan2(y, x) for y > 0, x > 0 (the only case an unclamped facet can produce, see facet()).
// ocml's general atan2 costs ~130 fp64 operations per cell -- more than a quarter of the whole
// stencil; this one is ~45: q = min/max in (0, 1], c = nearest multiple of 1/16,
// atan(q) = atan(c) + atan(u), u = (q - c)/(1 + q*c), |u| <= 1/32, odd Taylor series to u^11
// (truncation < 1e-19 relative), table of correctly rounded atan(k/16).  Error <= ~1.5 ulp of the result: 1.35 measured on
// the designed ratios of tests/stencil_fields.py (both sides of every switch of the table entry, with and without the swap,
// slopes from 2^-470 to 2^470), which tests/test_gpu_stencil_bits.py holds to 2 ulp on every path of this file.
__device__ __constant__ const double ATAN_16[17] = {
    0, 0.06241880999595735, 0.12435499454676144, 0.18534794999569476, 0.24497866312686414, 0.30288486837497142,
    0.35877067027057225, 0.41241044159738732, 0.46364760900080609, 0.51238946031073773, 0.55859931534356244,
    0.60228734613496415, 0.64350110879328437, 0.68231655487474807, 0.71882999962162453, 0.75315128096219441,
    0.78539816339744828};

__device__ __forceinline__ double atan2_pos(double y, double x)
{
    // atan(num/den), num <= den: c = nearest multiple of 1/16 to the quotient (a raw reciprocal is good enough to pick
    // it), u = (num/den - c) / (1 + c num/den) = (num - c den) / (den + c num): one division
    const bool swap = y > x;
    const double num = swap ? x : y, den = swap ? y : x;
    const double kf = rint(num * __builtin_amdgcn_rcp(den) * 16.0);
    const double c = kf * 0.0625;
    const double u = __builtin_fma(-c, den, num) / __builtin_fma(c, num, den);
    const double w = u * u;
    double p = __builtin_fma(w, -1.0 / 11, 1.0 / 9);
    p = __builtin_fma(w, p, -1.0 / 7);
    p = __builtin_fma(w, p, 1.0 / 5);
    p = __builtin_fma(w, p, -1.0 / 3);
    p = __builtin_fma(w * u, p, u);
    const double a = ATAN_16[(int)kf] + p;
    return swap ? PI_D / 2 - a : a;
}

// direction of the winner: r * ang[1] + ang[0] * pi / 2 (:1989); ang_adj table :184-193
__device__ __forceinline__ double direction_of(int k, int kind, double s1, double s2, double theta, int tie = 0)
{
    if (tie) kind = 2;                             // (the arctangent of the winner equals the table angle exactly)
    if (k < 0) return -1.0;
    const int a0 = (k + 1) >> 1;                   // 0,1,1,2,2,3,3,4
    const double a1 = (k & 1) ? -1.0 : 1.0;        // 1,-1,1,-1,...
    double r = 0.0;
    if (kind == 2) r = theta;
    else if (kind == 3) r = atan2_pos(s2, s1);
    return r * a1 + (double)a0 * PI_D / 2;
}

__device__ __forceinline__ double winner_direction(const Best &b) { return direction_of(b.k, b.kind, b.s1, b.s2, b.theta, b.tie); }

// Lean facet for the marching kernel: only (rad2, code = 4*k + kind) is tracked; the winner's
// slopes are re-selected once at the end.  Same decisions as facet() except that `r > theta` is the
// plain cross-multiplication (exact ties compare equal on both sides and stay unclamped, like
// atan2(s, s) == atan2(d, d) in the reference).
struct Acc { double rad2; int code; };

// squares are passed in: an edge quotient enters up to two facets of a cell, its square is computed once
__device__ __forceinline__ void facet_lean(double s1, double s2, double sd, double s1sq, double s2sq, double sdsq,
                                           double d1, double d2, int k, Acc &acc)
{
    const bool s1gt = s1 > 0, s1le = s1 <= 0, s2gt = s2 > 0, s2le = s2 <= 0;
    const bool rgt = s1gt && s2gt && (s2 * d1 > s1 * d2);
    const bool diag = (s1le && s2gt) || rgt;                    // I1 :1973-1976
    const bool card = s1gt && s2le;                             // I2 :1978-1981
    const bool none = s1le && (s2le || (s2gt && sd <= 0));      // I3 :1983-1984 (rad2 = -1 never beats the running maximum)
    const double cand = card ? s1sq : (diag ? sdsq : s1sq + s2sq);
    const bool upd = !none && cand > acc.rad2;                  // I4 :1986-1989
    acc.rad2 = upd ? cand : acc.rad2;
    acc.code = upd ? 4 * k + (card ? 1 : (diag ? 2 : 3)) : acc.code;
}

// x / d for a per-row spacing d with r = RN(1/d) from the host: q = RN(x*r), one exact remainder, one
// correction -- Markstein's sequence returns the correctly rounded quotient (checked against 4e8
// IEEE divisions on the host; tests/test_gpu_stencil_bits.py compares magnitudes that are one such quotient, by spacings
// whose reciprocals round badly, with numpy's bit for bit -- the other tests only to 1e-11), 3 full-rate
// operations instead of ~11 with a quarter-rate v_rcp_f64
__device__ __forceinline__ double div_row(double x, double d, double r)
{
#ifdef PYDEM_STENCIL_CHEAP      // upper-bound experiment (DESIGN.md section 4 "Round 4" (5)): NOT exact, never the product build
    (void)d; return x * r;
#endif
    const double q = x * r;
    const double rem = __builtin_fma(-q, d, x);
    return __builtin_fma(rem, r, q);
}

// elevation difference in the dtype the reference subtracts in: numpy keeps a float32 DEM float32 through
// `data[slc0] - data[slc1]` and only the division by the float64 spacing promotes (_calc_direction :1958-1962), so a
// float32 tile (uploaded PYDEM_F32, conditioning off) rounds every difference to 24 bits first.  The casts are exact
// (the device copy holds the float32 values), RN subtraction is sign-symmetric in either width.
template <bool F32>
__device__ __forceinline__ double zsub(double a, double b)
{
    if (F32) return (double)((float)a - (float)b);
    return a - b;
}

// all 8 facets of an interior cell.  tn = spacing row i-1 (facets 0-3), ts = row i (facets 4-7)
// (_get_d1_d2 :1912-1924: facets 0,3,4,7 use d1 = dX, d2 = dY; facets 1,2,5,6 d1 = dY, d2 = dX)
template <bool F32>
__device__ __forceinline__ void eight_facets(double z0, double zN, double zS, double zE, double zW,
                                             double zNE, double zNW, double zSW, double zSE,
                                             const RowTab &tn, const RowTab &ts, Best &b)
{
    const double sdNE = zsub<F32>(z0, zNE) / tn.hyp, sdNW = zsub<F32>(z0, zNW) / tn.hyp;
    const double sdSW = zsub<F32>(z0, zSW) / ts.hyp, sdSE = zsub<F32>(z0, zSE) / ts.hyp;
    const double s1N = zsub<F32>(z0, zN) / tn.dY, s1S = zsub<F32>(z0, zS) / ts.dY;
    facet(zsub<F32>(z0, zE) / tn.dX, zsub<F32>(zE, zNE) / tn.dY, sdNE, tn.dX, tn.dY, tn.thA, 0, b);
    facet(s1N, zsub<F32>(zN, zNE) / tn.dX, sdNE, tn.dY, tn.dX, tn.thB, 1, b);
    facet(s1N, zsub<F32>(zN, zNW) / tn.dX, sdNW, tn.dY, tn.dX, tn.thB, 2, b);
    facet(zsub<F32>(z0, zW) / tn.dX, zsub<F32>(zW, zNW) / tn.dY, sdNW, tn.dX, tn.dY, tn.thA, 3, b);
    facet(zsub<F32>(z0, zW) / ts.dX, zsub<F32>(zW, zSW) / ts.dY, sdSW, ts.dX, ts.dY, ts.thA, 4, b);
    facet(s1S, zsub<F32>(zS, zSW) / ts.dX, sdSW, ts.dY, ts.dX, ts.thB, 5, b);
    facet(s1S, zsub<F32>(zS, zSE) / ts.dX, sdSE, ts.dY, ts.dX, ts.thB, 6, b);
    facet(zsub<F32>(z0, zE) / ts.dX, zsub<F32>(zE, zSE) / ts.dY, sdSE, ts.dX, ts.dY, ts.thA, 7, b);
}

__device__ __forceinline__ Best best_init()
{
    Best b; b.rad2 = -1.0; b.s1 = 0; b.s2 = 0; b.theta = 0; b.k = -1; b.kind = 0; b.tie = 0;
    return b;
}

// ---------------------------------------------------------------------------------------------
// interior kernel: block = 64 x 4 threads, tile = 64 columns x 32 rows, LDS halo tile 66 x 34.
// Tiles are column-aligned to multiples of 64 so each wavefront stores whole 512 B row segments.
// XCD-aware tile order: consecutive block ids land on different XCDs (b % 8), so block b is
// remapped to tile (b % 8) * tiles_per_xcd + b / 8: each XCD walks a contiguous band of tiles
// and neighbouring tiles share halo lines in the same L2.
// ---------------------------------------------------------------------------------------------
template <bool XCD_SWIZZLE, bool F32>
__global__ __launch_bounds__(256) void k_stencil_interior(const double *__restrict__ elev, int n, int m,
                                                          const RowTab *__restrict__ rowtab,
                                                          double *__restrict__ mag, double *__restrict__ dir,
                                                          uint8_t *__restrict__ flat0, int tiles_x, int tiles_total)
{
    __shared__ double tile[(TY + 2) * LW];
    int tid = blockIdx.x;
    if (XCD_SWIZZLE) {
        const int per = (tiles_total + 7) >> 3;
        tid = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
        if (tid >= tiles_total) return;
    }
    const int by = tid / tiles_x, bx = tid - by * tiles_x;
    const int j0 = bx * TX, i0 = by * TY;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;

    for (int idx = threadIdx.x; idx < (TY + 2) * LW; idx += 256) {
        const int lr = idx / LW, lc = idx - lr * LW;
        const int gi = i0 - 1 + lr, gj = j0 - 1 + lc;
        double v = 0.0;
        if (gi >= 0 && gi < n && gj >= 0 && gj < m) v = elev[(size_t)gi * m + gj];
        tile[idx] = v;
    }
    __syncthreads();

    const int j = j0 + tx;
    const int lc = tx + 1;
    int lr = ty * RPT + 1;                       // LDS row of the first cell of this thread
    // 3x3 window, rolled down the column
    double aW = tile[(lr - 1) * LW + lc - 1], a0 = tile[(lr - 1) * LW + lc], aE = tile[(lr - 1) * LW + lc + 1];
    double cW = tile[lr * LW + lc - 1], c0 = tile[lr * LW + lc], cE = tile[lr * LW + lc + 1];
#pragma unroll
    for (int q = 0; q < RPT; q++, lr++) {
        const int i = i0 + ty * RPT + q;
        const double bW = tile[(lr + 1) * LW + lc - 1], b0 = tile[(lr + 1) * LW + lc], bE = tile[(lr + 1) * LW + lc + 1];
        if (i >= 1 && i < n - 1 && j >= 1 && j < m - 1) {
            const RowTab tn = rowtab[i - 1], ts = rowtab[i];
            Best b = best_init();
            eight_facets<F32>(c0, a0, b0, cE, cW, aE, aW, bW, bE, tn, ts, b);
            const size_t c = (size_t)i * m + j;
            mag[c] = b.rad2 > 0 ? sqrt(b.rad2) : b.rad2;           // :1901
            dir[c] = winner_direction(b);
            flat0[c] = (b.rad2 == -1.0);
        }
        aW = cW; a0 = c0; aE = cE;
        cW = bW; c0 = b0; cE = bE;
    }
}

// ---------------------------------------------------------------------------------------------
// Variant 2 -- "march": one lane per column, rows marched in registers, quotients shared.
// Every slope the 8 facets need is an EDGE quotient: (z_a - z_b)/d for two neighbouring cells and
// a row spacing.  Per cell there are only 5 distinct ones (E-edge over the north and the south
// spacing, the S-edge, the SE and SW diagonals); the other 13 of the 18 divisions of variant 1 are
// the same numbers seen from the neighbouring cell (IEEE subtraction and division are sign-
// symmetric, so -(a-b)/d == (b-a)/d bit for bit).  Each lane computes its 5 quotients when a row
// enters its 3-row window and fetches the neighbours' copies with wavefront lane shifts; the
// arithmetic that reaches `facet()` is bit-identical to variant 1.  A wavefront covers 64 columns
// and produces 62 (lanes 0 and 63 are halo), rows are 512 B coalesced loads, no LDS.
// ---------------------------------------------------------------------------------------------
// lane shifts as DPP moves (v_mov_b32_dpp wave_shr:1 / wave_shl:1 -- gfx9 wavefront shifts; 2 VALU
// moves per double, no LDS crossbar round trip).  The lane without a neighbour (0 / 63: halo lanes, their results are
// never stored) reads zero: with `bound_ctrl` the move has no tied old value, i.e. no copy of the source in front of
// it (keeping the own value there cost a v_mov per dword: 16 of the 312 vector instructions of a row).
__device__ __forceinline__ double lane_prev(double x)    // value held by lane-1 (column j-1)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_next(double x)    // value held by lane+1 (column j+1)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

constexpr int MARCH_ROWS = 128;   // output rows per wavefront on large tiles (fewer on small ones: the chip wants >= ~10 k wavefronts)

// ---- lane masks.  A comparison lands in an SGPR pair; everything that is only boolean algebra on comparison results
// (the I1..I4 logic of _calc_direction, :1973-1989, and the "same test seen from the neighbouring column" shifts) is
// done on those pairs by the scalar unit, which runs beside the vector pipeline this kernel is bound by.
typedef uint64_t lmask;
#define LM(cond) __builtin_amdgcn_ballot_w64(cond)
#define ON(mask) __builtin_amdgcn_inverse_ballot_w64(mask)
__device__ __forceinline__ lmask from_left(lmask x) { return x << 1; }    // the test lane-1 (column j-1) made
__device__ __forceinline__ lmask from_right(lmask x) { return x >> 1; }   // the test lane+1 (column j+1) made

// v_max_f64 without the canonicalising self-maximum the compiler puts in front of fmax() operands it cannot prove quiet
// (no NaN reaches this: the window test below sends rows with NaN / huge elevations down the exact path)
__device__ __forceinline__ double vmax(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a candidate that is not in play: high dword replaced by that of -1.0, so it is <= -1.0 and loses every maximum against
// the -1.0 start value (one v_cndmask instead of a 64-bit select)
__device__ __forceinline__ double only_if(lmask keep, double x, int dead_hi)
{
    const int hi = ON(keep) ? __double2hiint(x) : dead_hi;
    return __hiloint2double(hi, __double2loint(x));
}
__device__ __forceinline__ double pick(lmask m, double a, double b) { return ON(m) ? a : b; }

// IEEE division u = a / b for the arctangent's reduced argument, 0 <= a, 0 < b with b within a factor 2 of the larger
// slope: reciprocal seed + two Newton steps + Markstein's residual correction (correctly rounded like `/`; without the
// exponent rescue of the generic expansion).  The window test bounds elevations (< 2^500) and spacings (2^-500 .. 2^500), NOT
// slopes: all it guarantees here is that a and b are finite.  The sequence needs more -- the reciprocal, the Newton residuals
// and the last remainder (about 2^-53 a) must stay normal -- which slopes within [2^-480, 2^480] leave ample room for; that
// is the range tests/test_gpu_stencil_bits.py holds to the bit and to 2 ulp.  Nothing is promised for slopes outside it.
__device__ __forceinline__ double div_pos(double a, double b)
{
#ifdef PYDEM_STENCIL_CHEAP
    { double y0 = __builtin_amdgcn_rcp(b); const double e0 = __builtin_fma(-b, y0, 1.0); y0 = __builtin_fma(y0, e0, y0); return a * y0; }
#endif
    double y = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    const double q = a * y;
    const double rem = __builtin_fma(-q, b, a);
    return __builtin_fma(rem, y, q);
}

// sqrt(x) for the squares of slopes within [2^-480, 2^480] (tests/test_gpu_stencil_bits.py: numpy's bits there): the compiler's
// correctly rounded expansion (reciprocal square root seed, Goldschmidt step, two residual corrections) without the exponent
// scaling and the zero / infinity special cases it wraps around it.  The window test bounds elevations and spacings, not
// slopes: a far smaller square loses the last place (its residuals go subnormal), and +inf -- the square of a slope next to a
// huge elevation, which the exact path does meet -- would come out as NaN (rsq(inf) = 0, times inf): mag_of() keeps it away
__device__ __forceinline__ double sqrt_window(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g); h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}

// the magnitude a cell stores (:1901): the root of a positive finite square; -1 (no facet descends), 0, NaN and +inf (the
// reference's sqrt(inf) = inf) as they are.  One v_cmp_class instead of the v_cmp_gt of `M > 0`.
__device__ __forceinline__ double mag_of(double M)
{
    return __builtin_amdgcn_class(M, 0x180) ? sqrt_window(M) : M;      // 0x180: +normal | +subnormal
}

__device__ __forceinline__ double atan2_pos_fast(double y, double x, const double *atan_16)
{
    const bool swap = y > x;
    double num, den;                                       // (both positive, no NaN on this path: the plain minimum / maximum)
    asm("v_min_f64 %0, %1, %2" : "=v"(num) : "v"(y), "v"(x));
    asm("v_max_f64 %0, %1, %2" : "=v"(den) : "v"(y), "v"(x));
    const double kf = rint(num * __builtin_amdgcn_rcp(den) * 16.0);
    const double c = kf * 0.0625;
    const double u = div_pos(__builtin_fma(-c, den, num), __builtin_fma(c, num, den));
    const double w = u * u;
    double p = __builtin_fma(w, -1.0 / 11, 1.0 / 9);
    p = __builtin_fma(w, p, -1.0 / 7);
    p = __builtin_fma(w, p, 1.0 / 5);
    p = __builtin_fma(w, p, -1.0 / 3);
    p = __builtin_fma(w * u, p, u);
    const double a = atan_16[(int)kf] + p;
    return swap ? PI_D / 2 - a : a;
}

// The marching kernel works band by band: the band between rows b and b+1 (spacing row b) holds every quotient that
// the four south facets (4-7) of the cells of row b and the four north facets (0-3) of the cells of row b+1 need --
// the E-edges of both rows over dX[b], the vertical edges, the two diagonals (_get_d1_d2 :1912-1924 gives facets 0-3 the
// spacing row above the cell and 4-7 the one below).  Per band and lane (= column j): 5 quotients of its own (the fifth
// is the E-edge of row b+1 over dX[b+1], kept for the next band), 8 lane shifts, 10 sign tests, 11 squares, 7 cross
// products.  After that no facet needs arithmetic on slopes: each is in one of four states (none / cardinal / diagonal
// / interior, :1973-1984) decided by mask algebra; the squared magnitude of a half (north or south) is a maximum over 9
// ready-made numbers (4 interior sums, 3 distinct cardinal squares, 2 distinct diagonal squares) and "the first facet
// that reaches the maximum" (:1986-1989, strict >) is 9 equality tests plus mask algebra.  A cell's north half (computed
// in the band above it) is carried to the next iteration as (maximum, slopes of an interior winner, four masks); the
// north half wins ties against the south half (facets 0-3 come first).
// Names: hs1 / hn = E-edge quotient of row b / b+1 over dX[b]; v = vertical edge b -> b+1; se / sw = diagonals from
// (b, j) to (b+1, j+-1); suffix L / R = the copy of the lane to the left / right.

// what a band hands to the next one: its bottom row (the next top row) with the E-edge over the next spacing, and the
// north half of the cells of that row
struct BandCarry {
    double z0;                 // elevations of the top row
    double hs1, hsL1;          // E-edge of the top row over the band's dX, own and left neighbour's
    lmask Phs1, Nhs1;          // hs1 > 0, hs1 < 0
    double Mn;                 // north half: squared magnitude
    lmask Nk0, Nk1, NdA, NdB, Nint;   // north winner: bits of its facet number; diagonal with table angle thA / thB; interior (r = atan2(s2, s1))
    double thAn, thBn;         // those angles (spacing row above)
    bool ex_top;               // NaN / huge elevations in the top row
};
// the row table of a band as VECTOR registers: as scalars the two rows in flight take 32 of the ~100 SGPRs, and the mask
// algebra then spills its lane masks into VGPR lanes (35 v_readlane / v_writelane per row).  The rows of the workgroup's
// chunk are copied to LDS once (130 x 64 B) and read from there as broadcasts: a GLOBAL load per band would be counted by
// vmcnt together with the band's stores, and the compiler's waits then sit out the store latency in every band.
struct RowV { double dX, dY, hyp, thA, thB, rdX, rdY, rhyp; };
__device__ __forceinline__ RowV rowv_load(const double *rtv, int r)      // rtv: the workgroup's copy of its rows' table in LDS
{
    const double4 *p = reinterpret_cast<const double4 *>(rtv + r * 8);
    const double4 a = p[0], b = p[1];
    RowV v;
    v.dX = a.x; v.dY = a.y; v.hyp = a.z; v.thA = a.w; v.thB = b.x; v.rdX = b.y; v.rdY = b.z; v.rhyp = b.w;
    return v;
}
// The slopes of the winning facet are FETCHED, not selected: every lane leaves the three quotients a band computes (hn, hs1, v)
// in LDS, two bands deep; once the winner's facet number k is known (three mask bits) and whether it is an interior winner,
// its two slopes are two ds_read_b64 at offsets from a 9-entry table (facet k -> which array, which lane, which of the two
// bands; entry 8 = "not interior" -> the constants (1, 0), whose arctangent is exactly 0).  Carrying the candidates' slopes
// through select chains instead (the north half's to the next band, then north against south) cost 32 v_cndmask per row
// and four carried registers.
constexpr int QS = 66;                         // lanes + one pad slot either side
struct WaveQ { double a[2][3][QS]; double one[QS], zero[QS]; double dg[2][QS]; };      // a[band parity][0: hn, 1: hs1, 2: v]; dg: se, sw of the running band
// Producer / store split (round 6 experiment, PYDEM_STENCIL_SPLIT=1; k_stencil_march_split): a compute wavefront leaves the
// (mag, direction, flat0) of a finished row in a small ring in LDS instead of storing it; ONE more wavefront per workgroup drains the
// rings of its eleven producers into HBM.  prod / cons count rows of the chunk; a producer may be SR_ROWS rows ahead.
#ifndef PYDEM_SPLIT_ROWS
#define PYDEM_SPLIT_ROWS 4
#endif
constexpr int SR_ROWS = PYDEM_SPLIT_ROWS;
struct StoreRing { double mag[SR_ROWS][64]; double dir[SR_ROWS][64]; uint8_t flat[SR_ROWS][64]; int prod, cons, pad[2]; };
struct MarchCtx {
    StoreRing *ring;                           // (split kernel only)
    WaveQ *q; const uint16_t *tab;             // tab[parity of the running band][k][0 / 1]: byte offsets of s1 / s2 from &q->a[0][0][lane]
    const double *col; const RowTab *rowtab; const double *rtv; const double *atan_16;
    double *mag, *dir; uint8_t *flat0;
    int n, m, j, i0, r0, exact_only; bool writes;
};

// The row in flight.  The compiler's own bookkeeping of vmcnt treats a load behind stores as "wait for everything": every band
// then sat out the latency of its own stores (~2 us under load against 0.4 us of arithmetic; the vector ALUs idled 40 % of
// the time with three wavefronts per SIMD).  The row is therefore requested by hand and waited for by hand: vmcnt counts in
// issue order, the three stores of a band are issued AFTER the request, so "at most three still outstanding" at the end of
// the band means the row has arrived and says nothing about the stores.  (The first band of a wavefront issues no stores:
// it waits for everything.)
__device__ __forceinline__ double row_request(const double *p)
{
    double v;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    return v;
}
template <int YOUNGER>
__device__ __forceinline__ void row_arrived(double &v)
{
#ifdef PYDEM_STENCIL_NOSTORE
    if (false) ;
#else
    if (YOUNGER == 3) asm volatile("s_waitcnt vmcnt(3)" : "+v"(v) : : "memory");
#endif
    else asm volatile("s_waitcnt vmcnt(0)" : "+v"(v) : : "memory");
}

// between a lane's LDS store and its neighbours' loads of that slot: nothing for the hardware to do (the LDS operations of a
// wavefront execute in order), but the compiler must not move a load of slot lane +- 1 above the store of slot lane
__device__ __forceinline__ void lanes_published()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

template <bool F32, int P, bool FIRST = false, bool SPLIT = false>
__device__ __forceinline__ void march_band(const MarchCtx &cx, BandCarry &c, const RowV &ts, RowV &tnx, const int b, const double zS, double &z_ahead)
{
    const int lane = (int)(threadIdx.x & 63);
#ifdef PYDEM_STENCIL_NOMATH     // memory-pattern experiment (NOT a product build): the loads and stores of the band, no arithmetic
    {
        z_ahead = row_request(cx.col + (size_t)((b + 2 <= cx.n - 1) ? b + 2 : cx.n - 1) * cx.m);
        if (cx.writes && b >= cx.i0) {
            const size_t cc = (size_t)b * cx.m + cx.j;
            cx.mag[cc] = c.z0 + zS; cx.dir[cc] = c.z0 - zS; cx.flat0[cc] = zS > c.z0 ? 1 : 0;
        }
        c.z0 = zS; tnx = ts;
        row_arrived<FIRST ? 0 : 3>(z_ahead);
        return;
    }
#endif
    const int n = cx.n, m = cx.m;
    const int dead_hi = __double2hiint(-1.0);
    const double BIG = 0x1p500;
    // software pipeline: the elevations of row b+2 and the spacing row b+1 are requested now and first touched in the
    // next band / at the very end of this one, so neither wait is exposed (the caller alternates two registers for the
    // row in flight: it is never copied before it has been used)
    tnx = rowv_load(cx.rtv, ((b + 1 <= n - 2) ? b + 1 : n - 2) - cx.r0);      // (the caller alternates two register sets, like for the row in flight)
    z_ahead = row_request(cx.col + (size_t)((b + 2 <= n - 1) ? b + 2 : n - 1) * m);
    const double thAs = ts.thA, thBs = ts.thB;
    const double z0 = c.z0, hs1 = c.hs1, hsL1 = c.hsL1;
    const lmask Phs1 = c.Phs1, Nhs1 = c.Nhs1;
    // ---- row b+1 enters
    const bool ex_bot = LM(!(fabs(zS) < BIG)) != 0;
    const bool exact = c.ex_top || ex_bot;
    const double zES = lane_next(zS), zWS = lane_prev(zS);
    const double dE = zsub<F32>(zS, zES);
    const double hn = div_row(dE, ts.dX, ts.rdX);
    const double v = div_row(zsub<F32>(z0, zS), ts.dY, ts.rdY);
    const double se = div_row(zsub<F32>(z0, zES), ts.hyp, ts.rhyp);
    const double sw = div_row(zsub<F32>(z0, zWS), ts.hyp, ts.rhyp);
    // the neighbours' copies of the quotients come back from the slots the lanes have just written (a ds_read_b64 each
    // instead of two DPP moves: the kernel is bound by its vector instructions, the LDS port is idle)
    cx.q->a[P][0][1 + lane] = hn; cx.q->a[P][2][1 + lane] = v; cx.q->dg[0][1 + lane] = se; cx.q->dg[1][1 + lane] = sw;
    lanes_published();
    const double hnL = cx.q->a[P][0][lane], vL = cx.q->a[P][2][lane], vR = cx.q->a[P][2][2 + lane];
    const double seL = cx.q->dg[0][lane], swR = cx.q->dg[1][2 + lane];
    const double q_v = v * v, q_vL = vL * vL, q_vR = vR * vR, q_hn = hn * hn, q_hnL = hnL * hnL, q_hs1 = hs1 * hs1, q_hsL1 = hsL1 * hsL1;
    const double q_se = se * se, q_sw = sw * sw, q_seL = seL * seL, q_swR = swR * swR;
    const double n0 = q_hn + q_vR, n1 = q_v + q_hs1, n2 = q_v + q_hsL1, n3 = q_hnL + q_vL;     // s1^2 + s2^2 of the facets below
    const double n4 = q_hsL1 + q_vL, n5 = q_v + q_hnL, n6 = q_v + q_hn, n7 = q_hs1 + q_vR;
    // facets: s1, s2, sd                                     4: s1 = -hsL1  s2 = vL    sd = sw
    //   0: s1 = hn    s2 = -vR    sd = -swR                  5: s1 = v      s2 = -hnL  sd = sw
    //   1: s1 = -v    s2 = hs1    sd = -swR                  6: s1 = v      s2 = hn    sd = se
    //   2: s1 = -v    s2 = -hsL1  sd = -seL                  7: s1 = hs1    s2 = vR    sd = se
    //   3: s1 = -hnL  s2 = -vL    sd = -seL      (0-3: cell (b+1, j), 4-7: cell (b, j))
    // sign tests and cross products (r > theta as s2*d1 > s1*d2; d1, d2 = dX, dY for facets 0,3,4,7, dY, dX for the others);
    // a test on a neighbour's quotient is that lane's own test, shifted
    const lmask Pv = LM(v > 0), Nv = LM(v < 0), Phn = LM(hn > 0), Nhn = LM(hn < 0);
    const double p_v = v * ts.dX, p_vL = vL * ts.dX, p_vR = vR * ts.dX, p_hn = hn * ts.dY, p_hnL = hnL * ts.dY;
    const double p_hs = hs1 * ts.dY, p_hsL = hsL1 * ts.dY;
#define STATES(k, ak, bk, gk, dk)                                                                         \
    const lmask both##k = (ak) & (bk), g##k = gk;                                                          \
    const lmask in##k = both##k & ~g##k;                               /* interior: r = atan2(s2, s1) */    \
    const lmask dg##k = (both##k & g##k) | (~(ak) & (bk) & (dk));      /* I1: r = theta, mag = sd; I3: only when sd > 0 */ \
    const lmask cd##k = (ak) & ~(bk);                                  /* I2: r = 0, mag = s1 */

    // ================= south half of row b, then the whole cell =================
    double M;
    lmask tAn, tBn, tAs, tBs, k0, k1, k2, flat, wint;
    if (__builtin_expect(!exact, 1)) {
        const lmask dSW = LM(sw > 0), dSE = LM(se > 0);
        STATES(4, from_left(Nhs1), from_left(Pv), LM(p_vL > -p_hsL), dSW)
        STATES(5, Pv, from_left(Nhn), LM(-p_hnL > p_v), dSW)
        STATES(6, Pv, Phn, LM(p_hn > p_v), dSE)
        STATES(7, Phs1, from_right(Pv), LM(p_vR > p_hs), dSE)
        // candidates that are not in play are made negative in place; after that an equality with the maximum needs no
        // second look at the state (a lane where nothing is in play may see a false match: it is `flat` and stores -1)
        const double kn4 = only_if(in4, n4, dead_hi), kn5 = only_if(in5, n5, dead_hi), kn6 = only_if(in6, n6, dead_hi), kn7 = only_if(in7, n7, dead_hi);
        const double kc4 = only_if(cd4, q_hsL1, dead_hi), kcS = only_if(cd5 | cd6, q_v, dead_hi), kc7 = only_if(cd7, q_hs1, dead_hi);
        const double kdSW = only_if(dg4 | dg5, q_sw, dead_hi), kdSE = only_if(dg6 | dg7, q_se, dead_hi);
        const double Ms = vmax(vmax(vmax(vmax(-1.0, kn4), vmax(kn5, kn6)), vmax(vmax(kn7, kc4), vmax(kcS, kc7))), vmax(kdSW, kdSE));
        const lmask eSW = LM(kdSW == Ms), eSE = LM(kdSE == Ms), ecS = LM(kcS == Ms);
        const lmask h4 = LM(kn4 == Ms) | LM(kc4 == Ms) | (dg4 & eSW);
        const lmask h5 = LM(kn5 == Ms) | (cd5 & ecS) | (dg5 & eSW);
        const lmask h6 = LM(kn6 == Ms) | (cd6 & ecS) | (dg6 & eSE);
        const lmask h7 = LM(kn7 == Ms) | LM(kc7 == Ms) | (dg7 & eSE);
        M = vmax(c.Mn, Ms);
        const lmask north = LM(c.Mn >= Ms);                   // facets 0-3 come first: they keep a tie
        flat = LM(M < 0);                                     // no facet descends: mag = -1 (:1983-1984)
        const lmask s4 = h4 & ~north, s5 = h5 & ~(north | h4), s6 = h6 & ~(north | h4 | h5), s7 = h7 & ~(north | h4 | h5 | h6);
        wint = (north & c.Nint) | (s4 & in4) | (s5 & in5) | (s6 & in6) | (s7 & in7);
        tAn = north & c.NdA; tBn = north & c.NdB; tAs = (s4 & dg4) | (s7 & dg7); tBs = (s5 & dg5) | (s6 & dg6);
        k0 = (north & c.Nk0) | s5 | s7; k1 = (north & c.Nk1) | s6 | s7; k2 = s4 | s5 | s6 | s7;
    } else {
        // exact path (NaN or huge elevations in the band): every comparison is made on the slopes themselves, facet after
        // facet in the reference's order, starting from the carried north half
        const double s1_4 = -hsL1, s2_4 = vL, s1_5 = v, s2_5 = -hnL, s2_6 = hn, s1_7 = hs1, s2_7 = vR;
        Acc acc; acc.rad2 = c.Mn; acc.code = -8;
        facet_lean(s1_4, s2_4, sw, q_hsL1, q_vL, q_sw, ts.dX, ts.dY, 4, acc);
        facet_lean(s1_5, s2_5, sw, q_v, q_hnL, q_sw, ts.dY, ts.dX, 5, acc);
        facet_lean(s1_5, s2_6, se, q_v, q_hn, q_se, ts.dY, ts.dX, 6, acc);
        facet_lean(s1_7, s2_7, se, q_hs1, q_vR, q_se, ts.dX, ts.dY, 7, acc);
        M = acc.rad2;
        flat = LM(acc.rad2 == -1.0);
        const int k = acc.code >> 2, kind = acc.code & 3;
        const bool south = acc.code >= 0, sin = south && kind == 3, sdg = south && kind == 2;
        const lmask sm = LM(south);
        wint = LM(sin) | (~sm & c.Nint);
        tAn = ~sm & c.NdA; tBn = ~sm & c.NdB; tAs = LM(sdg && (k == 4 || k == 7)); tBs = LM(sdg && (k == 5 || k == 6));
        k0 = (~sm & c.Nk0) | LM(south && (k & 1)); k1 = (~sm & c.Nk1) | LM(south && (k & 2)); k2 = sm;
    }
    if (cx.writes && b >= cx.i0) {
        // direction of the winner: r * ang[1] + ang[0] * pi / 2 (:1989).  r = atan2(s2, s1) for an interior winner (both
        // slopes positive there, so the un-negated quotients serve: |x|); every other lane runs the arctangent on (0, 1),
        // which is exactly 0 -- the r of a cardinal winner -- and a diagonal winner takes its table angle
        const int k = (ON(k0) ? 1 : 0) | (ON(k1) ? 2 : 0) | (ON(k2) ? 4 : 0);
        const uint16_t *te = cx.tab + (P * 9 + (ON(wint) ? k : 8)) * 2;
        const char *lb = reinterpret_cast<const char *>(&cx.q->a[0][0][lane]);
        const double w1 = *reinterpret_cast<const double *>(lb + te[0]), w2 = *reinterpret_cast<const double *>(lb + te[1]);
        double r = atan2_pos_fast(fabs(w2), fabs(w1), cx.atan_16);
        // An interior winner whose cross products are EQUAL (s2 * d1 == s1 * d2: `r > theta` is false, the facet is not clamped,
        // :1973) has r == theta exactly: the reference's arctangent of two slopes in the exact ratio of the spacings IS the table
        // angle, the arctangent above may be an ulp off -- and an ulp across a section boundary is another section (soak case
        // 900039: an int32 DEM with dX = 1, dY = 17).  The test is made on the winner alone (facets 0, 3, 4, 7: d1, d2 = dX, dY,
        // the others dY, dX; spacings of the band the winner was decided in), the angle is the table angle of that facet.
        {
            const double2 dn = *reinterpret_cast<const double2 *>(cx.rtv + (b - 1 - cx.r0 > 0 ? b - 1 - cx.r0 : 0) * 8);     // dX, dY of the band above
            const double dXw = pick(k2, ts.dX, dn.x), dYw = pick(k2, ts.dY, dn.y);
            const double a1 = fabs(w1), a2 = fabs(w2);
            const lmask famA = ~(k0 ^ k1);
            const lmask tie = wint & ((famA & LM(a2 * dXw == a1 * dYw)) | (~famA & LM(a2 * dYw == a1 * dXw)));
            tAn |= ~k2 & famA & tie; tBn |= ~k2 & ~famA & tie; tAs |= k2 & famA & tie; tBs |= k2 & ~famA & tie;
        }
        r = pick(tAn, c.thAn, r); r = pick(tBn, c.thBn, r); r = pick(tAs, thAs, r); r = pick(tBs, thBs, r);
        const double rs = __hiloint2double(__double2hiint(r) ^ (int)((unsigned)k << 31), __double2loint(r));   // ang[1] = -1 for odd facets
        const double direction = rs + (double)((k + 1) >> 1) * (PI_D / 2);
        const size_t cc = (size_t)b * m + cx.j;
#ifdef PYDEM_STENCIL_NOSTORE            // timing experiment: the arithmetic without its stores
        if (M == 1.2345e300) { cx.mag[cc] = direction; cx.dir[cc] = r; cx.flat0[cc] = ON(flat) ? 1 : 0; }
        if (false) {
#else
        {
#endif
#ifdef PYDEM_STENCIL_CHEAP
        cx.mag[cc] = M > 0 ? M * __builtin_amdgcn_rsq(M) : M;
#else
        if (SPLIT) {
            StoreRing &R = *cx.ring;
            const int slot = (b - cx.i0) & (SR_ROWS - 1);
            R.mag[slot][lane] = mag_of(M);
            R.dir[slot][lane] = pick(flat, -1.0, direction);
            R.flat[slot][lane] = ON(flat) ? 1 : 0;
        } else {
        cx.mag[cc] = mag_of(M);                                        // :1901
#endif
        cx.dir[cc] = pick(flat, -1.0, direction);
        cx.flat0[cc] = ON(flat) ? 1 : 0;
#ifndef PYDEM_STENCIL_CHEAP
        }
#endif
        }
    }
    if (SPLIT && b >= cx.i0) {
        // the row is in the ring: tell the store wavefront (LDS operations of a wavefront execute in order; the fence is for the
        // compiler), then make sure the slot of the row after the next SR_ROWS - 1 is free before anybody writes it
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) __atomic_store_n(&cx.ring->prod, b - cx.i0 + 1, __ATOMIC_RELAXED);
        const int need = b - cx.i0 + 2 - SR_ROWS;                       // rows that must have left before row b + 1 is written
        if (need > 0) while (__atomic_load_n(&cx.ring->cons, __ATOMIC_RELAXED) < need) __builtin_amdgcn_s_sleep(1);
    }
    // ================= north half of row b+1 =================
    if (__builtin_expect(!exact, 1)) {
        const lmask dNE = from_right(LM(sw < 0)), dNW = from_left(LM(se < 0));
        STATES(0, Phn, from_right(Nv), LM(-p_vR > p_hn), dNE)
        STATES(1, Nv, Phs1, LM(p_hs > -p_v), dNE)
        STATES(2, Nv, from_left(Nhs1), LM(-p_hsL > -p_v), dNW)
        STATES(3, from_left(Nhn), from_left(Nv), LM(-p_vL > -p_hnL), dNW)
        const double kn0 = only_if(in0, n0, dead_hi), kn1 = only_if(in1, n1, dead_hi), kn2 = only_if(in2, n2, dead_hi), kn3 = only_if(in3, n3, dead_hi);
        const double kc0 = only_if(cd0, q_hn, dead_hi), kcN = only_if(cd1 | cd2, q_v, dead_hi), kc3 = only_if(cd3, q_hnL, dead_hi);
        const double kdNE = only_if(dg0 | dg1, q_swR, dead_hi), kdNW = only_if(dg2 | dg3, q_seL, dead_hi);
        const double Mq = vmax(vmax(vmax(vmax(-1.0, kn0), vmax(kn1, kn2)), vmax(vmax(kn3, kc0), vmax(kcN, kc3))), vmax(kdNE, kdNW));
        const lmask eNE = LM(kdNE == Mq), eNW = LM(kdNW == Mq), ecN = LM(kcN == Mq);
        const lmask h0 = LM(kn0 == Mq) | LM(kc0 == Mq) | (dg0 & eNE);
        const lmask h1 = LM(kn1 == Mq) | (cd1 & ecN) | (dg1 & eNE);
        const lmask h2 = LM(kn2 == Mq) | (cd2 & ecN) | (dg2 & eNW);
        const lmask h3 = LM(kn3 == Mq) | LM(kc3 == Mq) | (dg3 & eNW);
        const lmask f0 = h0, f1 = h1 & ~h0, f2 = h2 & ~(h0 | h1), f3 = h3 & ~(h0 | h1 | h2);
        c.Mn = Mq;
        c.Nint = (f0 & in0) | (f1 & in1) | (f2 & in2) | (f3 & in3);
        c.Nk0 = f1 | f3; c.Nk1 = f2 | f3; c.NdA = (f0 & dg0) | (f3 & dg3); c.NdB = (f1 & dg1) | (f2 & dg2);
    } else {
        const double s1_0 = hn, s2_0 = -vR, s1_1 = -v, s2_1 = hs1, s2_2 = -hsL1, s1_3 = -hnL, s2_3 = -vL;
        Acc an; an.rad2 = -1.0; an.code = -4;
        facet_lean(s1_0, s2_0, -swR, q_hn, q_vR, q_swR, ts.dX, ts.dY, 0, an);
        facet_lean(s1_1, s2_1, -swR, q_v, q_hs1, q_swR, ts.dY, ts.dX, 1, an);
        facet_lean(s1_1, s2_2, -seL, q_v, q_hsL1, q_seL, ts.dY, ts.dX, 2, an);
        facet_lean(s1_3, s2_3, -seL, q_hnL, q_vL, q_seL, ts.dX, ts.dY, 3, an);
        const int k = an.code >> 2, kind = an.code & 3;       // k = -1, kind = 0: no north facet descends
        const bool nin = kind == 3, ndg = kind == 2;
        c.Mn = an.rad2;
        c.Nint = LM(nin);
        c.Nk0 = LM(k >= 0 && (k & 1)); c.Nk1 = LM(k >= 0 && (k & 2));
        c.NdA = LM(ndg && (k == 0 || k == 3)); c.NdB = LM(ndg && (k == 1 || k == 2));
    }
#undef STATES
    // ---- the E-edge of row b+1 over its own south spacing opens the next band
    const double hs = (b + 1 <= n - 2) ? div_row(dE, tnx.dX, tnx.rdX) : 0.0;
    c.z0 = zS; c.ex_top = cx.exact_only || ex_bot;
    cx.q->a[1 - P][1][1 + lane] = hs;
    lanes_published();
    c.hs1 = hs; c.hsL1 = cx.q->a[1 - P][1][lane]; c.Phs1 = LM(hs > 0); c.Nhs1 = LM(hs < 0);
    c.thAn = thAs; c.thBn = thBs;
    row_arrived<(FIRST || SPLIT) ? 0 : 3>(z_ahead);
}

// OCC = workgroups the compiler must fit on a CU: 1 = free choice (135 VGPRs: three wavefronts per SIMD), 4 = at most 128
// VGPRs for a fourth wavefront per SIMD (PYDEM_STENCIL_OCC=4; measured, DESIGN.md section 4 "Round 4")
template <bool F32, int OCC>
__global__ __launch_bounds__(256, OCC) void k_stencil_march(const double *__restrict__ elev, int n, int m,
                                                       const RowTab *__restrict__ rowtab,
                                                       double *__restrict__ mag, double *__restrict__ dir,
                                                       uint8_t *__restrict__ flat0, int strips, int chunks, int rows_per_wave,
                                                       int exact_only)
{
    // the arctangent table sits in LDS: a global (vmcnt) load in the loop body would make every row wait for the
    // stores of the row before it as well
    __shared__ double s_atan[17];
    __shared__ WaveQ s_q[4];
    __shared__ uint16_t s_tab[2 * 9 * 2];
    __shared__ double s_rt[(MARCH_ROWS + 2) * 8];
    if (threadIdx.x < 17) s_atan[threadIdx.x] = ATAN_16[threadIdx.x];
    if (threadIdx.x < 36) {
        // facet k: (array, lane offset) of s1 and s2 -- 0: hn(0) v(+1)  1: v(0) hs1(0)  2: v(0) hs1(-1)  3: hn(-1) v(-1)
        //                                               4: hs1(-1) v(-1)  5: v(0) hn(-1)  6: v(0) hn(0)  7: hs1(0) v(+1)
        // facets 0-3 were decided in the band before the running one (the other parity), 4-7 in the running band
        const int par = threadIdx.x / 18, k = (threadIdx.x % 18) / 2, which = threadIdx.x & 1;
        const int arr1[8] = {0, 2, 2, 0, 1, 2, 2, 1}, dl1[8] = {0, 0, 0, -1, -1, 0, 0, 0};
        const int arr2[8] = {2, 1, 1, 2, 2, 0, 0, 2}, dl2[8] = {1, 0, -1, -1, -1, -1, 0, 1};
        int off;
        if (k == 8) off = (6 * QS + (which ? QS : 0) + 1) * 8;
        else {
            const int band = k < 4 ? 1 - par : par;
            off = ((band * 3 + (which ? arr2[k] : arr1[k])) * QS + 1 + (which ? dl2[k] : dl1[k])) * 8;
        }
        s_tab[threadIdx.x] = (uint16_t)off;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // the four wavefronts of a workgroup march four neighbouring strips of ONE chunk of rows (strips4 = the strips padded to
    // a multiple of four), so that they share the chunk's row table
    const int strips4 = (strips + 3) & ~3;
    const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));   // wavefront id (scalar)
    const int chunk = wid / strips4, strip = wid - chunk * strips4;  // consecutive waves walk along a row band
    const int i0 = 1 + chunk * rows_per_wave;                       // first output row
    const int i1 = (i0 + rows_per_wave < n - 1) ? i0 + rows_per_wave : n - 1;   // one past the last output row
    {
        const int r_last = i1 < n - 2 ? i1 : n - 2;                 // table rows i0-1 .. r_last
        const double2 *src = reinterpret_cast<const double2 *>(rowtab + (i0 - 1));
        double2 *dst = reinterpret_cast<double2 *>(s_rt);
        const int n16 = (r_last - (i0 - 1) + 1) * 4;
        if (chunk < chunks) for (int q = threadIdx.x; q < n16; q += 256) dst[q] = src[q];
    }
    __syncthreads();
    if (chunk >= chunks || strip >= strips) return;
    const int j = strip * 62 + lane;                                // this lane's column (lane 0 / 63 = halo)
    MarchCtx cx;
    cx.col = elev + ((j < m) ? j : m - 1); cx.rowtab = rowtab; cx.rtv = s_rt; cx.r0 = i0 - 1;
    cx.atan_16 = s_atan; cx.mag = mag; cx.dir = dir; cx.flat0 = flat0;
    cx.q = &s_q[threadIdx.x >> 6]; cx.tab = s_tab;
    cx.q->one[1 + lane] = 1.0; cx.q->zero[1 + lane] = 0.0;
    cx.n = n; cx.m = m; cx.j = j; cx.i0 = i0; cx.exact_only = exact_only;
    cx.writes = lane >= 1 && lane <= 62 && j >= 1 && j < m - 1;

    // ---- the top row of the first band (row i0-1: not an output row of this wavefront, its north half is never used)
    BandCarry c;
    RowV ts = rowv_load(cx.rtv, 0), tu;
    c.z0 = cx.col[(size_t)(i0 - 1) * m];
    c.ex_top = exact_only || LM(!(fabs(c.z0) < 0x1p500)) != 0;
    c.hs1 = div_row(zsub<F32>(c.z0, lane_next(c.z0)), ts.dX, ts.rdX);
    c.hsL1 = lane_prev(c.hs1);
    c.Phs1 = LM(c.hs1 > 0); c.Nhs1 = LM(c.hs1 < 0);
    cx.q->a[0][1][1 + lane] = c.hs1;
    c.Mn = -1.0; c.thAn = 0.0; c.thBn = 0.0;
    c.Nk0 = 0; c.Nk1 = 0; c.NdA = 0; c.NdB = 0; c.Nint = 0;
    double zP = cx.col[(size_t)i0 * m], zQ = 0.0;                  // the bottom row of a band alternates between zP and zQ
    int b = i0 - 1;
    march_band<F32, 0, true>(cx, c, ts, tu, b, zP, zQ);             // (row i0 - 1 is not an output row: no stores)
    for (b++; b + 1 < i1; b += 2) {
        march_band<F32, 1>(cx, c, tu, ts, b, zQ, zP);
        march_band<F32, 0>(cx, c, ts, tu, b + 1, zP, zQ);
    }
    if (b < i1) march_band<F32, 1>(cx, c, tu, ts, b, zQ, zP);
}

// Producer / store split (see StoreRing): NCW compute wavefronts + one store wavefront per workgroup = twelve wavefronts, the CU's
// whole allowance at the kernel's 135 VGPRs (three per SIMD) -- eleven compute wavefronts per CU instead of twelve.  LDS is carved
// from the dynamic allocation (114 KB: above the 64 KB a static allocation may take).
#ifndef PYDEM_SPLIT_NCW
#define PYDEM_SPLIT_NCW 11
#endif
constexpr int SPLIT_NCW = PYDEM_SPLIT_NCW;
struct SplitLds {
    double atan16[18];
    double rt[(MARCH_ROWS + 2) * 8];
    WaveQ q[SPLIT_NCW];
    StoreRing ring[SPLIT_NCW];
    uint16_t tab[2 * 9 * 2 + 4];
};

template <bool F32>
__global__ __launch_bounds__(64 * (SPLIT_NCW + 1), 1) void k_stencil_march_split(const double *__restrict__ elev, int n, int m,
                                                       const RowTab *__restrict__ rowtab,
                                                       double *__restrict__ mag, double *__restrict__ dir,
                                                       uint8_t *__restrict__ flat0, int strips, int chunks, int rows_per_wave,
                                                       int exact_only)
{
    extern __shared__ __align__(16) char dyn_lds[];
    SplitLds &L = *reinterpret_cast<SplitLds *>(dyn_lds);
    if (threadIdx.x < 17) L.atan16[threadIdx.x] = ATAN_16[threadIdx.x];
    if (threadIdx.x < 36) {
        const int par = threadIdx.x / 18, k = (threadIdx.x % 18) / 2, which = threadIdx.x & 1;
        const int arr1[8] = {0, 2, 2, 0, 1, 2, 2, 1}, dl1[8] = {0, 0, 0, -1, -1, 0, 0, 0};
        const int arr2[8] = {2, 1, 1, 2, 2, 0, 0, 2}, dl2[8] = {1, 0, -1, -1, -1, -1, 0, 1};
        int off;
        if (k == 8) off = (6 * QS + (which ? QS : 0) + 1) * 8;
        else {
            const int band = k < 4 ? 1 - par : par;
            off = ((band * 3 + (which ? arr2[k] : arr1[k])) * QS + 1 + (which ? dl2[k] : dl1[k])) * 8;
        }
        L.tab[threadIdx.x] = (uint16_t)off;
    }
    if (threadIdx.x < SPLIT_NCW) { L.ring[threadIdx.x].prod = 0; L.ring[threadIdx.x].cons = 0; }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int groups = (strips + SPLIT_NCW - 1) / SPLIT_NCW;           // workgroups per chunk of rows
    const int chunk = blockIdx.x / groups, strip0 = (blockIdx.x - chunk * groups) * SPLIT_NCW;
    const int i0 = 1 + chunk * rows_per_wave;
    const int i1 = (i0 + rows_per_wave < n - 1) ? i0 + rows_per_wave : n - 1;
    {
        const int r_last = i1 < n - 2 ? i1 : n - 2;
        const double2 *src = reinterpret_cast<const double2 *>(rowtab + (i0 - 1));
        double2 *dst = reinterpret_cast<double2 *>(L.rt);
        const int n16 = (r_last - (i0 - 1) + 1) * 4;
        if (chunk < chunks) for (int q = threadIdx.x; q < n16; q += blockDim.x) dst[q] = src[q];
    }
    __syncthreads();
    if (chunk >= chunks) return;
    if (wave == SPLIT_NCW) {
        // ---- the store wavefront: drain the producers' rings row by row
        const int rows = i1 - i0;
        int c[SPLIT_NCW];
        unsigned wmask = 0;
        int left = 0;
#pragma unroll
        for (int w = 0; w < SPLIT_NCW; w++) {
            c[w] = 0;
            const int strip = strip0 + w, j = strip * 62 + lane;
            const bool live = strip < strips;
            if (live) left += rows;
            if (live && lane >= 1 && lane <= 62 && j >= 1 && j < m - 1) wmask |= 1u << w;
        }
        while (left > 0) {
            bool progress = false;
#pragma unroll
            for (int w = 0; w < SPLIT_NCW; w++) {
                if (strip0 + w >= strips) continue;
                const int p = __atomic_load_n(&L.ring[w].prod, __ATOMIC_RELAXED);
                if (c[w] >= p) continue;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                while (c[w] < p) {
                    const int slot = c[w] & (SR_ROWS - 1);
                    const double mv = L.ring[w].mag[slot][lane], dv = L.ring[w].dir[slot][lane];
                    const uint8_t fv = L.ring[w].flat[slot][lane];
                    if ((wmask >> w) & 1u) {
                        const size_t cc = (size_t)(i0 + c[w]) * m + ((strip0 + w) * 62 + lane);
                        mag[cc] = mv; dir[cc] = dv; flat0[cc] = fv;
                    }
                    c[w]++; left--;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) __atomic_store_n(&L.ring[w].cons, c[w], __ATOMIC_RELAXED);
                progress = true;
            }
            if (!progress) __builtin_amdgcn_s_sleep(2);
        }
        return;
    }
    const int strip = strip0 + wave;
    if (strip >= strips) return;
    const int j = strip * 62 + lane;
    MarchCtx cx;
    cx.ring = &L.ring[wave];
    cx.col = elev + ((j < m) ? j : m - 1); cx.rowtab = rowtab; cx.rtv = L.rt; cx.r0 = i0 - 1;
    cx.atan_16 = L.atan16; cx.mag = mag; cx.dir = dir; cx.flat0 = flat0;
    cx.q = &L.q[wave]; cx.tab = L.tab;
    cx.q->one[1 + lane] = 1.0; cx.q->zero[1 + lane] = 0.0;
    cx.n = n; cx.m = m; cx.j = j; cx.i0 = i0; cx.exact_only = exact_only;
    cx.writes = lane >= 1 && lane <= 62 && j >= 1 && j < m - 1;
    BandCarry c;
    RowV ts = rowv_load(cx.rtv, 0), tu;
    c.z0 = cx.col[(size_t)(i0 - 1) * m];
    c.ex_top = exact_only || LM(!(fabs(c.z0) < 0x1p500)) != 0;
    c.hs1 = div_row(zsub<F32>(c.z0, lane_next(c.z0)), ts.dX, ts.rdX);
    c.hsL1 = lane_prev(c.hs1);
    c.Phs1 = LM(c.hs1 > 0); c.Nhs1 = LM(c.hs1 < 0);
    cx.q->a[0][1][1 + lane] = c.hs1;
    c.Mn = -1.0; c.thAn = 0.0; c.thBn = 0.0;
    c.Nk0 = 0; c.Nk1 = 0; c.NdA = 0; c.NdB = 0; c.Nint = 0;
    double zP = cx.col[(size_t)i0 * m], zQ = 0.0;
    int b = i0 - 1;
    march_band<F32, 0, true, true>(cx, c, ts, tu, b, zP, zQ);
    for (b++; b + 1 < i1; b += 2) {
        march_band<F32, 1, false, true>(cx, c, tu, ts, b, zQ, zP);
        march_band<F32, 0, false, true>(cx, c, ts, tu, b + 1, zP, zQ);
    }
    if (b < i1) march_band<F32, 1, false, true>(cx, c, tu, ts, b, zQ, zP);
}

// ---------------------------------------------------------------------------------------------
// perimeter kernel: one thread per edge/corner cell (dem_processing.py:1779-1899).
// ---------------------------------------------------------------------------------------------
template <bool F32>
__device__ void interior_cell(const double *elev, int n, int m, const RowTab *rowtab, int i, int j,
                              double &rad2, double &d)
{
    // pre-sqrt magnitude and direction of interior cell (i, j) recomputed from global memory;
    // cells that are not interior still hold the initial -1 at the time of the copy rules
    rad2 = -1.0; d = -1.0;
    if (i < 1 || i > n - 2 || j < 1 || j > m - 2) return;
    const double *r0 = elev + (size_t)(i - 1) * m + j, *r1 = r0 + m, *r2 = r1 + m;
    Best b = best_init();
    eight_facets<F32>(r1[0], r0[0], r2[0], r1[1], r1[-1], r0[1], r0[-1], r2[-1], r2[1], rowtab[i - 1], rowtab[i], b);
    rad2 = b.rad2; d = winner_direction(b);
}

// one facet of an edge cell; mode 0: per-row spacing (left/right edges, topbot == None),
// mode 1: fixed spacing row `sr` ('top' -> 0, 'bot' -> n-2) (:1925-1934)
template <bool F32>
__device__ void edge_facet(const double *elev, int n, int m, const RowTab *rowtab, int i, int j, int k,
                           int mode, int sr, Best &b)
{
    int r;
    if (mode == 1) r = sr;
    else r = (k <= 3) ? i - 1 : i;   // facets 0-3 reference spacing row i-1, 4-7 row i (:1914-1921)
    const RowTab t = rowtab[r];
    const bool A = (k == 0 || k == 3 || k == 4 || k == 7);
    const double d1 = A ? t.dX : t.dY, d2 = A ? t.dY : t.dX, th = A ? t.thA : t.thB;
    const double z0 = elev[(size_t)i * m + j];
    const double z1 = elev[(size_t)(i + fe1r(k)) * m + (j + fe1c(k))];
    const double z2 = elev[(size_t)(i + fe2r(k)) * m + (j + fe2c(k))];
    facet(zsub<F32>(z0, z1) / d1, zsub<F32>(z1, z2) / d2, zsub<F32>(z0, z2) / t.hyp, d1, d2, th, k, b);
}

template <bool F32>
__global__ void k_stencil_perimeter(const double *__restrict__ elev, int n, int m,
                                    const RowTab *__restrict__ rowtab,
                                    double *__restrict__ mag, double *__restrict__ dir, uint8_t *__restrict__ flat0)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nper = 2 * (int64_t)m + 2 * (int64_t)(n - 2);
    if (p >= nper) return;
    int i, j;
    if (p < m) { i = 0; j = (int)p; }
    else if (p < 2 * (int64_t)m) { i = n - 1; j = (int)(p - m); }
    else if (p < 2 * (int64_t)m + (n - 2)) { i = (int)(p - 2 * (int64_t)m) + 1; j = 0; }
    else { i = (int)(p - 2 * (int64_t)m - (n - 2)) + 1; j = m - 1; }

    const double HP = PI_D / 2, P32 = 3 * PI_D / 2, TWOPI = 2 * PI_D;
    double rad2 = -1.0, d = -1.0;
    // --- copy-from-interior rules in the reference's order: left, right, top, bottom (:1782-1795).
    // For a corner the value can arrive through two hops (side copy on row 1 / n-2, then the
    // top / bottom copy).
    const bool top = (i == 0), bot = (i == n - 1), left = (j == 0), right = (j == m - 1);
    if ((left || right) && !top && !bot) {
        double r2, dd;
        interior_cell<F32>(elev, n, m, rowtab, i, left ? 1 : m - 2, r2, dd);
        const bool take = left ? (dd > HP && dd < P32) : (dd < HP || dd > P32);
        if (take) { rad2 = r2; d = dd; }
    } else {
        // row 0 copies from row 1, row n-1 from row n-2; on the corner columns row 1 / n-2 itself
        // holds whatever the side copy put there
        const int ii = top ? 1 : n - 2;
        double r2 = -1.0, dd = -1.0;
        if (left || right) {
            double r3, d3;
            interior_cell<F32>(elev, n, m, rowtab, ii, left ? 1 : m - 2, r3, d3);
            const bool take1 = left ? (d3 > HP && d3 < P32) : (d3 < HP || d3 > P32);
            if (take1) { r2 = r3; dd = d3; }
        } else {
            interior_cell<F32>(elev, n, m, rowtab, ii, j, r2, dd);
        }
        const bool take = top ? (dd > 0 && dd < PI_D) : (dd > PI_D && dd < TWOPI);
        if (take) { rad2 = r2; d = dd; }
    }
    // --- inward facets (:1800-1899); the copied value competes through the same strict '>'
    Best b = best_init();
    b.rad2 = rad2;
    int copied = (rad2 > -1.0) || (d != -1.0);
    (void)copied;
    const int sr = top ? 0 : n - 2;
    if (top && left) { edge_facet<F32>(elev, n, m, rowtab, i, j, 6, 1, sr, b); edge_facet<F32>(elev, n, m, rowtab, i, j, 7, 1, sr, b); }
    else if (top && right) { edge_facet<F32>(elev, n, m, rowtab, i, j, 4, 1, sr, b); edge_facet<F32>(elev, n, m, rowtab, i, j, 5, 1, sr, b); }
    else if (bot && left) { edge_facet<F32>(elev, n, m, rowtab, i, j, 0, 1, sr, b); edge_facet<F32>(elev, n, m, rowtab, i, j, 1, 1, sr, b); }
    else if (bot && right) { edge_facet<F32>(elev, n, m, rowtab, i, j, 2, 1, sr, b); edge_facet<F32>(elev, n, m, rowtab, i, j, 3, 1, sr, b); }
    else if (left) { const int ks[4] = {0, 1, 6, 7}; for (int q = 0; q < 4; q++) edge_facet<F32>(elev, n, m, rowtab, i, j, ks[q], 0, 0, b); }
    else if (right) { const int ks[4] = {2, 3, 4, 5}; for (int q = 0; q < 4; q++) edge_facet<F32>(elev, n, m, rowtab, i, j, ks[q], 0, 0, b); }
    else if (top) { const int ks[4] = {4, 5, 6, 7}; for (int q = 0; q < 4; q++) edge_facet<F32>(elev, n, m, rowtab, i, j, ks[q], 1, sr, b); }
    else { const int ks[4] = {0, 1, 2, 3}; for (int q = 0; q < 4; q++) edge_facet<F32>(elev, n, m, rowtab, i, j, ks[q], 1, sr, b); }
    const double dout = (b.k >= 0) ? winner_direction(b) : d;   // no facet beat the copied value
    const size_t c = (size_t)i * m + j;
    mag[c] = b.rad2 > 0 ? sqrt(b.rad2) : b.rad2;
    dir[c] = dout;
    flat0[c] = (b.rad2 == -1.0);
}

template <bool SW>
int launch_interior(pydem_tile *t)
{
    const int tiles_x = (int)cdiv(t->m, TX), tiles_y = (int)cdiv(t->n, TY);
    const int total = tiles_x * tiles_y;
    const int grid = SW ? ((total + 7) / 8) * 8 : total;
    if (t->elev_f32)
        hipLaunchKernelGGL((k_stencil_interior<SW, true>), dim3(grid), dim3(256), 0, t->stream, t->elev, (int)t->n, (int)t->m,
                           t->rowtab, t->mag, t->dir, t->flat0, tiles_x, total);
    else
        hipLaunchKernelGGL((k_stencil_interior<SW, false>), dim3(grid), dim3(256), 0, t->stream, t->elev, (int)t->n, (int)t->m,
                           t->rowtab, t->mag, t->dir, t->flat0, tiles_x, total);
    return 0;
}

}  // namespace

static int stencil_variant()
{
    static int v = -1;
    if (v < 0) { const char *e = getenv("PYDEM_STENCIL"); v = (e && !strcmp(e, "tile")) ? 1 : 2; }
    return v;
}

static void launch_stencil(pydem_tile *t)
{
    if (stencil_variant() == 1) { launch_interior<true>(t); return; }
    const int strips = (int)cdiv(t->m - 2, 62);
    int rows = MARCH_ROWS;            // every chunk re-reads two halo rows: long chunks on big tiles, enough wavefronts on small ones
    while (rows > 16 && (int64_t)strips * cdiv(t->n - 2, rows) < 12288) rows >>= 1;
    const int chunks = (int)cdiv(t->n - 2, rows);
    const int waves = ((strips + 3) & ~3) * chunks;
    const int exact_only = t->stencil_exact_only;   // set with the row tables: a spacing outside [2^-500, 2^500] (or PYDEM_STENCIL_EXACT=1)
    // PYDEM_STENCIL_SPLIT=1 (read per launch: the tests switch it): the producer / store split, a round-6 experiment that LOSES
    // (3.58 against 2.77 ms back to back, profiles/r06_stencil_split_ab.txt) and is kept as such, never the default
    int split = 0;
    { const char *e = getenv("PYDEM_STENCIL_SPLIT"); split = e ? atoi(e) : 0; }
    if (split) {
        static int attr_ok = -1;
        if (attr_ok < 0)
            attr_ok = hipFuncSetAttribute((const void *)k_stencil_march_split<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SplitLds)) == hipSuccess &&
                      hipFuncSetAttribute((const void *)k_stencil_march_split<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SplitLds)) == hipSuccess;
        if (!attr_ok) { (void)hipGetLastError(); split = 0; }
    }
    if (split) {
        const int groups = (strips + SPLIT_NCW - 1) / SPLIT_NCW;
        if (t->elev_f32)
            hipLaunchKernelGGL((k_stencil_march_split<true>), dim3((unsigned)(groups * chunks)), dim3(64 * (SPLIT_NCW + 1)), sizeof(SplitLds), t->stream, t->elev,
                               (int)t->n, (int)t->m, t->rowtab, t->mag, t->dir, t->flat0, strips, chunks, rows, exact_only);
        else
            hipLaunchKernelGGL((k_stencil_march_split<false>), dim3((unsigned)(groups * chunks)), dim3(64 * (SPLIT_NCW + 1)), sizeof(SplitLds), t->stream, t->elev,
                               (int)t->n, (int)t->m, t->rowtab, t->mag, t->dir, t->flat0, strips, chunks, rows, exact_only);
        return;
    }
    static int occ = -1;
    if (occ < 0) { const char *e = getenv("PYDEM_STENCIL_OCC"); occ = (e && atoi(e) == 4) ? 4 : 1; }
#define MARCH(F32, OCC) hipLaunchKernelGGL((k_stencil_march<F32, OCC>), dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, t->stream, t->elev, \
                                           (int)t->n, (int)t->m, t->rowtab, t->mag, t->dir, t->flat0, strips, chunks, rows, exact_only)
    if (t->elev_f32) { if (occ == 4) MARCH(true, 4); else MARCH(true, 1); }
    else { if (occ == 4) MARCH(false, 4); else MARCH(false, 1); }
#undef MARCH
}

// diagnostic (PYDEM_STENCIL_WARM): what the stencil -- the first kernel of a step -- pays for starting on a GPU that has been idle
// or in the sweep's latency-bound tail: 1 = a few ms of fp64 arithmetic on every CU first (clocks), 2 = the output planes
// touched first (TLB / page state), 3 = both
__global__ __launch_bounds__(256) void k_warm_alu(double *sink, int iters)
{
    double a = threadIdx.x * 1e-3, b = 1.0000001, c = 1e-9;
    for (int i = 0; i < iters; i++) { a = __builtin_fma(a, b, c); b = __builtin_fma(b, a, c); }
    if (a + b == 12345.678) sink[0] = a;
}

int stage_stencil(pydem_tile *t)
{
    static int warm = -1;
    if (warm < 0) { const char *e = getenv("PYDEM_STENCIL_WARM"); warm = e ? atoi(e) : 0; }
    if (warm & 2) { HIP_TRY(hipMemsetAsync(t->mag, 0, (size_t)t->NN * 8, t->stream)); HIP_TRY(hipMemsetAsync(t->dir, 0, (size_t)t->NN * 8, t->stream)); }
    if (warm & 1) hipLaunchKernelGGL(k_warm_alu, dim3(256 * 8), dim3(256), 0, t->stream, t->mag, 200000);
    HIP_TRY(hipEventRecord(t->ev[0], t->stream));
    launch_stencil(t);
    HIP_TRY(hipEventRecord(t->ev[1], t->stream));
    const int64_t nper = 2 * t->m + 2 * (t->n - 2);
    if (t->elev_f32)
        hipLaunchKernelGGL(k_stencil_perimeter<true>, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, t->elev,
                           (int)t->n, (int)t->m, t->rowtab, t->mag, t->dir, t->flat0);
    else
        hipLaunchKernelGGL(k_stencil_perimeter<false>, dim3((unsigned)cdiv(nper, 128)), dim3(128), 0, t->stream, t->elev,
                           (int)t->n, (int)t->m, t->rowtab, t->mag, t->dir, t->flat0);
    HIP_TRY(hipEventRecord(t->ev[2], t->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventSynchronize(t->ev[2]));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, t->ev[0], t->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, t->ev[0], t->ev[2]));
    t->tm.stencil_kernel_ms = a;
    t->tm.slopes_directions_ms = b;
    return 0;
}

int bench_stencil(pydem_tile *t, int iters, double *avg_ms)
{
    launch_stencil(t);   // warm-up
    HIP_TRY(hipEventRecord(t->ev[0], t->stream));
    for (int q = 0; q < iters; q++) launch_stencil(t);
    HIP_TRY(hipEventRecord(t->ev[1], t->stream));
    HIP_TRY(hipEventSynchronize(t->ev[1]));
    HIP_TRY(hipGetLastError());
    float a = 0;
    HIP_TRY(hipEventElapsedTime(&a, t->ev[0], t->ev[1]));
    *avg_ms = (double)a / iters;
    return 0;
}
