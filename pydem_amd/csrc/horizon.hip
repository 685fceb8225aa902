// horizon.hip -- pydem_horizon: the horizon tangent per azimuth and the sky-view factor of the resident elevation.  No reference
// method; include/pydem_hip.h states the definition, and the numpy twin (pydem_amd/horizon.py: horizon_ref) is held to it bit for
// bit: a tangent is the maximum of a fixed set of products (z[sample] - z0) * w, which no sample order changes, and the sky-view
// factor is 1.0 / (1.0 + T * T) summed from 0.0 in ascending direction and divided by the number of directions.
//   k_hz            A workgroup of four wavefronts owns HZ_BR x HZ_BC = 32 x 64 output cells: a lane per column, eight rows per
//                   lane (rows wave, wave + 4, ...), z0, T and the running svf sum of its eight cells in registers.  It walks the
//                   ray of a direction in segments of at most HZ_SEG = 32 steps.  For each segment it stages the source region in
//                   LDS -- the block shifted by the segment's offsets: (32 + span of dr) x (64 + span of dc) cells, one-sided, at
//                   most 64 rows of 96 doubles (kept 97 apart: 49 664 bytes), cells off the tile as NaN, which compare false like no data --,
//                   synchronises, takes its 8 x steps samples (a wavefront reads 64 consecutive doubles of one staged row: no bank
//                   conflicts; a lane's eight rows are constant offsets from one address; the step's weight and LDS offset sit
//                   in the lane of the step's number and come over v_readlane: no memory but the samples in the loop) and
//                   synchronises again.  A sample costs one LDS read, a subtraction, a multiplication and a maximum.
//                   One launch takes a group of consecutive directions (at most HZ_LAUNCH_STEPS steps in all, so that a launch
//                   stays short on a shared device); the svf sum travels from group to group through its plane, which the
//                   launches, issued in ascending direction on one stream, read and write: the additions keep their order.
// *n_defined: the last launch counts the cells with a finite svf (without an svf, the sum carries 0.0 for a finite tangent and NaN
// otherwise, so the same test counts the cells with every tangent finite) into the slotted counter of stage_kit.h, one atomic per
// workgroup.  The counter, the table, the svf plane and the horizon planes are one block of the tile's (tile_mem.h), grown to the
// largest request.
#include "stage_kit.h"

namespace {

constexpr int HZ_BR = 32, HZ_BC = 64;       // output rows and columns of a workgroup
constexpr int HZ_ROWS = HZ_BR / 4;          // rows per lane
constexpr int HZ_SEG = 32;                  // steps per staged segment, at most
// doubles between two staged rows: the 96 of the widest region and one more, so that a lane's rows are not a multiple of 512
// bytes apart and stay single 8-byte reads (paired into ds_read2st64_b64 they would move half the bytes per LDS cycle)
constexpr int HZ_LC = HZ_BC + HZ_SEG + 1;
constexpr int HZ_LDS = (HZ_BR + HZ_SEG) * HZ_LC;               // doubles
constexpr int HZ_LAUNCH_STEPS = 512;        // steps of all directions of one launch (one direction at least)
constexpr int HZ_MAX_DIR = 64, HZ_MAX_STEPS = 1024;

struct HzStep { double w; int off; int pad; };                          // off: (dr - rmin) * HZ_LC + (dc - cmin) in the staged region
// steps k0 .. k1 - 1 of the device's step list, k1 - k0 a multiple of 4 (padded with steps of weight 0, whose products are zeros
// or NaN and raise no tangent); the region's origin and size
struct HzSeg { int k0, k1, rmin, cmin, rows, cols, pad0, pad1; };
struct HzDir { int s0, s1, rlo, rhi, clo, chi, pad0, pad1; };           // segments s0 .. s1 - 1; the extents of all offsets (with 0)

struct HzArgs {
    int n, m, blocks_x, d0, d1, n_dir;
    int edge_nan, want_svf, first, last;
};

// planes: the n_dir horizon planes, or null; acc: the svf plane, the running sum between launches and the result after the last.
__global__ void __launch_bounds__(256)
k_hz(const double *__restrict__ elev, const HzStep *__restrict__ steps, const HzSeg *__restrict__ segs, const HzDir *__restrict__ dirs,
     double *__restrict__ planes, double *__restrict__ accp, u64 *__restrict__ ctr, HzArgs a)
{
    __shared__ double s_z[HZ_LDS];
    slot_count_begin();
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const int by = (int)(blockIdx.x / (unsigned)a.blocks_x), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)a.blocks_x);
    const int r0 = by * HZ_BR, c0 = bx * HZ_BC;
    const int n = a.n, m = a.m;
    const size_t NN = (size_t)n * m;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int col = c0 + lane;
    double z0[HZ_ROWS], acc[HZ_ROWS], T[HZ_ROWS];
#pragma unroll
    for (int i = 0; i < HZ_ROWS; i++) {
        const int row = r0 + wv + 4 * i;
        const bool in = row < n && col < m;
        z0[i] = in ? elev[(size_t)row * m + col] : nan;
        acc[i] = (in && !a.first) ? accp[(size_t)row * m + col] : 0.0;
    }
    for (int d = a.d0; d < a.d1; d++) {
        const HzDir dir = dirs[d];
#pragma unroll
        for (int i = 0; i < HZ_ROWS; i++) T[i] = 0.0;
        for (int sg = dir.s0; sg < dir.s1; sg++) {
            const HzSeg seg = segs[sg];
            const int cols = seg.cols;
            // the segment's steps, one per lane (at most HZ_SEG = 32; the lanes above them repeat): the weight and the LDS offset
            // of step j reach the wavefront over v_readlane, so that nothing but the samples waits on memory in the loop below
            const HzStep st = steps[seg.k0 + (lane < seg.k1 - seg.k0 ? lane : 0)];
            const int w_lo = __double2loint(st.w), w_hi = __double2hiint(st.w);
            __syncthreads();                                        // the samples of the segment before are taken
            // the block shifted by the segment's offsets; a cell off the tile is NaN.  A wavefront per staged row
            // (cols <= 96: two half rows), four rows per round: eight loads from clamped addresses in flight, then the stores
            for (int rb = wv; rb < seg.rows; rb += 16) {
                double x[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int gr = r0 + seg.rmin + rb + 4 * (u >> 1), gc = c0 + seg.cmin + lane + 64 * (u & 1);
                    const bool in = gr >= 0 && gr < n && gc >= 0 && gc < m;
                    const double e = elev[(size_t)(gr < 0 ? 0 : (gr < n ? gr : n - 1)) * m + (gc < 0 ? 0 : (gc < m ? gc : m - 1))];
                    x[u] = in ? e : nan;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int rr = rb + 4 * (u >> 1), cc = lane + 64 * (u & 1);
                    if (rr < seg.rows && cc < cols) s_z[rr * HZ_LC + cc] = x[u];
                }
            }
            __syncthreads();
            // the staged rows are HZ_LC doubles apart whatever the region's width: a lane's eight rows are constant offsets
            const double *base = s_z + wv * HZ_LC + lane;
            const int nk = seg.k1 - seg.k0;                         // a multiple of 4: the host pads a segment with steps of weight 0
            for (int kc = 0; kc < nk; kc += 4) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double w = __hiloint2double(__builtin_amdgcn_readlane(w_hi, kc + j), __builtin_amdgcn_readlane(w_lo, kc + j));
                    const double *p = base + __builtin_amdgcn_readlane(st.off, kc + j);
#pragma unroll
                    for (int i = 0; i < HZ_ROWS; i++) {
                        const double v = (p[i * 4 * HZ_LC] - z0[i]) * w;    // one subtraction, one multiplication (no contraction)
                        T[i] = fmax(T[i], v);                       // v where v > T; a NaN v leaves T; which zero wins is settled below
                    }
                }
            }
        }
        double *plane = planes ? planes + (size_t)d * NN : nullptr;
#pragma unroll
        for (int i = 0; i < HZ_ROWS; i++) {
            const int row = r0 + wv + 4 * i;
            const bool complete = row + dir.rlo >= 0 && row + dir.rhi < n && col + dir.clo >= 0 && col + dir.chi < m;
            // (T + 0.0: a maximum that is a zero is +0.0, as "T = 0.0; if v > T" leaves it, whichever zero fmax returned)
            const double t = (isnan(z0[i]) || (a.edge_nan && !complete)) ? nan : T[i] + 0.0;
            if (plane && row < n && col < m) plane[(size_t)row * m + col] = t;
            const double term = a.want_svf ? 1.0 / (1.0 + t * t) : (isfinite(t) ? 0.0 : nan);
            acc[i] = acc[i] + term;
        }
    }
    u64 mine = 0;
#pragma unroll
    for (int i = 0; i < HZ_ROWS; i++) {
        const int row = r0 + wv + 4 * i;
        if (row < n && col < m) {
            const double v = a.last ? acc[i] / (double)a.n_dir : acc[i];
            accp[(size_t)row * m + col] = v;
            mine += (a.last && isfinite(v)) ? 1u : 0u;
        }
    }
    if (!a.last) return;                                            // (uniform over the grid; no barrier below on this path)
    mine = wave_add(mine);
    __syncthreads();                                                // (directions without steps have no barrier above: the LDS word is zero from here)
    slot_count(ctr, mine);
}

size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

}  // namespace

int stage_horizon(pydem_tile *t, int n_dir, const int32_t *start, const int16_t *dr, const int16_t *dc, const double *w, int edge_nan,
                  double *const *horizon, double *svf, double *ms, int64_t *n_defined)
{
    const char *who = "pydem_horizon";
    if (n_dir < 1 || n_dir > HZ_MAX_DIR) { pydem_set_error("%s: n_dir %d (1 .. %d allowed)", who, n_dir, HZ_MAX_DIR); return -2; }
    if (!start || !dr || !dc || !w) { pydem_set_error("%s: the ray table is missing", who); return -2; }
    if (!horizon && !svf) { pydem_set_error("%s: no plane was asked for", who); return -2; }
    if (horizon) for (int d = 0; d < n_dir; d++) if (!horizon[d]) { pydem_set_error("%s: horizon plane %d is missing", who, d); return -2; }
    if (start[0] != 0) { pydem_set_error("%s: the table's start[0] must be 0", who); return -2; }
    // the table: per direction at most 1024 steps; finite weights > 0 that do not grow along a ray; and a segment of 32 steps
    // spans at most 32 rows and columns -- the LDS region of k_hz rests on that
    std::vector<HzStep> steps;
    std::vector<HzSeg> segs;
    std::vector<HzDir> dirs((size_t)n_dir);
    for (int d = 0; d < n_dir; d++) {
        const int lo = start[d], hi = start[d + 1];
        if (hi < lo || hi - lo > HZ_MAX_STEPS) { pydem_set_error("%s: direction %d has %d steps (0 .. %d allowed)", who, d, hi - lo, HZ_MAX_STEPS); return -2; }
        HzDir D = {(int)segs.size(), 0, 0, 0, 0, 0, 0, 0};
        // segments of equal length, a multiple of 4: 100 steps are 28 + 28 + 28 + 16, not 32 + 32 + 32 and a region staged for 4
        const int n_seg = (hi - lo + HZ_SEG - 1) / HZ_SEG;
        const int len = n_seg ? ((hi - lo + n_seg - 1) / n_seg + 3) / 4 * 4 : HZ_SEG;
        for (int k0 = lo; k0 < hi; k0 += len) {
            const int k1 = k0 + len < hi ? k0 + len : hi;
            int rmin = dr[k0], rmax = dr[k0], cmin = dc[k0], cmax = dc[k0];
            for (int k = k0; k < k1; k++) {
                if (!(std::isfinite(w[k]) && w[k] > 0) || (k > lo && w[k] > w[k - 1])) {
                    pydem_set_error("%s: weight %d of direction %d must be finite, > 0 and not above the one before", who, k - lo, d);
                    return -2;
                }
                rmin = dr[k] < rmin ? dr[k] : rmin; rmax = dr[k] > rmax ? dr[k] : rmax;
                cmin = dc[k] < cmin ? dc[k] : cmin; cmax = dc[k] > cmax ? dc[k] : cmax;
            }
            if (rmax - rmin > HZ_SEG || cmax - cmin > HZ_SEG) {
                pydem_set_error("%s: steps %d .. %d of direction %d span more than %d cells", who, k0 - lo, k1 - 1 - lo, d, HZ_SEG);
                return -2;
            }
            HzSeg S = {(int)steps.size(), 0, rmin, cmin, HZ_BR + (rmax - rmin), HZ_BC + (cmax - cmin), 0, 0};
            for (int k = k0; k < k1; k++) steps.push_back({w[k], (dr[k] - rmin) * HZ_LC + (dc[k] - cmin), 0});
            while ((steps.size() - (size_t)S.k0) % 4) steps.push_back({0.0, 0, 0});
            S.k1 = (int)steps.size();
            segs.push_back(S);
            D.rlo = rmin < D.rlo ? rmin : D.rlo; D.rhi = rmax > D.rhi ? rmax : D.rhi;
            D.clo = cmin < D.clo ? cmin : D.clo; D.chi = cmax > D.chi ? cmax : D.chi;
        }
        D.s1 = (int)segs.size();
        dirs[d] = D;
    }
    if (!t->spacing_set) { pydem_set_error("%s: call pydem_tile_set_spacing first", who); return -3; }
    if (!t->elev || !t->have[PYDEM_ELEV]) { pydem_set_error("%s: required input field %d is missing", who, (int)PYDEM_ELEV); return -3; }

    const int64_t NN = t->NN;
    // one block: the counter block (8192 bytes), the table, the svf plane, the horizon planes
    const size_t b_steps = round_up(steps.size() * sizeof(HzStep), 256), b_segs = round_up(segs.size() * sizeof(HzSeg), 256),
                 b_dirs = round_up(dirs.size() * sizeof(HzDir), 256);
    const size_t planes = 1 + (horizon ? (size_t)n_dir : 0);
    const size_t need = SLOT_BYTES + b_steps + b_segs + b_dirs + planes * (size_t)NN * 8;
    PYDEM_TRY(tile_reserve(t, &t->hz_mem, &t->hz_bytes, need, need, false));
    char *p = (char *)t->hz_mem;
    HzArgs a = {};
    u64 *ctr = (u64 *)p; p += SLOT_BYTES;
    HzStep *d_steps = (HzStep *)p; p += b_steps;
    HzSeg *d_segs = (HzSeg *)p; p += b_segs;
    HzDir *d_dirs = (HzDir *)p; p += b_dirs;
    double *d_acc = (double *)p; p += (size_t)NN * 8;
    double *d_planes = horizon ? (double *)p : nullptr;
    a.n = (int)t->n; a.m = (int)t->m; a.blocks_x = (int)cdiv(t->m, HZ_BC);
    a.n_dir = n_dir; a.edge_nan = edge_nan ? 1 : 0; a.want_svf = svf ? 1 : 0;
    if (!steps.empty()) PYDEM_TRY(tile_plane_copy(t, d_steps, steps.data(), steps.size() * sizeof(HzStep), false));
    if (!segs.empty()) PYDEM_TRY(tile_plane_copy(t, d_segs, segs.data(), segs.size() * sizeof(HzSeg), false));
    PYDEM_TRY(tile_plane_copy(t, d_dirs, dirs.data(), dirs.size() * sizeof(HzDir), false));

    Events<2> ev;
    PYDEM_TRY(ev.create());
    HIP_TRY(hipMemsetAsync(ctr, 0, SLOT_BYTES, t->stream));
    HIP_TRY(hipEventRecord(ev.e[0], t->stream));
    const unsigned blocks = (unsigned)(cdiv(t->n, HZ_BR) * (int64_t)a.blocks_x);
    for (int d0 = 0; d0 < n_dir;) {
        int d1 = d0 + 1;
        while (d1 < n_dir && start[d1 + 1] - start[d0] <= HZ_LAUNCH_STEPS) d1++;
        a.d0 = d0; a.d1 = d1; a.first = d0 == 0; a.last = d1 == n_dir;
        hipLaunchKernelGGL(k_hz, dim3(blocks), dim3(256), 0, t->stream, (const double *)t->elev, (const HzStep *)d_steps, (const HzSeg *)d_segs,
                           (const HzDir *)d_dirs, d_planes, d_acc, ctr, a);
        HIP_TRY(hipGetLastError());
        d0 = d1;
    }
    hipLaunchKernelGGL(k_slot_total<>, dim3(1), dim3(64), 0, t->stream, ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], t->stream));
    HIP_TRY(hipMemcpyAsync(t->h_counters, ctr + SLOT_TOTAL, 8, hipMemcpyDeviceToHost, t->stream));       // (the pinned mirror: scratch of every stage)
    HIP_TRY(hipStreamSynchronize(t->stream));
    const u64 count = *(volatile u64 *)t->h_counters;
    if (horizon) for (int d = 0; d < n_dir; d++) PYDEM_TRY(tile_plane_copy(t, d_planes + (size_t)d * NN, horizon[d], (size_t)NN * 8, true));
    if (svf) PYDEM_TRY(tile_plane_copy(t, d_acc, svf, (size_t)NN * 8, true));
    if (n_defined) *n_defined = (int64_t)count;
    if (ms) PYDEM_TRY(ev.elapsed(0, 1, ms));
    return 0;
}
