// streamnet.h -- what the units on the receiver tree share (streamnet.hip, pydem_stream_network; flowacc_tree.hip,
// pydem_tree_accum): the two receiver planes and the one pass over the rows that writes them, and how a call takes its stream
// set.  Semantics: include/pydem_hip.h, pydem_stream_network.
#pragma once
#include "flowdist.h"

namespace {

constexpr uint8_t SN_PIT = 8, SN_NONE = 255;

struct SnPlanes { const int32_t *recv; const uint8_t *code; };

// ---- the receivers
// "the first out-edge of greatest weight in ascending destination order, a regular edge before a pit edge to the same cell" is
// the greatest weight with ties going to the lower destination; the regular edges are offered first, so a pit edge of equal
// weight to the same cell does not replace one
__global__ __launch_bounds__(256) void k_sn_receiver(DistArgs A, int32_t *__restrict__ recv, uint8_t *__restrict__ code)
{
    for (int i = blockIdx.y; i < A.n; i += gridDim.y)
    for (int j0 = blockIdx.x * blockDim.x; j0 < A.m; j0 += gridDim.x * blockDim.x) {
        const int j = j0 + (int)threadIdx.x;
        if (j >= A.m) continue;
        const int32_t c = i * A.m + j;
        const uint32_t cw = A.cinfo[c];
        const double z = A.elev[c];
        int32_t best = -1;
        int bc = SN_NONE;
        double bw = -INFINITY;
        auto offer = [&](int32_t dst, int cd, double w) {
            if (w > bw || (w == bw && dst < best)) { bw = w; best = dst; bc = cd; }
        };
        if (z == z) {
            if (cw & (CI_OUT1 | CI_OUT2)) {
                const Facet f = dd_facet_sorted(A, cw, A.prop[c]);
                auto dir = [](int di, int dj) { const int q = (di + 1) * 3 + dj + 1; return q > 4 ? q - 1 : q; };
                if (f.a.has) offer(c + f.a.di * A.m + f.a.dj, dir(f.a.di, f.a.dj), f.a.w);
                if (f.b.has) offer(c + f.b.di * A.m + f.b.dj, dir(f.b.di, f.b.dj), f.b.w);
            }
            if (cw & CI_PIT_OUT)
                for (PitBlock b = dd_pit_block(A.pit_src, A.n_pit, c); b.more(); b.e++) offer(A.pit_dst[b.e], SN_PIT, A.pit_w[b.e]);
        }
        recv[c] = best; code[c] = (uint8_t)bc;
    }
}

}  // namespace

// The receivers are written again by every call, though they depend on the graph alone and the planes stay with the tile:
// a flag "the planes match the graph" would have to be cleared by every writer of the graph words, the proportion and the
// pit lists (tile.hip, uca.hip, uca_edge.hip, pits.hip), and one pass over the rows is 5 % of a call with both sweeps.
static int sn_receivers(pydem_tile *t, const DistArgs &A)
{
    hipLaunchKernelGGL(k_sn_receiver, dist_row_grid(t), dim3(256), 0, t->stream, A, t->sn_recv, t->sn_code);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the stream set of a call (`what`: the function's name), in the two steps of the entry points' checks: the threshold is
// finite and >= 0 when it is read; then the mask goes to the engine's byte plane, or the tile's uca is there and settled
static int sn_check_threshold(const char *what, const uint8_t *streams, double uca_threshold)
{
    if (!streams && !(uca_threshold >= 0.0 && uca_threshold < INFINITY)) {
        pydem_set_error("%s: uca_threshold must be finite and >= 0 when no stream mask is given (got %g)", what, uca_threshold);
        return -2;
    }
    return 0;
}
static int sn_stream_set(pydem_tile *t, const char *what, const uint8_t *streams)
{
    if (streams) return dist_upload(t, &t->dd_mask, streams);
    if (!t->uca || !t->have[PYDEM_UCA]) { pydem_set_error("%s: uca_threshold needs the tile's uca (pydem_uca first)", what); return -3; }
    return stage_edge_flush(t);                 // incremental edge rounds: the areas the threshold reads are settled first
}
