// uca_graph.h -- what the per-tile flow accumulation (uca.hip) and the cross-tile edge fix-up (uca_edge.hip) share: the
// per-cell graph word, the neighbour tables and keep-filter of the implicit flow graph (reference
// pydem/dem_processing.py _mk_adjacency_matrix :1072-1153), the sweep's argument block and queue entry, and the layout
// of the tile's 64-word counter block.  Device helpers stay __forceinline__ in the unnamed namespace of the including unit.
#pragma once
#include "internal.h"
#include <stdlib.h>

namespace {

// Per-cell graph word `cinfo` (one 32-bit load tells a thread everything static about a cell and its
// sweep state; the sweep is bound by the number of distinct cache lines it touches per cell):
//   bits 0-7   inmask: which of the 8 neighbours (NW N NE W E SW S SE) drain into this cell
//   bit  8/9   regular out-edge to the facet's first / second neighbour survives the keep-filter
//   bit  10/11 cell has pit out-edges / pit in-edges (side lists)
//   bits 12-14 facet index (section) when bit 8 or 9 is set
//   bits 15-31 level: sweep round in which the cell is processed (CI_LEVEL_INF = not yet known)
constexpr uint32_t CI_OUT1 = 1u << 8, CI_OUT2 = 1u << 9, CI_PIT_OUT = 1u << 10, CI_PIT_IN = 1u << 11;
constexpr int CI_SEC_SHIFT = 12, CI_LEVEL_SHIFT = 15;
constexpr uint32_t CI_LEVEL_INF = 0x1FFFFu, CI_STATIC_MASK = 0x7FFFu;
__device__ __forceinline__ uint32_t ci_level(uint32_t w) { return w >> CI_LEVEL_SHIFT; }
__device__ __forceinline__ int ci_section(uint32_t w) { return (int)((w >> CI_SEC_SHIFT) & 7u); }
__device__ __forceinline__ uint32_t ci_with_level(uint32_t w, uint32_t lv) { return (w & CI_STATIC_MASK) | (lv << CI_LEVEL_SHIFT); }

// 8-neighbour offsets in ascending cell-id order: NW N NE W E SW S SE
__device__ __constant__ const int NB_DI[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
__device__ __constant__ const int NB_DJ[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
// a neighbour at offset d drains into the centre iff its section is one of these two facets
// (its e1 -- for cardinal offsets -- or e2 -- for diagonal offsets -- points back at the centre)
__device__ __constant__ const int NB_S0[8] = {6, 5, 4, 0, 3, 0, 1, 2};
__device__ __constant__ const int NB_S1[8] = {7, 6, 5, 7, 4, 1, 2, 3};

// keep-filter of _mk_adjacency_matrix (:1136-1137)
__device__ __forceinline__ bool keep_edge(double w, double z_to, double z_from)
{
    return !isnan(w) && (w > 1e-8) && (z_to <= z_from);
}

struct SweepArgs {
    uint32_t *cinfo;
    const double *prop, *a0;     // a0[i] = dX2[i]*dY2[i]
    double *area;
    double2 *contrib;            // per cell: (area*w1, area*w2), negated when the cell carries edge_todo taint
    uint8_t *todo_work;
    int n, m;
    // pit side lists: out-edges sorted by (src, dst), in-edges sorted by (dst, src), block start tables
    const int32_t *pit_src, *pit_dst;
    const int32_t *pin_dst, *pin_src; const double *pin_w;
    int64_t n_pit;
    int dbg;                     // timing experiments only (PYDEM_TILE_DEBUG)
    int32_t qcap;                // frontier queue capacity (entries)
    int32_t *err;                // queue overflow counter
    int32_t *tile_open;          // per 32x32 tile: cells still open after its last visit (INT_MAX pattern: not visited yet)
};

// A frontier entry carries the cell AND its graph word: the round that processes it starts its
// gathers straight from the queue load (one dependent memory round trip less per round -- the long
// tail of the sweep is nothing but such round trips).
struct QE { int32_t c; uint32_t cw; };

// Slots of pydem_tile::counters (64 device words) and of its pinned mirror h_counters, as uca.hip, uca_edge.hip and
// pydem_uca_weighted (tile.hip) use them.  A stage owns the block while it runs: stages of one tile never overlap, so
// words may be reused from one stage to the next, never inside one.  (pits.hip, flats.hip and the conditioning units
// index the block on their own while THEY run.)
enum CounterSlot : int {
    // ---- [0..15]: the window that every look of the host at a queue cascade copies (CS_WINDOW words)
    CS_FRONTIER = 0,        // [0..2] rotating frontier sizes: level r reads queue[r % 2] / [r % 3], appends to [(r + 1) % 3], clears
                            // [(r + 2) % 3].  Queue rounds of the sweep; every cascade of the fix-up.  Zeroed with the window.
    CS_PROCESSED = 3,       // sweep: cells processed so far (kernels add, the host reads after each batch, the re-seed replay adds its own)
    CS_SOURCES = 4,         // sweep, queue schedule: source cells of round 0
    CS_ROUNDS = 5,          // sweep: rounds run (kernels add through CS_PROCESSED + 2) -> pydem_timings::sweep_rounds
    CS_EDGE_REACHED = 6,    // classic fix-up round: length of the list of reached cells (k_edge_init .. k_edge_cleanup)
    CS_EDGE_CLEARED = 7,    // classic fix-up round: cells whose edge_done byte it cleared -> pydem_tile::etodo_prev
    CS_EDGE_SEEDS = 8,      // classic fix-up round: seeds found by k_edge_init
    CS_CASCADE_STATE = 12,  // fix-up: the level a one-workgroup kernel (k_edge_small, k_einc_small, k_cinc_small) stopped at
    CS_SWEEP_STATE = 14,    // sweep, queue schedule: the round k_sweep_small stopped at
    CS_QUEUE_ERR = 15,      // SweepArgs::err: entries that did not fit the frontier queue
    CS_WINDOW = 16,         // (a count, not a slot)
    CS_H_CB_TOTALS = 16,    // h_counters only: while the device operator build (uca_cbuild.inl) runs, the mirror holds the build's own
                            // CBC_* words in [0..15] and, here, two list totals read back with them
    // ---- [16..39]: scratch of the per-tile path.  Shared on purpose, one user after the other: the 12 doubles of the corner sums
    // (stage_section_graph, dead before the sweep), then the 16 band counters of the two full tile passes, then the 3 x 8
    // rotating work counters of the listed passes.
    CS_WORK = 16, CS_WORK_WORDS = 24,
    // ---- [32..55]: 12 64-bit accumulators of the PYDEM_TILE_DEBUG & 4 visit profile (kernels reach them as SweepArgs::err + 17).
    // Overlaps [32..39] of the work counters and, across stages, the fix-up's words below: intended (a timing diagnostic of the
    // tile visits; stage_sweep zeroes it before the passes it profiles).
    CS_TILE_PROF = 32, CS_TILE_PROF_WORDS = 24,
    // ---- [40..55]: the fix-up's own words, live across the incremental rounds of a tile (einc_prepare zeroes [48..55])
    CS_EINC_PROF = 40,      // [40..47] PYDEM_EINC_PROF: counts and clocks of the four phases of a one-workgroup cascade
    CS_ND_COUNT = 48,       // [48..49] 64-bit: cells that are not done (k_nd_count); [48..55] are zeroed with it
    CS_ND_NEXT = 50,        // compact form: next free record (k_nd_assign)
    CS_NAN_SEEDS = 53,      // length of the NaN seed list of a round (k_*_seed append, k_*_nan_flood reads)
    CS_COND_EDGES = 54,     // condensed form: pit -> drain edges between records (k_cond_pit_edges)
    // ---- [56..63]: the sweep's tile lists and re-seed replay
    CS_TILE_LIST = 56,      // [56..58] rotating sizes of the tile lists (pass p reads [p % 3]); [59] is zeroed with them
    CS_RESEED = 60,         // [60] unfinished cells collected, [61] NaN flag, [62] cells the replay finished
    CS_FLAT_SAVE = 62,      // [62..63] 64-bit: flats counted by pydem_uca_weighted before the graph stage (dead before the sweep starts)
    CS_END = 64
};
static_assert(CS_FRONTIER + 3 <= CS_PROCESSED && CS_ROUNDS == CS_PROCESSED + 2, "kernels reach the round count through the processed-cells pointer");
static_assert(CS_ROUNDS < CS_EDGE_REACHED && CS_EDGE_SEEDS < CS_CASCADE_STATE && CS_CASCADE_STATE < CS_SWEEP_STATE && CS_SWEEP_STATE < CS_QUEUE_ERR,
              "the scalars of a cascade are live together");
static_assert(CS_QUEUE_ERR < CS_WINDOW && CS_WINDOW <= CS_WORK, "one copy of the window shows the host every scalar of a cascade, and no scratch");
static_assert(CS_WORK + CS_WORK_WORDS <= CS_EINC_PROF, "zeroing the per-tile scratch leaves the fix-up's words alone");
static_assert(CS_TILE_PROF + CS_TILE_PROF_WORDS <= CS_TILE_LIST, "the visit profile ends before the tile lists");
static_assert(CS_EINC_PROF + 8 <= CS_ND_COUNT && CS_ND_COUNT + 2 <= CS_ND_NEXT && CS_ND_NEXT < CS_NAN_SEEDS && CS_NAN_SEEDS < CS_COND_EDGES
              && CS_COND_EDGES < CS_TILE_LIST, "the fix-up's words are live together and stay clear of the sweep's");
static_assert(CS_TILE_LIST + 4 <= CS_RESEED && CS_RESEED + 3 <= CS_END && CS_FLAT_SAVE + 2 <= CS_END, "the sweep's lists and replay words are live together");

inline int grid_for(int64_t work, int cap) { const int64_t g = cdiv(work, 256); return (int)(g < cap ? (g > 0 ? g : 1) : cap); }
}  // namespace

static void fill_sweep_args(pydem_tile *t, SweepArgs &A)
{
    A.cinfo = t->cinfo; A.prop = t->prop; A.a0 = t->row_area; A.area = t->uca;
    A.contrib = (double2 *)t->contrib; A.todo_work = t->todo_work; A.n = (int)t->n; A.m = (int)t->m;
    A.pit_src = t->pits.src; A.pit_dst = t->pits.dst; A.n_pit = t->pits.n_edges;
    A.pin_dst = t->pits.in_dst; A.pin_src = t->pits.in_src; A.pin_w = t->pits.in_w;
    A.qcap = (int32_t)(t->NN / 2 < INT32_MAX ? t->NN / 2 : INT32_MAX);      // queue buffers hold NN ints = NN/2 entries
    A.err = t->counters + CS_QUEUE_ERR;
    A.tile_open = nullptr;           // (stage_sweep points it at its scratch)
    { const char *e = getenv("PYDEM_TILE_DEBUG"); A.dbg = e ? atoi(e) : 0; }
}
