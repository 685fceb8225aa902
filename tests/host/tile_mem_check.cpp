// tile_mem_check.cpp -- the tile's ownership layer (pydem_amd/csrc/tile_mem.h) on the host, against malloc-backed fakes of the
// four calls through which it reaches the device.  Built and run by tests/test_tile_mem_host.py with the address and
// undefined-behaviour sanitizers; no GPU is touched.  Exit status 0 and a last line "tile_mem_check: ok" mean every check held.
#include "../../pydem_amd/csrc/internal.h"
#include <functional>
#include <map>
#include <stdarg.h>

namespace {

// ---- the fake device: counts live bytes, remembers the way every block came, fails the k-th allocation on request.  Freed
// blocks stay on a graveyard until the scenario ends, so an address is never handed out twice and a second free of a block
// is seen as such
struct Block { size_t bytes; bool cached; };
struct FakeDevice {
    std::map<void *, Block> live;
    std::vector<void *> graveyard;
    size_t live_bytes = 0;
    long allocs = 0, fail_at = 0;           // fail_at: 1-based index of the allocation that fails (0: none)
    long freed_cached = 0, freed_plain = 0, wrong_way = 0, not_live = 0, errors_set = 0;
    void reset(long fail)
    {
        for (auto &kv : live) free(kv.first);
        for (void *q : graveyard) free(q);
        *this = FakeDevice();
        fail_at = fail;
    }
} F;

void *fake_alloc(size_t bytes, bool cached)
{
    if (++F.allocs == F.fail_at) return nullptr;
    void *q = malloc(bytes ? bytes : 1);
    F.live[q] = Block{bytes, cached};
    F.live_bytes += bytes;
    return q;
}

void fake_free(void *q, bool cached)
{
    if (!q) return;
    auto it = F.live.find(q);
    if (it == F.live.end()) { F.not_live++; return; }        // freed twice, or never allocated
    if (it->second.cached != cached) F.wrong_way++;
    (cached ? F.freed_cached : F.freed_plain)++;
    F.live_bytes -= it->second.bytes;
    F.live.erase(it);
    F.graveyard.push_back(q);
}

int g_failed = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            g_failed++;                                                             \
            fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                           \
            fprintf(stderr, "\n");                                                  \
        }                                                                           \
    } while (0)

}  // namespace

void pydem_set_error(const char *, ...) { F.errors_set++; }
void *plane_take(int, size_t bytes)
{
    void *q = fake_alloc(bytes, true);
    if (!q) pydem_set_error("plane_take failed");
    return q;
}
void plane_give(int, void *q) { fake_free(q, true); }
hipError_t dev_malloc(void **p, size_t bytes) { *p = fake_alloc(bytes, false); return *p ? hipSuccess : hipErrorOutOfMemory; }
void dev_free(void *p) { fake_free(p, false); }

namespace {

// ---- the script: what a tile does to its slots over a few calls (planes that keep their size, scratch that regrows, a pit
// view that regrows through the plane cache, headroom that swallows a slightly larger need)
struct World { pydem_tile t; size_t raw_bytes = 0; };
struct Step {
    const char *what;
    std::function<int(World &)> run;
    std::function<void **(World &)> slot;
    std::function<size_t *(World &)> cap;      // null for tile_alloc slots
    bool allocates;
};

template <typename T> std::function<void **(World &)> slot_of(T *pydem_tile::*m) { return [m](World &w) { return (void **)&(w.t.*m); }; }

std::vector<Step> script()
{
    auto scratch = [](World &w) { return (void **)&w.t.scratch; };
    auto scratch_cap = [](World &w) { return &w.t.scratch_bytes; };
    auto raw = [](World &w) { return (void **)&w.t.pits.raw_src; };
    auto raw_cap = [](World &w) { return &w.raw_bytes; };
    auto sortb = [](World &w) { return (void **)&w.t.pits.sort_buf; };
    auto sort_cap = [](World &w) { return &w.t.pits.sort_bytes; };
    auto cond = [](World &w) { return (void **)&w.t.cond_mem; };
    auto cond_cap = [](World &w) { return &w.t.cond_bytes; };
    return {
        {"alloc elev", [](World &w) { return tile_alloc(&w.t, &w.t.elev, 4096); }, slot_of(&pydem_tile::elev), nullptr, true},
        {"alloc flats", [](World &w) { return tile_alloc(&w.t, &w.t.flats, 4096); }, slot_of(&pydem_tile::flats), nullptr, true},
        {"alloc elev again, same size", [](World &w) { return tile_alloc(&w.t, &w.t.elev, 4096); }, slot_of(&pydem_tile::elev), nullptr, false},
        {"reserve scratch 1000", [](World &w) { return tile_reserve(&w.t, &w.t.scratch, &w.t.scratch_bytes, 1000, 1000, false); }, scratch, scratch_cap, true},
        {"reserve scratch 500 (held)", [](World &w) { return tile_reserve(&w.t, &w.t.scratch, &w.t.scratch_bytes, 500, 500, false); }, scratch, scratch_cap, false},
        {"reserve scratch 3000 (regrows)", [](World &w) { return tile_reserve(&w.t, &w.t.scratch, &w.t.scratch_bytes, 3000, 3000, false); }, scratch, scratch_cap, true},
        {"reserve pit view 8192, cached", [](World &w) { return tile_reserve(&w.t, &w.t.pits.raw_src, &w.raw_bytes, 8192, 8192, true); }, raw, raw_cap, true},
        {"reserve pit view 20000, cached (regrows)", [](World &w) { return tile_reserve(&w.t, &w.t.pits.raw_src, &w.raw_bytes, 20000, 20000, true); }, raw, raw_cap, true},
        {"reserve sort 100 + headroom", [](World &w) { return tile_reserve(&w.t, &w.t.pits.sort_buf, &w.t.pits.sort_bytes, 100, 125, false); }, sortb, sort_cap, true},
        {"reserve sort 120 (inside the headroom)", [](World &w) { return tile_reserve(&w.t, &w.t.pits.sort_buf, &w.t.pits.sort_bytes, 120, 150, false); }, sortb, sort_cap, false},
        {"reserve sort 200 + headroom (regrows)", [](World &w) { return tile_reserve(&w.t, &w.t.pits.sort_buf, &w.t.pits.sort_bytes, 200, 250, false); }, sortb, sort_cap, true},
        {"alloc counters, count 0", [](World &w) { return tile_alloc(&w.t, &w.t.counters, 0); }, slot_of(&pydem_tile::counters), nullptr, true},
        {"reserve cond 4096 + headroom", [](World &w) { return tile_reserve(&w.t, &w.t.cond_mem, &w.t.cond_bytes, 4096, 4608, false); }, cond, cond_cap, true},
    };
}

size_t listed_bytes(const pydem_tile &t)
{
    size_t s = 0;
    for (const TileBlock &b : t.blocks) s += b.bytes;
    return s;
}

void check_books(const World &w, const char *what)
{
    CHECK(w.t.device_bytes == (int64_t)F.live_bytes, "%s: device_bytes %lld, live %zu", what, (long long)w.t.device_bytes, F.live_bytes);
    CHECK(listed_bytes(w.t) == F.live_bytes, "%s: listed %zu, live %zu", what, listed_bytes(w.t), F.live_bytes);
    CHECK(w.t.blocks.size() == F.live.size(), "%s: %zu blocks listed, %zu live", what, w.t.blocks.size(), F.live.size());
    CHECK(F.wrong_way == 0 && F.not_live == 0, "%s: %ld blocks went back the wrong way, %ld were not live", what, F.wrong_way, F.not_live);
}

void check_released(World &w, const char *what)
{
    const long n_cached = [&] { long k = 0; for (auto &kv : F.live) k += kv.second.cached; return k; }();
    const long n_plain = (long)F.live.size() - n_cached;
    const long c0 = F.freed_cached, p0 = F.freed_plain;
    tile_release_all(&w.t);
    CHECK(F.live.empty() && F.live_bytes == 0, "%s: %zu blocks (%zu bytes) live after tile_release_all", what, F.live.size(), F.live_bytes);
    CHECK(F.freed_cached - c0 == n_cached && F.freed_plain - p0 == n_plain, "%s: release gave back %ld cached / %ld plain blocks, held %ld / %ld",
          what, F.freed_cached - c0, F.freed_plain - p0, n_cached, n_plain);
    CHECK(F.wrong_way == 0 && F.not_live == 0, "%s: %ld blocks went back the wrong way, %ld were freed twice", what, F.wrong_way, F.not_live);
    CHECK(w.t.device_bytes == 0 && w.t.blocks.empty(), "%s: device_bytes %lld, %zu blocks after tile_release_all", what, (long long)w.t.device_bytes, w.t.blocks.size());
    tile_release_all(&w.t);                 // a second walk finds nothing
    CHECK(F.not_live == 0, "%s: a second tile_release_all freed %ld blocks again", what, F.not_live);
}

// the whole script without a failure; returns the number of allocations it made
long run_clean()
{
    F.reset(0);
    World w;
    const std::vector<Step> steps = script();
    for (const Step &s : steps) {
        const long a0 = F.allocs;
        void *before = *s.slot(w);
        const int rc = s.run(w);
        CHECK(rc == 0, "%s: returned %d", s.what, rc);
        CHECK((F.allocs != a0) == s.allocates, "%s: %ld allocations", s.what, F.allocs - a0);
        if (!s.allocates) CHECK(*s.slot(w) == before, "%s: the slot moved", s.what);
        CHECK(*s.slot(w) != nullptr, "%s: empty slot", s.what);
        check_books(w, s.what);
    }
    CHECK(F.freed_cached == 1 && F.freed_plain == 2, "regrowth gave back %ld cached / %ld plain blocks, expected 1 / 2", F.freed_cached, F.freed_plain);
    CHECK(w.t.device_bytes == 4096 * 8 + 4096 + 3000 + 20000 + 250 + 4 + 4608, "device_bytes %lld at the end of the script", (long long)w.t.device_bytes);
    // a held slot: the same or a smaller size is a no-op, a larger one an error that changes nothing
    {
        const long a0 = F.allocs, e0 = F.errors_set;
        double *held = w.t.elev;
        CHECK(tile_alloc(&w.t, &w.t.elev, 4096) == 0 && tile_alloc(&w.t, &w.t.elev, 100) == 0, "tile_alloc of a held slot, same / smaller size");
        CHECK(F.errors_set == e0, "a message was set for a no-op");
        CHECK(tile_alloc(&w.t, &w.t.elev, 4097) != 0, "tile_alloc of a held slot with a larger size returned 0");
        CHECK(F.errors_set == e0 + 1, "%ld messages for the larger request", F.errors_set - e0);
        CHECK(F.allocs == a0 && w.t.elev == held, "tile_alloc of a held slot allocated or moved the slot");
        check_books(w, "held slot");
    }
    const long n = F.allocs;
    check_released(w, "clean run");
    for (const Step &s : steps) CHECK(*s.slot(w) == nullptr, "%s: slot not cleared by tile_release_all", s.what);
    return n;
}

// the script with its k-th allocation failing
void run_failing(long k)
{
    F.reset(k);
    World w;
    char what[160];
    bool failed = false;
    for (const Step &s : script()) {
        snprintf(what, sizeof(what), "allocation %ld fails, step '%s'", k, s.what);
        const long e0 = F.errors_set;
        const int rc = s.run(w);
        check_books(w, what);
        if (rc == 0) { CHECK(F.allocs < k || !s.allocates, "%s: returned 0", what); continue; }
        failed = true;
        CHECK(F.allocs == k, "%s: failed at allocation %ld", what, F.allocs);
        CHECK(F.errors_set > e0, "%s: no message", what);
        CHECK(*s.slot(w) == nullptr, "%s: the slot keeps %p", what, *s.slot(w));
        if (s.cap) CHECK(*s.cap(w) == 0, "%s: the capacity is still %zu", what, *s.cap(w));
        CHECK(tile_block(&w.t, s.slot(w)) == nullptr, "%s: the slot is still listed", what);
        // the caller's next call finds an empty slot and simply allocates
        F.fail_at = 0;
        CHECK(s.run(w) == 0 && *s.slot(w) != nullptr, "%s: the retry did not allocate", what);
        check_books(w, what);
        break;
    }
    CHECK(failed, "allocation %ld: no step failed", k);
    check_released(w, what);
}

// dev_reserve: the same growth for a block that no tile owns
void run_dev_reserve()
{
    F.reset(0);
    double *p = nullptr; int64_t cap = 0;
    CHECK(dev_reserve(&p, &cap, 100, 100) == 0 && p && cap == 100 && F.live_bytes == 800, "dev_reserve 100");
    double *held = p;
    CHECK(dev_reserve(&p, &cap, 50, 50) == 0 && p == held && cap == 100, "dev_reserve 50 (held)");
    F.fail_at = F.allocs + 1;
    CHECK(dev_reserve(&p, &cap, 200, 200) != 0, "dev_reserve with a failing allocation returned 0");
    CHECK(p == nullptr && cap == 0 && F.live_bytes == 0, "dev_reserve after a failure: %p, capacity %lld, %zu bytes live", (void *)p, (long long)cap, F.live_bytes);
    CHECK(dev_reserve(&p, &cap, 200, 200) == 0 && p && cap == 200 && F.live_bytes == 1600, "dev_reserve 200 after the failure");
    dev_free(p);
    CHECK(F.live.empty() && F.wrong_way == 0 && F.not_live == 0, "dev_reserve: %zu blocks left", F.live.size());
}

}  // namespace

int main()
{
    const long n = run_clean();
    CHECK(n == 10, "the script made %ld allocations", n);
    for (long k = 1; k <= n; k++) run_failing(k);
    run_dev_reserve();
    F.reset(0);
    if (g_failed) { fprintf(stderr, "tile_mem_check: %d checks failed\n", g_failed); return 1; }
    printf("tile_mem_check: ok (%ld allocations, each failed once)\n", n);
    return 0;
}
