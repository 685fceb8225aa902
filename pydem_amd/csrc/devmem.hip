// devmem.hip -- where the library's device and pinned memory comes from: the plane cache, dev_malloc / dev_free, the per-device
// scratch arena, the tile's pinned staging and the threaded whole-plane transfers.  What a tile holds is kept by tile_mem.h.
#include "internal.h"
#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <sys/mman.h>

// ---- planes of destroyed tiles are kept for the next tile of the same shape ------------------------------------------
// A fresh DEMProcessor per elevation file is how the reference is used, and a 16384^2 tile is a dozen 0.25-2 GiB planes:
// mapping them anew costs the drop-in call more than its kernels (measured: ~240 ms of hipMalloc inside a 54-ms calc_twi).
// Blocks of 1 MiB and more that tile_alloc handed out go on a per-device free list when their tile is destroyed and are
// handed out again on an exact size match (the contents are whatever the last owner left: no stage relies on fresh
// memory).  PYDEM_PLANE_CACHE_GB bounds what is kept per device (default 32, 0 = off; the least recently returned blocks are evicted first); pydem_hip_release_scratch and a
// failing hipMalloc empty the lists.
namespace {
struct FreeBlock { void *p; uint64_t stamp; };      // stamp: when the block was given back (the oldest is evicted first)
struct PlaneCache {
    std::mutex mu;
    std::multimap<size_t, FreeBlock> free_blocks;
    uint64_t clock = 0;
    std::unordered_map<void *, size_t> live;          // blocks handed out by tile_alloc (size known at destroy time)
    size_t kept = 0;
};
std::mutex g_pc_table;
std::map<int, PlaneCache *> g_pc;
PlaneCache *plane_cache(int device)
{
    std::lock_guard<std::mutex> g(g_pc_table);
    PlaneCache *&c = g_pc[device];
    if (!c) c = new PlaneCache();
    return c;
}
size_t plane_cache_limit()
{
    // default 32 GiB: the planes of one 16384^2 tile (24.7 GB) -- what the drop-in pattern "a fresh DEMProcessor per file" reuses;
    // fractions of a GB are honoured, a negative value means 0 (off)
    static const size_t lim = [] {
        const char *e = getenv("PYDEM_PLANE_CACHE_GB");
        const double gb = e ? atof(e) : 32.0;
        return (size_t)((gb > 0.0 ? gb : 0.0) * (double)((size_t)1 << 30));
    }();
    return lim;
}
// (c->mu held) take the least recently returned blocks off the lists until `room` more bytes fit under the limit; the caller
// frees them AFTER it has let go of the lock (hipFree synchronises the device)
void plane_cache_evict(PlaneCache *c, size_t room, std::vector<void *> &victims)
{
    const size_t lim = plane_cache_limit();
    while (!c->free_blocks.empty() && c->kept + room > lim) {
        auto old = c->free_blocks.begin();
        for (auto it = c->free_blocks.begin(); it != c->free_blocks.end(); ++it) if (it->second.stamp < old->second.stamp) old = it;
        victims.push_back(old->second.p);
        c->kept -= old->first;
        c->free_blocks.erase(old);
    }
}
constexpr size_t PLANE_MIN = (size_t)1 << 20;

// ---- PYDEM_MEM_POISON=<0..255>: a debug mode that makes "whatever the last owner left" a known byte --------------------
// Read at every hand-out (like PYDEM_STENCIL_SPLIT per launch: a test switches it between calls), never cached.  When it is
// set, every device block this file hands out -- a plane off the free list or mapped anew, a dev_malloc block, the whole arena
// at the start of a lease -- is filled with that byte, and the device is idle again before the pointer is returned.  Unset (or
// not a number in 0..255): nothing happens.  pydem_hip_poison_stats reports how much was filled.
std::atomic<int64_t> g_poison_blocks{0}, g_poison_bytes{0};
int poison_byte()
{
    const char *e = getenv("PYDEM_MEM_POISON");
    if (!e || !*e) return -1;
    char *end = nullptr;
    const long v = strtol(e, &end, 0);
    return (end == e || *end || v < 0 || v > 255) ? -1 : (int)v;
}
// `drain_first`: work of an earlier owner may still run on some stream of the device (the arena: the previous lease's stage
// ran on a tile stream)
void poison(void *p, size_t bytes, bool drain_first = false)
{
    const int v = poison_byte();
    if (v < 0 || !p || !bytes) return;
    if (drain_first) (void)hipDeviceSynchronize();
    (void)hipMemset(p, v, bytes);
    (void)hipDeviceSynchronize();
    g_poison_blocks += 1; g_poison_bytes += (int64_t)bytes;
}
void plane_cache_flush(int device)
{
    PlaneCache *c = plane_cache(device);
    std::lock_guard<std::mutex> g(c->mu);
    for (auto &kv : c->free_blocks) (void)hipFree(kv.second.p);
    c->free_blocks.clear(); c->kept = 0;
}
}  // namespace

void *plane_take(int device, size_t bytes)
{
    std::vector<void *> victims;                     // (PYDEM_PLANE_EVICT_ON_MISS only; freed once the lock is released)
    if (bytes >= PLANE_MIN && plane_cache_limit()) {
        PlaneCache *c = plane_cache(device);
        std::lock_guard<std::mutex> g(c->mu);
        auto it = c->free_blocks.find(bytes);
        if (it != c->free_blocks.end()) {
            void *q = it->second.p;
            c->free_blocks.erase(it); c->kept -= bytes;
            c->live[q] = bytes;
            poison(q, bytes);
            return q;
        }
        // (a size the lists do not hold: nothing is evicted here -- the blocks on the lists are those of the tile destroyed
        // last, i.e. what the tile being built asks for next; dead sizes leave when plane_give needs their room, and a failing
        // hipMalloc empties the lists.  PYDEM_PLANE_EVICT_ON_MISS=1: the round-5 behaviour, for A/B runs)
        static const bool on_miss = [] { const char *e = getenv("PYDEM_PLANE_EVICT_ON_MISS"); return e && atoi(e) > 0; }();
        if (on_miss) plane_cache_evict(c, bytes, victims);
    }
    for (void *v : victims) (void)hipFree(v);
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    {   // PYDEM_PLANE_DEBUG=1: one line per block that is mapped anew (a steady state maps nothing)
        static const bool dbg = [] { const char *d = getenv("PYDEM_PLANE_DEBUG"); return d && atoi(d) > 0; }();
        if (dbg) fprintf(stderr, "[pydem] plane_take: hipMalloc(%zu)\n", bytes);
    }
    if (e != hipSuccess) {                          // the free lists may hold what is missing
        (void)hipGetLastError();
        plane_cache_flush(device);
        e = hipMalloc(&q, bytes);
    }
    if (e != hipSuccess) { pydem_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); return nullptr; }
    if (bytes >= PLANE_MIN && plane_cache_limit()) {
        PlaneCache *c = plane_cache(device);
        std::lock_guard<std::mutex> g(c->mu);
        c->live[q] = bytes;
    }
    poison(q, bytes);
    return q;
}

void plane_give(int device, void *q)
{
    if (!q) return;
    PlaneCache *c = plane_cache(device);
    std::vector<void *> victims;
    bool kept = false;
    {
        std::lock_guard<std::mutex> g(c->mu);
        auto it = c->live.find(q);
        if (it != c->live.end()) {
            const size_t bytes = it->second;
            c->live.erase(it);
            if (bytes <= plane_cache_limit()) {
                plane_cache_evict(c, bytes, victims);
                c->free_blocks.emplace(bytes, FreeBlock{q, ++c->clock}); c->kept += bytes;
                kept = true;
            }
        }
    }
    for (void *v : victims) (void)hipFree(v);
    if (!kept) (void)hipFree(q);
}

// hipMalloc for everything else the library maps on a device (scratch, arenas, record buffers): when it fails the free lists
// of the current device are emptied and the call repeated
hipError_t dev_malloc(void **p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        int device = 0;
        (void)hipGetLastError();
        if (hipGetDevice(&device) == hipSuccess) { plane_cache_flush(device); e = hipMalloc(p, bytes); }
    }
    if (e == hipSuccess) poison(*p, bytes);
    return e;
}

int pydem_hip_poison_stats(int64_t *blocks, int64_t *bytes)
{
    if (blocks) *blocks = g_poison_blocks.load();
    if (bytes) *bytes = g_poison_bytes.load();
    return 0;
}

void dev_free(void *p) { if (p) (void)hipFree(p); }

// ---- per-device scratch arena of the conditioning stages (internal.h)
namespace {
struct DevArena { std::mutex busy; void *p = nullptr; size_t bytes = 0; };
std::mutex g_arena_table;
std::map<int, DevArena *> g_arenas;
DevArena *arena_of(int device)
{
    std::lock_guard<std::mutex> g(g_arena_table);
    DevArena *&a = g_arenas[device];
    if (!a) a = new DevArena();
    return a;
}
}  // namespace

int arena_acquire(int device, ArenaLease *L)
{
    DevArena *a = arena_of(device);
    a->busy.lock();
    L->device = device; L->arena = a; L->base = (char *)a->p; L->bytes = a->bytes; L->off = 0; L->want = 0; L->held = true;
    poison(a->p, a->bytes, true);       // (the lease starts empty: nothing the arena holds means anything)
    return 0;
}

void *arena_take(ArenaLease *L, size_t bytes)
{
    const size_t need = (bytes + 255) & ~(size_t)255;
    L->want += need ? need : 256;
    if (L->base && L->off + need <= L->bytes) { void *q = L->base + L->off; L->off += need ? need : 256; return q; }
    void *q = nullptr;
    const hipError_t e = dev_malloc(&q, need ? need : 256);
    if (e != hipSuccess) { pydem_set_error("hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e)); return nullptr; }
    L->extra.push_back(q);
    return q;
}

ArenaLease::~ArenaLease()
{
    if (!held) return;
    DevArena *a = static_cast<DevArena *>(arena);
    (void)hipSetDevice(device);
    for (void *q : extra) (void)hipFree(q);
    if (want > a->bytes) {              // next time everything fits
        if (a->p) (void)hipFree(a->p);
        a->p = nullptr; a->bytes = 0;
        void *q = nullptr;
        if (dev_malloc(&q, want + want / 8) == hipSuccess) { a->p = q; a->bytes = want + want / 8; }
    }
    a->busy.unlock();
}

int tile_pinned(pydem_tile *t, size_t bytes, void **out)
{
    if (t->h_stage_bytes < bytes) {
        if (t->h_stage) { (void)hipHostFree(t->h_stage); t->h_stage = nullptr; t->h_stage_bytes = 0; }
        const size_t want = bytes + bytes / 4 + 4096;
        HIP_TRY(hipHostMalloc(&t->h_stage, want, hipHostMallocDefault));
        t->h_stage_bytes = want;
    }
    *out = t->h_stage;
    return 0;
}

// ---- whole-plane transfers between pageable host arrays and the device ------------------------------------------------
// A plain hipMemcpy of a pageable array pins the caller's pages on the fly: measured here at ~3 GB/s for a fresh 2 GiB array
// (0.7 s for the 16384^2 elevations).  Planes of XFER_MIN bytes or more go through per-device pinned chunks instead: XFER_T
// host threads each copy their chunks between the caller's array and their two pinned buffers while their own stream moves
// the previous chunk over PCIe (the threads also take the first-touch page faults of a fresh destination array in
// parallel).  PYDEM_XFER_THREADS=0 restores the plain copy.
namespace {
constexpr size_t XFER_CHUNK = (size_t)8 << 20;
constexpr size_t XFER_MIN = (size_t)32 << 20;
constexpr int XFER_TMAX = 16;
struct XferLane { void *pin[2] = {nullptr, nullptr}; hipStream_t stream = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; };
struct XferPool { std::mutex busy; XferLane lane[XFER_TMAX]; int ready = 0; };
std::mutex g_xfer_table;
std::map<int, XferPool *> g_xfer;

int xfer_threads()
{
    static const int n = [] {
        const char *e = getenv("PYDEM_XFER_THREADS");
        int v = e ? atoi(e) : 8;
        return v < 0 ? 0 : (v > XFER_TMAX ? XFER_TMAX : v);
    }();
    return n;
}

int xfer_pool(int device, int T, XferPool **out)
{
    XferPool *P;
    {
        std::lock_guard<std::mutex> g(g_xfer_table);
        XferPool *&p = g_xfer[device];
        if (!p) p = new XferPool();
        P = p;
    }
    *out = P;
    return 0;
}

int xfer_prepare(XferPool *P, int T)      // under P->busy
{
    for (int k = P->ready; k < T; ++k) {
        XferLane &L = P->lane[k];
        for (int b = 0; b < 2; ++b) {
            if (!L.pin[b]) HIP_TRY(hipHostMalloc(&L.pin[b], XFER_CHUNK, hipHostMallocDefault));
            if (!L.ev[b]) HIP_TRY(hipEventCreateWithFlags(&L.ev[b], hipEventDisableTiming));
        }
        if (!L.stream) HIP_TRY(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        P->ready = k + 1;
    }
    return 0;
}

// one lane's share of the plane: chunks k, k + T, ...
hipError_t xfer_lane_run(int device, XferLane &L, char *dev, char *host, size_t bytes, int k, int T, bool to_host)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return e;
    const size_t nchunk = (bytes + XFER_CHUNK - 1) / XFER_CHUNK;
    size_t prev_off = 0, prev_len = 0; int prev_b = -1;
    int it = 0;
    for (size_t c = (size_t)k; c < nchunk; c += (size_t)T, ++it) {
        const int b = it & 1;
        const size_t off = c * XFER_CHUNK, len = (bytes - off < XFER_CHUNK) ? bytes - off : XFER_CHUNK;
        if (!to_host) {
            if (it >= 2 && (e = hipEventSynchronize(L.ev[b])) != hipSuccess) return e;     // the buffer's previous chunk has left
            memcpy(L.pin[b], host + off, len);
            if ((e = hipMemcpyAsync(dev + off, L.pin[b], len, hipMemcpyHostToDevice, L.stream)) != hipSuccess) return e;
            if ((e = hipEventRecord(L.ev[b], L.stream)) != hipSuccess) return e;
        } else {
            if ((e = hipMemcpyAsync(L.pin[b], dev + off, len, hipMemcpyDeviceToHost, L.stream)) != hipSuccess) return e;
            if ((e = hipEventRecord(L.ev[b], L.stream)) != hipSuccess) return e;
            if (prev_b >= 0) {
                if ((e = hipEventSynchronize(L.ev[prev_b])) != hipSuccess) return e;
                memcpy(host + prev_off, L.pin[prev_b], prev_len);
            }
            prev_b = b; prev_off = off; prev_len = len;
        }
    }
    if (to_host && prev_b >= 0) {
        if ((e = hipEventSynchronize(L.ev[prev_b])) != hipSuccess) return e;
        memcpy(host + prev_off, L.pin[prev_b], prev_len);
    }
    return hipStreamSynchronize(L.stream);
}
}  // namespace

// copy `bytes` between a device plane and a (pageable) host array; the tile's stream is drained first and the call returns
// with the transfer complete
int tile_plane_copy(pydem_tile *t, void *dev, void *host, size_t bytes, bool to_host)
{
    const int T = xfer_threads();
    if (T == 0 || bytes < XFER_MIN) {
        if (to_host) HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, t->stream));
        else HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        return 0;
    }
    HIP_TRY(hipStreamSynchronize(t->stream));          // what the plane holds (or what still reads it) is settled
    if (to_host) {
        // a fresh destination array is faulted in by the copy threads: ask for huge pages where the kernel gives them on request
        const uintptr_t a = ((uintptr_t)host + 4095) & ~(uintptr_t)4095, b = ((uintptr_t)host + bytes) & ~(uintptr_t)4095;
        if (b > a) (void)madvise((void *)a, b - a, MADV_HUGEPAGE);
    }
    XferPool *P;
    PYDEM_TRY(xfer_pool(t->device, T, &P));
    std::lock_guard<std::mutex> g(P->busy);
    PYDEM_TRY(xfer_prepare(P, T));
    hipError_t err[XFER_TMAX];
    std::thread th[XFER_TMAX];
    for (int k = 1; k < T; ++k)
        th[k] = std::thread([&, k] { err[k] = xfer_lane_run(t->device, P->lane[k], (char *)dev, (char *)host, bytes, k, T, to_host); });
    err[0] = xfer_lane_run(t->device, P->lane[0], (char *)dev, (char *)host, bytes, 0, T, to_host);
    for (int k = 1; k < T; ++k) th[k].join();
    for (int k = 0; k < T; ++k)
        if (err[k] != hipSuccess) { pydem_set_error("plane transfer: %s", hipGetErrorString(err[k])); return -1; }
    return 0;
}

void devmem_release_all()
{
    // lock order: never `busy` under the table lock (a lease holds `busy` for the length of a conditioning stage; records are
    // never deleted, so the snapshot stays valid)
    std::vector<std::pair<int, DevArena *>> all;
    {
        std::lock_guard<std::mutex> g(g_arena_table);
        for (auto &kv : g_arenas) all.push_back(kv);
    }
    for (auto &kv : all) {
        std::lock_guard<std::mutex> b(kv.second->busy);
        if (kv.second->p) { (void)hipSetDevice(kv.first); (void)hipFree(kv.second->p); kv.second->p = nullptr; kv.second->bytes = 0; }
    }
    std::vector<int> devs;
    {
        std::lock_guard<std::mutex> g(g_pc_table);
        for (auto &kv : g_pc) devs.push_back(kv.first);
    }
    for (int d : devs) { (void)hipSetDevice(d); plane_cache_flush(d); }
    // ... and the pinned chunks / streams of the whole-plane transfers (they come back with the next large transfer)
    std::vector<std::pair<int, XferPool *>> pools;
    {
        std::lock_guard<std::mutex> g(g_xfer_table);
        for (auto &kv : g_xfer) pools.push_back(kv);
    }
    for (auto &kv : pools) {
        std::lock_guard<std::mutex> b(kv.second->busy);
        (void)hipSetDevice(kv.first);
        for (int k = 0; k < kv.second->ready; k++) {
            XferLane &L = kv.second->lane[k];
            for (int q = 0; q < 2; q++) {
                if (L.pin[q]) { (void)hipHostFree(L.pin[q]); L.pin[q] = nullptr; }
                if (L.ev[q]) { (void)hipEventDestroy(L.ev[q]); L.ev[q] = nullptr; }
            }
            if (L.stream) { (void)hipStreamDestroy(L.stream); L.stream = nullptr; }
        }
        kv.second->ready = 0;
    }
}
