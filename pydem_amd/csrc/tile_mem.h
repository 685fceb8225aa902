// tile_mem.h -- what a tile holds on the device: one registry, one way in, one way to grow, one way out (host only).
// Every device block a pydem_tile member points to is listed in t->blocks with the address of that member, its size and the
// way it came: through the plane cache (plane_take / plane_give -- planes, handed to the next tile on an exact size match) or
// straight from the device (dev_malloc / dev_free -- scratch whose size moves from call to call and would only litter the
// exact-size free lists).  t->device_bytes is written here and nowhere else, and is the sum over the list.
#pragma once
#include "internal.h"

inline TileBlock *tile_block(pydem_tile *t, const void *slot)
{
    for (TileBlock &b : t->blocks) if (b.slot == slot) return &b;
    return nullptr;
}

// `bytes` for an empty slot, listed
inline int tile_hold(pydem_tile *t, void **slot, size_t bytes, bool cached)
{
    void *q = nullptr;
    if (cached) {
        q = plane_take(t->device, bytes);          // (sets the error itself)
        if (!q) return -1;
    } else {
        const hipError_t e = dev_malloc(&q, bytes);
        if (e != hipSuccess) { pydem_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); return -1; }
    }
    *slot = q;
    t->blocks.push_back({slot, bytes, cached});
    t->device_bytes += (int64_t)bytes;
    return 0;
}

// the slot's block goes back the way it came and off the list; the slot is null afterwards (an empty slot is fine)
inline void tile_drop(pydem_tile *t, void **slot)
{
    TileBlock *b = tile_block(t, slot);
    if (!b) return;
    if (b->cached) plane_give(t->device, *slot); else dev_free(*slot);
    t->device_bytes -= (int64_t)b->bytes;
    *slot = nullptr;
    *b = t->blocks.back();
    t->blocks.pop_back();
}

// `count` elements for a slot that keeps its first size for the life of the tile: the first call allocates (a plane), a later
// one is a no-op -- or an error when it asks for more than the slot holds
template <typename T>
int tile_alloc(pydem_tile *t, T **p, size_t count)
{
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    if (!*p) return tile_hold(t, (void **)p, bytes, true);
    const TileBlock *b = tile_block(t, p);
    if (b && bytes <= b->bytes) return 0;
    pydem_set_error("tile_alloc: %zu bytes asked of a slot that holds %zu", bytes, b ? b->bytes : (size_t)0);
    return -1;
}

// grow only: nothing while *cap_bytes >= need; otherwise the old block goes back and the slot and its capacity are cleared BEFORE
// `want` (>= need: the caller's headroom policy) bytes are allocated, so a failure leaves an empty slot, not a freed pointer
template <typename T>
int tile_reserve(pydem_tile *t, T **slot, size_t *cap_bytes, size_t need, size_t want, bool cached)
{
    if (*cap_bytes >= need) return 0;
    tile_drop(t, (void **)slot);
    *cap_bytes = 0;
    PYDEM_TRY(tile_hold(t, (void **)slot, want, cached));
    *cap_bytes = want;
    return 0;
}

// everything on the list goes back (pydem_tile_destroy, once the tile's streams are idle)
inline void tile_release_all(pydem_tile *t)
{
    while (!t->blocks.empty()) tile_drop(t, t->blocks.front().slot);
}

// the same growth for a device block that no tile owns (comm.hip): `need` / `want` / *cap count elements of T
template <typename T, typename N>
int dev_reserve(T **p, N *cap, size_t need, size_t want)
{
    if ((size_t)*cap >= need) return 0;
    dev_free(*p);
    *p = nullptr; *cap = 0;
    void *q = nullptr;
    HIP_TRY(dev_malloc(&q, want * sizeof(T)));
    *p = (T *)q; *cap = (N)want;
    return 0;
}
