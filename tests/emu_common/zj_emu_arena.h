// zj_emu_arena.h -- what the stage emulations (tests/emu_orient, emu_expand, emu_cmyk, emu_color, emu_planes, emu_to_tensor,
// emu_warp) share: the write map over the caller's destination arena, and the load check against the rows of the image the
// running lane works on.  TEST INFRASTRUCTURE ONLY; include it before the kernel's header, which the PUT / GET macros feed.
#pragma once
#include <stdint.h>
#include <string.h>

static uint8_t* g_map = nullptr;     // one count per byte of [g_lo, g_hi)
static uint64_t g_lo = 0, g_hi = 0;
static long long g_outside = 0, g_bad_loads = 0, g_loads = 0;

inline void emu_arena(uint8_t* arena, size_t len, uint8_t* map)
{
    g_map = map; g_lo = (uint64_t)(uintptr_t)arena; g_hi = g_lo + len;
    g_outside = g_bad_loads = g_loads = 0;
}

// a store: performed and counted in the map; outside the arena (ALIGNED: or not on a boundary of T): counted apart, NOT performed
template <typename T, bool ALIGNED = false>
static inline void emu_put(uint64_t a, T v)
{
    if (a < g_lo || a + sizeof(T) > g_hi || (ALIGNED && (a & (sizeof(T) - 1)))) { g_outside++; return; }
    memcpy(reinterpret_cast<void*>((uintptr_t)a), &v, sizeof(T));
    for (size_t k = 0; k < sizeof(T); k++)
        if (g_map[a - g_lo + k] < 255) g_map[a - g_lo + k]++;
}

// the image the running lane belongs to: its first byte, pitch, bytes of a row, rows
static uint64_t g_img = 0, g_pitch = 1, g_rowbytes = 0, g_rows = 0;
inline void emu_image(uint64_t first, uint64_t pitch, uint64_t rowbytes, uint64_t rows)
{
    g_img = first; g_pitch = pitch; g_rowbytes = rowbytes; g_rows = rows;
}

// a load: counted; one that touches a byte outside the image's rows (ALIGNED: or is not on a boundary of T) is counted
// apart, NOT performed and yields 0
template <typename T, bool ALIGNED>
static inline T emu_get(uint64_t a)
{
    T v{};
    g_loads++;
    const uint64_t off = a - g_img, row = a >= g_img ? off / g_pitch : g_rows;
    if (a < g_img || row >= g_rows || off - row * g_pitch + sizeof(T) > g_rowbytes || (ALIGNED && (a & (sizeof(T) - 1)))) {
        g_bad_loads++;
        return v;
    }
    memcpy(&v, reinterpret_cast<const void*>((uintptr_t)a), sizeof(T));
    return v;
}
