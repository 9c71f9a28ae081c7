// zj_emu_planes.cpp -- CPU EMULATION of the planes-to-RGB kernel (zune-jpeg_amd/csrc/zj_planes.hip: zj_planes_combine_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_cmyk: the kernel's ZJ_HD functions (zj_planes.h) built by g++ with ZJ_EMU, every
// lane of every workgroup of the launch's grid run one after the other.  Every store is counted in a write map over the
// caller's destination arena; a store that falls outside the arena is counted apart and NOT performed.  Every load is looked
// up in the caller's map of the source bytes that are samples an image shows: a load that touches any other byte is counted
// and gives zeros.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../emu_common/zj_emu_arena.h"
#define ZJ_EXPAND_PUT(T, addr, v) emu_put<T>((addr), (v))

#include "../../zune-jpeg_amd/csrc/zj_expand.h"

// the loads of zj_planes.h (its stores are expand_put's, above)
static const uint8_t* g_needed = nullptr; // one flag per byte of [g_rlo, g_rhi)
static uint64_t g_rlo = 0, g_rhi = 0;
static long long g_bad_reads = 0;
alignas(16) static const uint8_t g_zero[16] = {0};
template <typename T>
static inline T* emu_needed(uint64_t a)
{
    bool ok = a >= g_rlo && a + sizeof(T) <= g_rhi;
    for (size_t k = 0; ok && k < sizeof(T); k++) ok = g_needed[a - g_rlo + k] != 0;
    if (!ok) { g_bad_reads++; return reinterpret_cast<T*>(g_zero); }
    return reinterpret_cast<T*>((uintptr_t)a);
}
#undef ZJ_RZ_GLOBAL
#define ZJ_RZ_GLOBAL(T, v) (emu_needed<T>(v))

#include "../../zune-jpeg_amd/csrc/zj_planes.h"
// (the other stages' headers, which come with zj_stage_pack.h and are not run here, load as they are written)
#undef ZJ_RZ_GLOBAL
#define ZJ_RZ_GLOBAL(T, v) (reinterpret_cast<T*>(v))
#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

template <bool CHW, bool STORED>
static void run(const PlanesParams& p)
{
    const int gx = planes_grid(p);
    for (int z = 0; z < p.nimg; z++)
        for (int bx = 0; bx < gx; bx++)
            for (int t = 0; t < PLANES_NT; t++) planes_lane<CHW, STORED>(p, z, (uint32_t)bx * PLANES_NT + (uint32_t)t);
}

extern "C" int zjpl_run(void) { return PLANES_RUN; }
extern "C" int zjpl_batch(void) { return PLANES_BATCH; }
extern "C" int zjpl_params_bytes(void) { return (int)sizeof(PlanesParams); }
extern "C" long long zjpl_bad_reads(void) { return g_bad_reads; }

// n images as the launches of the library's call (PLANES_BATCH images each); planes, pitch: three per image; wh: w, h pairs;
// geo: twelve per image, rx ry px py of each component.  Every destination byte must lie in [arena, arena + len): map gets
// the number of times each of them was stored; every source byte read must be flagged in needed[0, src_len) over
// [src, src + src_len).  Returns the stores that fell outside (not performed), < 0: arguments; zjpl_bad_reads() then gives
// the loads that touched a byte not flagged
extern "C" long long zjpl_combine(int n, const uint8_t* const* planes, const unsigned* pitch, const unsigned* wh, const uint8_t* geo,
                                  int stored_rgb, int chw, uint8_t* const* out, const unsigned* out_pitch, uint8_t* arena, size_t len,
                                  uint8_t* map, const uint8_t* src, size_t src_len, const uint8_t* needed)
{
    if (n <= 0 || !stage_sizes((size_t)n, wh)) return -1;
    emu_arena(arena, len, map);
    g_needed = needed; g_rlo = (uint64_t)(uintptr_t)src; g_rhi = g_rlo + src_len; g_bad_reads = 0;
    std::vector<uint32_t> geos((size_t)n, 0);
    for (int f = 0; f < n; f++)
        for (int c = 0; c < 3; c++) {
            const uint8_t* g = geo + 12 * f + 4 * c;
            unsigned pw;
            uint32_t bits;
            if (!planes_component(wh[2 * f], g[0], g[1], g[2], g[3], pw, bits)) return -1;
            geos[f] |= bits << (8 * c);
        }
    const uint8_t* const* const of[3] = {planes, planes + 1, planes + 2};
    PlanesParams p{};
    stage_batches<PLANES_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_planes(p, of, 3, pitch, wh, geos.data(), out, out_pitch, f0, m);
        if (chw) { if (stored_rgb) run<true, true>(p); else run<true, false>(p); }
        else { if (stored_rgb) run<false, true>(p); else run<false, false>(p); }
        return 0;
    });
    return g_outside;
}
