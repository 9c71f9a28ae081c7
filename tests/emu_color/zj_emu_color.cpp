// zj_emu_color.cpp -- CPU EMULATION of the colour-matrix kernel (zune-jpeg_amd/csrc/zj_color.hip: zj_color_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_cmyk: the kernel's ZJ_HD functions (zj_color.h) built by g++ with ZJ_EMU, every
// lane of every workgroup of the launch's grid run one after the other.  Every store is counted in a write map over the
// caller's destination arena, every load in a read map over the caller's source arena; a store or a load that falls outside
// its arena is counted apart and NOT performed (the load yields 0).  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../emu_common/zj_emu_arena.h"

static uint8_t* g_rmap = nullptr; // one count per byte of [g_rlo, g_rhi)
static uint64_t g_rlo = 0, g_rhi = 0;
#define ZJ_EXPAND_PUT(T, addr, v) emu_put<T>((addr), (v))

// a load of the kernel: the address it may read from, counted; outside the source arena: zeros, counted apart
static const uint8_t g_zero[16] __attribute__((aligned(16))) = {0};
template <typename T>
static inline T* emu_at(uint64_t a)
{
    if (a < g_rlo || a + sizeof(T) > g_rhi) { g_outside++; return reinterpret_cast<T*>(const_cast<uint8_t*>(g_zero)); }
    for (size_t k = 0; k < sizeof(T); k++)
        if (g_rmap[a - g_rlo + k] < 255) g_rmap[a - g_rlo + k]++;
    return reinterpret_cast<T*>((uintptr_t)a);
}

#include "../../zune-jpeg_amd/csrc/zj_resize.h"
// (every load of zj_color.h goes through cmyk_get, which forms its addresses with this macro; the stores go through
// ZJ_EXPAND_PUT above)
#undef ZJ_RZ_GLOBAL
#define ZJ_RZ_GLOBAL(T, v) (emu_at<T>((uint64_t)(v)))
#include "../../zune-jpeg_amd/csrc/zj_color.h"
// (the other stages' headers, which come with zj_stage_pack.h and are not run here, load as they are written)
#undef ZJ_RZ_GLOBAL
#define ZJ_RZ_GLOBAL(T, v) (reinterpret_cast<T*>(v))
#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

template <bool CHW>
static void run(const ColorParams& p)
{
    const int gx = color_grid(p);
    for (int z = 0; z < p.nimg; z++)
        for (int bx = 0; bx < gx; bx++)
            for (int t = 0; t < COLOR_NT; t++) color_lane<CHW>(p, z, (uint32_t)bx * COLOR_NT + (uint32_t)t);
}

extern "C" int zjcl_run(void) { return COLOR_RUN; }
extern "C" int zjcl_batch(void) { return COLOR_BATCH; }
extern "C" int zjcl_params_bytes(void) { return (int)sizeof(ColorParams); }

// the host-side rule (zj_color_fixed.h): 1 and the 12 integers, or 0: a matrix the stage refuses
extern "C" int zjcl_fixed(const double* m, int32_t* q) { return color_fixed(m, q) ? 1 : 0; }

// n images as the launches of the library's call (COLOR_BATCH images each); wh: w, h pairs; q: 12 integers per image.  Every
// source byte must lie in [src, src + src_len), every destination byte in [arena, arena + len) (in place: the same range):
// rmap / wmap get the number of times each byte was loaded / stored; returns the loads and stores that fell outside (not
// performed), < 0: arguments
extern "C" long long zjcl_color(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int chw, const int32_t* q,
                                uint8_t* const* out, const unsigned* out_pitch, const uint8_t* src, size_t src_len, uint8_t* rmap,
                                uint8_t* arena, size_t len, uint8_t* wmap)
{
    if (n <= 0 || !stage_sizes((size_t)n, wh)) return -1;
    emu_arena(arena, len, wmap);
    g_rmap = rmap; g_rlo = (uint64_t)(uintptr_t)src; g_rhi = g_rlo + src_len;
    ColorParams p{};
    stage_batches<COLOR_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_color(p, in, wh, in_pitch, q, out, out_pitch, f0, m);
        if (chw) run<true>(p); else run<false>(p);
        return 0;
    });
    return g_outside;
}
