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

static uint8_t *g_wmap = nullptr, *g_rmap = nullptr; // one count per byte of [g_wlo, g_whi) / [g_rlo, g_rhi)
static uint64_t g_wlo = 0, g_whi = 0, g_rlo = 0, g_rhi = 0;
static long long g_outside = 0;
template <typename T>
static inline void emu_put(uint64_t a, T v)
{
    if (a < g_wlo || a + sizeof(T) > g_whi) { g_outside++; return; }
    memcpy(reinterpret_cast<void*>((uintptr_t)a), &v, sizeof(T));
    for (size_t k = 0; k < sizeof(T); k++)
        if (g_wmap[a - g_wlo + k] < 255) g_wmap[a - g_wlo + k]++;
}
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
    if (n <= 0) return -1;
    g_wmap = wmap; g_wlo = (uint64_t)(uintptr_t)arena; g_whi = g_wlo + len;
    g_rmap = rmap; g_rlo = (uint64_t)(uintptr_t)src; g_rhi = g_rlo + src_len;
    g_outside = 0;
    for (int f0 = 0; f0 < n; f0 += COLOR_BATCH) {
        ColorParams p{};
        p.nimg = n - f0 < COLOR_BATCH ? n - f0 : COLOR_BATCH;
        for (int i = 0; i < p.nimg; i++) {
            const int f = f0 + i;
            if (wh[2 * f] == 0 || wh[2 * f + 1] == 0 || wh[2 * f] > 65535 || wh[2 * f + 1] > 65535) return -1;
            p.in[i] = (uint64_t)(uintptr_t)in[f]; p.out[i] = (uint64_t)(uintptr_t)out[f];
            p.wh[i] = wh[2 * f] | (wh[2 * f + 1] << 16);
            p.in_pitch[i] = in_pitch[f]; p.out_pitch[i] = out_pitch[f];
            for (int k = 0; k < 12; k++) p.q[i][k] = q[12 * f + k];
        }
        if (chw) run<true>(p); else run<false>(p);
    }
    return g_outside;
}
