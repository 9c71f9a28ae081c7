// zj_emu_cmyk.cpp -- CPU EMULATION of the CMYK-to-RGB kernel (zune-jpeg_amd/csrc/zj_cmyk.hip: zj_cmyk_combine_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_expand: the kernel's ZJ_HD functions (zj_cmyk.h) built by g++ with ZJ_EMU, every
// lane of every workgroup of the launch's grid run one after the other.  Every store is counted in a write map over the
// caller's destination arena; a store that falls outside the arena is counted apart and NOT performed.  Never linked into
// libzjhip.so.
#define ZJ_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static uint8_t* g_map = nullptr;     // one count per byte of [g_lo, g_hi)
static uint64_t g_lo = 0, g_hi = 0;
static long long g_outside = 0;
template <typename T>
static inline void emu_put(uint64_t a, T v)
{
    if (a < g_lo || a + sizeof(T) > g_hi) { g_outside++; return; }
    memcpy(reinterpret_cast<void*>((uintptr_t)a), &v, sizeof(T));
    for (size_t k = 0; k < sizeof(T); k++)
        if (g_map[a - g_lo + k] < 255) g_map[a - g_lo + k]++;
}
#define ZJ_EXPAND_PUT(T, addr, v) emu_put<T>((addr), (v))

#include "../../zune-jpeg_amd/csrc/zj_cmyk.h"

using namespace zj;

template <bool CHW>
static void run(const CmykParams& p)
{
    const int gx = cmyk_grid(p);
    for (int z = 0; z < p.nimg; z++)
        for (int bx = 0; bx < gx; bx++)
            for (int t = 0; t < CMYK_NT; t++) cmyk_lane<CHW>(p, z, (uint32_t)bx * CMYK_NT + (uint32_t)t);
}

extern "C" int zjck_run(void) { return CMYK_RUN; }
extern "C" int zjck_batch(void) { return CMYK_BATCH; }
extern "C" int zjck_params_bytes(void) { return (int)sizeof(CmykParams); }

// n image pairs as the launches of the library's call (CMYK_BATCH pairs each); wh: w, h pairs; every destination byte must lie
// in [arena, arena + len): map gets the number of times each of them was stored; returns the stores that fell outside (not
// performed), < 0: arguments
extern "C" long long zjck_combine(int n, const uint8_t* const* a, const uint8_t* const* k, const unsigned* wh, const unsigned* a_pitch,
                                  const unsigned* k_pitch, int chw, const uint8_t* inverted, uint8_t* const* out,
                                  const unsigned* out_pitch, uint8_t* arena, size_t len, uint8_t* map)
{
    if (n <= 0) return -1;
    g_map = map; g_lo = (uint64_t)(uintptr_t)arena; g_hi = g_lo + len; g_outside = 0;
    for (int f0 = 0; f0 < n; f0 += CMYK_BATCH) {
        CmykParams p{};
        p.nimg = n - f0 < CMYK_BATCH ? n - f0 : CMYK_BATCH;
        for (int i = 0; i < p.nimg; i++) {
            const int f = f0 + i;
            if (wh[2 * f] == 0 || wh[2 * f + 1] == 0 || wh[2 * f] > 65535 || wh[2 * f + 1] > 65535) return -1;
            p.a[i] = (uint64_t)(uintptr_t)a[f]; p.k[i] = (uint64_t)(uintptr_t)k[f]; p.out[i] = (uint64_t)(uintptr_t)out[f];
            p.wh[i] = wh[2 * f] | (wh[2 * f + 1] << 16);
            p.a_pitch[i] = a_pitch[f]; p.k_pitch[i] = k_pitch[f]; p.out_pitch[i] = out_pitch[f];
            if (inverted[f]) p.inverted[i >> 5] |= 1u << (i & 31);
        }
        if (chw) run<true>(p); else run<false>(p);
    }
    return g_outside;
}
