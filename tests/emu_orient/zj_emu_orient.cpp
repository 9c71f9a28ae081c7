// zj_emu_orient.cpp -- CPU EMULATION of the orientation kernel (zune-jpeg_amd/csrc/zj_orient.hip: zj_orient_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_resize_aa: the kernel's ZJ_HD phases (zj_orient.h) built by g++ with ZJ_EMU, every
// workgroup of the launch run phase by phase, each phase for all of its lanes before the next (the kernel's barrier).  LDS is
// poisoned before every workgroup.  Every store is counted in a write map over the caller's destination arena; a store that
// falls outside the arena is counted apart and NOT performed.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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
#define ZJ_ORIENT_PUT(T, addr, v) emu_put<T>((addr), (v))

#include "../../zune-jpeg_amd/csrc/zj_orient.h"

using namespace zj;

template <int C, bool IN_CHW>
static void run(const OrientParams& p)
{
    constexpr int BPP = IN_CHW ? 1 : C, NPL = IN_CHW ? C : 1;
    std::vector<uint32_t> lds(orient_lds_bytes<BPP>() / 4);
    int gx, gy;
    orient_grid(p, &gx, &gy);
    for (int z = 0; z < p.nimg * NPL; z++)
        for (int by = 0; by < gy; by++)
            for (int bx = 0; bx < gx; bx++) {
                const int img = z / NPL, plane = z - img * NPL;
                const OrientBlock b = orient_block<BPP>(p, img, plane, bx, by);
                if (b.th == 0) continue;
                memset(lds.data(), 0xA5, lds.size() * 4);
                for (int t = 0; t < ORIENT_NT; t++) orient_load_phase<BPP>(b, lds.data(), t);
                for (int t = 0; t < ORIENT_NT; t++) orient_store_phase<BPP>(b, reinterpret_cast<const uint8_t*>(lds.data()), t);
            }
}

extern "C" int zjeo_tile(void) { return ORIENT_T; }
extern "C" int zjeo_batch(void) { return ORIENT_BATCH; }
extern "C" int zjeo_lds_bytes(int bpp) { return bpp == 3 ? orient_lds_bytes<3>() : orient_lds_bytes<1>(); }

// n images (n <= ORIENT_BATCH) as one launch; wh: STORED w, h pairs; every destination byte must lie in [arena, arena + len):
// map gets the number of times each of them was stored; returns the stores that fell outside (not performed), < 0: arguments
extern "C" long long zjeo_orient(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int channels,
                                 int in_chw, const uint8_t* o, uint8_t* const* out, const unsigned* out_pitch, uint8_t* arena,
                                 size_t len, uint8_t* map)
{
    if (n <= 0 || n > ORIENT_BATCH) return -1;
    OrientParams p{};
    p.nimg = n;
    for (int i = 0; i < n; i++) {
        if (!orient_valid(o[i])) return -1;
        p.in[i] = (uint64_t)(uintptr_t)in[i]; p.out[i] = (uint64_t)(uintptr_t)out[i];
        p.wh[i] = wh[2 * i] | (wh[2 * i + 1] << 16);
        p.in_pitch[i] = in_pitch[i]; p.out_pitch[i] = out_pitch[i];
        p.o[i] = o[i];
    }
    g_map = map; g_lo = (uint64_t)(uintptr_t)arena; g_hi = g_lo + len; g_outside = 0;
    if (channels == 1) run<1, false>(p);
    else if (channels == 3 && in_chw) run<3, true>(p);
    else if (channels == 3) run<3, false>(p);
    else return -1;
    return g_outside;
}
