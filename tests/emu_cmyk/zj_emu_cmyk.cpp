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

#include "../emu_common/zj_emu_arena.h"
#define ZJ_EXPAND_PUT(T, addr, v) emu_put<T>((addr), (v))

#include "../../zune-jpeg_amd/csrc/zj_cmyk.h"
#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

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
    if (n <= 0 || !stage_sizes((size_t)n, wh)) return -1;
    emu_arena(arena, len, map);
    CmykParams p{};
    stage_batches<CMYK_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_cmyk(p, a, k, wh, a_pitch, k_pitch, inverted, out, out_pitch, f0, m);
        if (chw) run<true>(p); else run<false>(p);
        return 0;
    });
    return g_outside;
}
