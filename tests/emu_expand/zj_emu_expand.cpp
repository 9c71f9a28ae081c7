// zj_emu_expand.cpp -- CPU EMULATION of the gray-to-RGB kernel (zune-jpeg_amd/csrc/zj_expand.hip: zj_gray_expand_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_orient: the kernel's ZJ_HD functions (zj_expand.h) built by g++ with ZJ_EMU, every
// lane of every workgroup of the launch's grid run one after the other.  Every store is counted in a write map over the
// caller's destination arena; a store that falls outside the arena is counted apart and NOT performed.  Never linked into
// libzjhip.so.
#define ZJ_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../emu_common/zj_emu_arena.h"
#define ZJ_EXPAND_PUT(T, addr, v) emu_put<T>((addr), (v))

#include "../../zune-jpeg_amd/csrc/zj_expand.h"
#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

template <bool OUT_CHW>
static void run(const ExpandParams& p)
{
    const int gx = expand_grid(p);
    for (int z = 0; z < p.nimg; z++)
        for (int bx = 0; bx < gx; bx++)
            for (int t = 0; t < EXPAND_NT; t++) expand_lane<OUT_CHW>(p, z, (uint32_t)bx * EXPAND_NT + (uint32_t)t);
}

extern "C" int zjex_run(void) { return EXPAND_RUN; }
extern "C" int zjex_batch(void) { return EXPAND_BATCH; }
extern "C" int zjex_params_bytes(void) { return (int)sizeof(ExpandParams); }

// n planes as the launches of the library's call (EXPAND_BATCH images each); wh: w, h pairs; every destination byte must lie
// in [arena, arena + len): map gets the number of times each of them was stored; returns the stores that fell outside (not
// performed), < 0: arguments
extern "C" long long zjex_expand(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int out_chw,
                                 uint8_t* const* out, const unsigned* out_pitch, uint8_t* arena, size_t len, uint8_t* map)
{
    if (n <= 0 || !stage_sizes((size_t)n, wh)) return -1;
    emu_arena(arena, len, map);
    ExpandParams p{};
    stage_batches<EXPAND_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_expand(p, in, wh, in_pitch, out, out_pitch, f0, m);
        if (out_chw) run<true>(p); else run<false>(p);
        return 0;
    });
    return g_outside;
}
