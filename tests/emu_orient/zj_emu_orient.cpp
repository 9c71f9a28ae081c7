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

#include "../emu_common/zj_emu_arena.h"
#define ZJ_ORIENT_PUT(T, addr, v) emu_put<T>((addr), (v))

#include "../../zune-jpeg_amd/csrc/zj_orient.h"
#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

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

// n images as the launches of the library's call (ORIENT_BATCH images each); wh: STORED w, h pairs; every destination byte must
// lie in [arena, arena + len): map gets the number of times each of them was stored; returns the stores that fell outside (not
// performed), < 0: arguments
extern "C" long long zjeo_orient(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int channels,
                                 int in_chw, const uint8_t* o, uint8_t* const* out, const unsigned* out_pitch, uint8_t* arena,
                                 size_t len, uint8_t* map)
{
    if (n <= 0 || (channels != 1 && channels != 3)) return -1;
    for (int i = 0; i < n; i++)
        if (!orient_valid(o[i])) return -1;
    emu_arena(arena, len, map);
    OrientParams p{};
    stage_batches<ORIENT_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_orient(p, in, wh, in_pitch, o, out, out_pitch, f0, m);
        if (channels == 1) run<1, false>(p);
        else if (in_chw) run<3, true>(p);
        else run<3, false>(p);
        return 0;
    });
    return g_outside;
}
