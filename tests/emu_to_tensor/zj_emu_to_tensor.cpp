// zj_emu_to_tensor.cpp -- CPU EMULATION of the u8-images-to-tensor kernel (zune-jpeg_amd/csrc/zj_to_tensor.hip:
// zj_to_tensor_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_expand: the kernel's ZJ_HD functions (zj_to_tensor.h) built by g++ with ZJ_EMU,
// every lane of every workgroup of the launch's grid run one after the other.  Every store is counted in a write map over
// the caller's destination arena; a store that falls outside the arena is counted apart and NOT performed.  Every load is
// checked against the rows of the image the lane works on: one that touches a byte outside that image's h rows of
// w * in_channels bytes is counted apart and NOT performed (it yields 0).  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../emu_common/zj_emu_arena.h"
#define ZJ_TT_PUT(T, addr, v) emu_put<T>((addr), (v))
#define ZJ_TT_GET(T, addr) emu_get<T, true>((addr)) // (a load must lie on a boundary of its type)

#include "../../zune-jpeg_amd/csrc/zj_to_tensor.h"
#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

static void run(const ToTensorParams& p)
{
    const uint32_t gx = tt_grid(p);
    for (int z = 0; z < p.nimg; z++) {
        emu_image(p.in[z], p.pitch[z], (uint64_t)p.w * p.cin, (uint64_t)p.h);
        for (uint32_t bx = 0; bx < gx; bx++)
            for (int t = 0; t < TT_NT; t++) tt_lane(p, z, bx * (uint32_t)TT_NT + (uint32_t)t);
    }
}

extern "C" int zjtt_run(void) { return TT_RUN; }
extern "C" int zjtt_batch(void) { return TT_BATCH; }
extern "C" int zjtt_params_bytes(void) { return (int)sizeof(ToTensorParams); }

// n images of w x h as the launches of the library's call (TT_BATCH images each); scale / bias: the kernel's factors, 3
// each; pitch resolved; every destination byte must lie in [arena, arena + len): map gets the number of times each of
// them was stored.  counts[0]: stores that fell outside (not performed), counts[1]: loads outside the lane's image (not
// performed).  Returns 0, < 0: arguments
extern "C" int zjtt_to_tensor(int n, const uint8_t* const* in, unsigned w, unsigned h, const unsigned* pitch, int cin, int cout,
                              int dtype, int nhwc, const float* scale, const float* bias, const uint8_t* flip, uint8_t* out,
                              uint8_t* arena, size_t len, uint8_t* map, long long* counts)
{
    if (n <= 0 || !stage_size(w, h) || !resize_elem_bytes(dtype)) return -1;
    if (!((cin == 1 && (cout == 1 || cout == 3)) || (cin == 3 && cout == 3))) return -1;
    emu_arena(arena, len, map);
    StageTensor t{out, (size_t)cout * w * h * (size_t)resize_elem_bytes(dtype), (int)w, (int)h, dtype, nhwc ? 1 : 0, {}, {}};
    for (int k = 0; k < 3; k++) { t.s[k] = scale[k]; t.b[k] = bias[k]; }
    ToTensorParams p{};
    stage_batches<TT_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_to_tensor(p, in, pitch, flip, cin, cout, t, f0, m);
        run(p);
        return 0;
    });
    counts[0] = g_outside; counts[1] = g_bad_loads;
    return 0;
}
