// zj_emu_warp.cpp -- CPU EMULATION of the affine-warp kernels (zune-jpeg_amd/csrc/zj_warp.hip: zj_warp_kernel<C>).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_to_tensor: the kernel's ZJ_HD functions (zj_warp.h) built by g++ with ZJ_EMU,
// every lane of every workgroup of the launch's grid run one after the other.  Every store is counted in a write map over
// the caller's destination arena; a store that falls outside the arena is counted apart and NOT performed.  Every load is
// checked against the rows of the image the lane works on: one that touches a byte outside that image's h rows of
// w * channels bytes is counted apart and NOT performed (it yields 0).  The host-side rules (zj_warp_fixed.h) are exposed
// as they are.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../emu_common/zj_emu_arena.h"
#define ZJ_WP_PUT(T, addr, v) emu_put<T, true>((addr), (v)) // (a store must lie on a boundary of its type)
#define ZJ_WP_GET(T, addr) emu_get<T, false>((addr))

#include "../../zune-jpeg_amd/csrc/zj_warp.h"
#include "../../zune-jpeg_amd/csrc/zj_warp_fixed.h"
#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

template <int C>
static void run(const WarpParams& p)
{
    const uint32_t gx = warp_grid_x(p.out_w), gy = warp_grid_y(p.out_h);
    for (int z = 0; z < p.nimg; z++) {
        emu_image(p.img[z].in, p.img[z].pitch, (uint64_t)(p.img[z].wh & 0xffffu) * C, (uint64_t)(p.img[z].wh >> 16));
        for (uint32_t by = 0; by < gy; by++)
            for (uint32_t bx = 0; bx < gx; bx++)
                for (uint32_t t = 0; t < (uint32_t)WARP_NT; t++) warp_lane<C>(p, z, bx, by, t);
    }
}

extern "C" int zjew_group(void) { return WARP_GROUP; }
extern "C" int zjew_batch(void) { return WARP_BATCH; }
extern "C" int zjew_block_rows(void) { return WARP_BY; }
extern "C" int zjew_params_bytes(void) { return (int)sizeof(WarpParams); }
extern "C" int zjew_fixed(const double* m, int64_t* q) { return warp_fixed(m, q) ? 0 : -1; }
extern "C" void zjew_window(const int64_t* q, unsigned fw, unsigned fh, unsigned ow, unsigned oh, int edge, unsigned* win, int64_t* shifted)
{
    warp_source_window(q, fw, fh, ow, oh, edge == WARP_REPLICATE, win, shifted);
}

// n images as the launches of the library's call (WARP_BATCH images each); wh: w, h pairs; ints: 6 per image; scale / bias:
// the kernel's factors, 3 each; fill: 3 bytes; every destination byte must lie in [arena, arena + len): map gets the number
// of times each of them was stored.  counts[0]: stores that fell outside (not performed), counts[1]: loads outside the
// lane's image (not performed), counts[2]: loads.  Returns 0, < 0: arguments
extern "C" int zjew_warp(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, int channels, const int64_t* ints,
                         int out_w, int out_h, int dtype, int nhwc, const float* scale, const float* bias, const uint8_t* fill,
                         int edge, uint8_t* out, uint8_t* arena, size_t len, uint8_t* map, long long* counts)
{
    if (n <= 0 || out_w <= 0 || out_h <= 0 || out_w > RESIZE_MAX_OUT || out_h > RESIZE_MAX_OUT || !resize_elem_bytes(dtype)) return -1;
    if ((channels != 1 && channels != 3) || (edge != WARP_FILL && edge != WARP_REPLICATE)) return -1;
    if (!stage_sizes((size_t)n, wh)) return -1; // (no empty window here: every image is one)
    emu_arena(arena, len, map);
    StageTensor t{out, (size_t)channels * out_w * out_h * (size_t)resize_elem_bytes(dtype), out_w, out_h, dtype, nhwc ? 1 : 0, {}, {}};
    for (int k = 0; k < 3; k++) { t.s[k] = scale[k]; t.b[k] = bias[k]; }
    WarpParams p{};
    stage_batches<WARP_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_warp(p, in, wh, pitch, ints, warp_fill(fill, 3), edge, t, 0, f0, m);
        if (channels == 1) run<1>(p); else run<3>(p);
        return 0;
    });
    counts[0] = g_outside; counts[1] = g_bad_loads; counts[2] = g_loads;
    return 0;
}
