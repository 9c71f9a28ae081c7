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

static uint8_t* g_map = nullptr;     // one count per byte of [g_lo, g_hi)
static uint64_t g_lo = 0, g_hi = 0;
static long long g_outside = 0, g_bad_loads = 0, g_loads = 0;
// the image the running lane belongs to: its first byte, pitch, bytes of a row, rows
static uint64_t g_img = 0, g_pitch = 1, g_rowbytes = 0, g_rows = 0;

template <typename T>
static inline void emu_put(uint64_t a, T v)
{
    if (a < g_lo || a + sizeof(T) > g_hi || (a & (sizeof(T) - 1))) { g_outside++; return; }
    memcpy(reinterpret_cast<void*>((uintptr_t)a), &v, sizeof(T));
    for (size_t k = 0; k < sizeof(T); k++)
        if (g_map[a - g_lo + k] < 255) g_map[a - g_lo + k]++;
}
template <typename T>
static inline T emu_get(uint64_t a)
{
    T v{};
    g_loads++;
    const uint64_t off = a - g_img, row = a >= g_img ? off / g_pitch : g_rows;
    if (a < g_img || row >= g_rows || off - row * g_pitch + sizeof(T) > g_rowbytes) { g_bad_loads++; return v; }
    memcpy(&v, reinterpret_cast<const void*>((uintptr_t)a), sizeof(T));
    return v;
}
#define ZJ_WP_PUT(T, addr, v) emu_put<T>((addr), (v))
#define ZJ_WP_GET(T, addr) emu_get<T>((addr))

#include "../../zune-jpeg_amd/csrc/zj_warp.h"
#include "../../zune-jpeg_amd/csrc/zj_warp_fixed.h"

using namespace zj;

template <int C>
static void run(const WarpParams& p)
{
    const uint32_t gx = warp_grid_x(p.out_w), gy = warp_grid_y(p.out_h);
    for (int z = 0; z < p.nimg; z++) {
        g_img = p.img[z].in; g_pitch = p.img[z].pitch;
        g_rowbytes = (uint64_t)(p.img[z].wh & 0xffffu) * C; g_rows = (uint64_t)(p.img[z].wh >> 16);
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
    g_map = map; g_lo = (uint64_t)(uintptr_t)arena; g_hi = g_lo + len; g_outside = 0; g_bad_loads = 0; g_loads = 0;
    const size_t img_bytes = (size_t)channels * out_w * out_h * (size_t)resize_elem_bytes(dtype);
    for (int f0 = 0; f0 < n; f0 += WARP_BATCH) {
        WarpParams p{};
        p.nimg = n - f0 < WARP_BATCH ? n - f0 : WARP_BATCH;
        p.out_w = out_w; p.out_h = out_h; p.dtype = dtype; p.nhwc = nhwc ? 1 : 0; p.edge = edge;
        p.fill = (uint32_t)fill[0] | (uint32_t)fill[1] << 8 | (uint32_t)fill[2] << 16;
        p.out = (uint64_t)(uintptr_t)(out + (size_t)f0 * img_bytes);
        for (int k = 0; k < 3; k++) { p.scale[k] = scale[k]; p.bias[k] = bias[k]; }
        for (int i = 0; i < p.nimg; i++) {
            const int f = f0 + i;
            if (wh[2 * f] == 0 || wh[2 * f + 1] == 0 || wh[2 * f] > 65535 || wh[2 * f + 1] > 65535) return -1;
            p.img[i].in = (uint64_t)(uintptr_t)in[f];
            p.img[i].wh = wh[2 * f] | wh[2 * f + 1] << 16;
            p.img[i].pitch = pitch[f];
            for (int k = 0; k < 6; k++) p.img[i].m[k] = ints[6 * f + k];
        }
        if (channels == 1) run<1>(p); else run<3>(p);
    }
    counts[0] = g_outside; counts[1] = g_bad_loads; counts[2] = g_loads;
    return 0;
}
