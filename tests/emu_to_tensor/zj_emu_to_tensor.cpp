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

static uint8_t* g_map = nullptr;     // one count per byte of [g_lo, g_hi)
static uint64_t g_lo = 0, g_hi = 0;
static long long g_outside = 0, g_bad_loads = 0;
// the image the running lane belongs to: its first byte, pitch, bytes of a row, rows
static uint64_t g_img = 0, g_pitch = 1, g_rowbytes = 0, g_rows = 0;

template <typename T>
static inline void emu_put(uint64_t a, T v)
{
    if (a < g_lo || a + sizeof(T) > g_hi) { g_outside++; return; }
    memcpy(reinterpret_cast<void*>((uintptr_t)a), &v, sizeof(T));
    for (size_t k = 0; k < sizeof(T); k++)
        if (g_map[a - g_lo + k] < 255) g_map[a - g_lo + k]++;
}
template <typename T>
static inline T emu_get(uint64_t a)
{
    T v{};
    const uint64_t off = a - g_img, row = a >= g_img ? off / g_pitch : g_rows;
    if (a < g_img || row >= g_rows || off - row * g_pitch + sizeof(T) > g_rowbytes || (a & (sizeof(T) - 1))) { g_bad_loads++; return v; }
    memcpy(&v, reinterpret_cast<const void*>((uintptr_t)a), sizeof(T));
    return v;
}
#define ZJ_TT_PUT(T, addr, v) emu_put<T>((addr), (v))
#define ZJ_TT_GET(T, addr) emu_get<T>((addr))

#include "../../zune-jpeg_amd/csrc/zj_to_tensor.h"

using namespace zj;

static void run(const ToTensorParams& p)
{
    const uint32_t gx = tt_grid(p);
    for (int z = 0; z < p.nimg; z++) {
        g_img = p.in[z]; g_pitch = p.pitch[z]; g_rowbytes = (uint64_t)p.w * p.cin; g_rows = (uint64_t)p.h;
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
    if (n <= 0 || w == 0 || h == 0 || w > 65535 || h > 65535 || !resize_elem_bytes(dtype)) return -1;
    if (!((cin == 1 && (cout == 1 || cout == 3)) || (cin == 3 && cout == 3))) return -1;
    g_map = map; g_lo = (uint64_t)(uintptr_t)arena; g_hi = g_lo + len; g_outside = 0; g_bad_loads = 0;
    const size_t img_bytes = (size_t)cout * w * h * (size_t)resize_elem_bytes(dtype);
    for (int f0 = 0; f0 < n; f0 += TT_BATCH) {
        ToTensorParams p{};
        p.nimg = n - f0 < TT_BATCH ? n - f0 : TT_BATCH;
        p.w = (int)w; p.h = (int)h; p.cin = cin; p.cout = cout; p.dtype = dtype; p.nhwc = nhwc ? 1 : 0;
        p.out = (uint64_t)(uintptr_t)(out + (size_t)f0 * img_bytes);
        for (int k = 0; k < 3; k++) { p.scale[k] = scale[k]; p.bias[k] = bias[k]; }
        for (int i = 0; i < p.nimg; i++) {
            p.in[i] = (uint64_t)(uintptr_t)in[f0 + i];
            p.pitch[i] = pitch[f0 + i];
            if (flip && flip[f0 + i]) p.flip[i >> 5] |= 1u << (i & 31);
        }
        run(p);
    }
    counts[0] = g_outside; counts[1] = g_bad_loads;
    return 0;
}
