// zj_emu_resize.cpp -- CPU EMULATION of the resize kernel (zune-jpeg_amd/csrc/zj_resize.hip: zj_resize_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_crop: the kernel's ZJ_HD functions (zj_resize.h) built by g++ with ZJ_EMU, each
// workgroup's tap tables filled and each lane's group run as the kernel does.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_resize.h"

#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

extern "C" uint32_t zjer_tap(uint32_t i, uint32_t n, uint32_t m) { return resize_tap(i, n, m); }
extern "C" uint32_t zjer_value(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t fx, uint32_t fy)
{
    return resize_value(p00, p01, p10, p11, fx, fy);
}
extern "C" float zjer_f32(uint32_t v, float s, float b) { return resize_f32(v, s, b); }
extern "C" uint32_t zjer_f16(float y) { return resize_f16_bits(y); }
extern "C" uint32_t zjer_bf16(float y) { return resize_bf16_bits(y); }

template <bool IN_CHW, int C, int DT, bool NHWC>
static void run(const ResizeParams& p)
{
    std::vector<uint32_t> ctap(p.out_w), rtap(p.rows);
    for (int img = 0; img < p.nimg; img++) {
        const uint32_t n_w = p.wh[img] & 0xffffu, n_h = p.wh[img] >> 16;
        const bool flip = (p.flip[img >> 5] >> (img & 31)) & 1u;
        const long long img_bytes = (long long)C * p.out_h * p.out_w * resize_elem_bytes(DT);
        uint8_t* const out = (uint8_t*)p.out + img * img_bytes;
        for (int r0 = 0; r0 < p.out_h; r0 += p.rows) {
            for (int i = 0; i < p.out_w; i++) ctap[i] = resize_tap((uint32_t)(flip ? p.out_w - 1 - i : i), n_w, (uint32_t)p.out_w);
            const int nr = p.out_h - r0 < p.rows ? p.out_h - r0 : p.rows;
            for (int i = 0; i < nr; i++) rtap[i] = resize_tap((uint32_t)(r0 + i), n_h, (uint32_t)p.out_h);
            for (int it = 0; it < nr * p.groups; it++) {
                const int rr = it / p.groups, g = it - rr * p.groups, x0 = g * RESIZE_GROUP;
                resize_group<IN_CHW, C, DT, NHWC>(p, (const uint8_t*)p.in[img], (int)p.pitch[img], (int)n_h, ctap.data() + x0,
                                                  rtap[rr], r0 + rr, x0, out);
            }
        }
    }
}

template <bool IN_CHW, int C, bool NHWC>
static int run_dt(int dt, const ResizeParams& p)
{
    switch (dt) {
    case RZ_F32: run<IN_CHW, C, RZ_F32, NHWC>(p); return 0;
    case RZ_F16: run<IN_CHW, C, RZ_F16, NHWC>(p); return 0;
    case RZ_BF16: run<IN_CHW, C, RZ_BF16, NHWC>(p); return 0;
    case RZ_U8: run<IN_CHW, C, RZ_U8, NHWC>(p); return 0;
    }
    return -1;
}

// n images as the launches of the library's call (RESIZE_BATCH images each); wh: w, h pairs; s / b: the kernel's factors (s_c = scale_c * 2^-16)
extern "C" int zjer_resize(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, int channels, int in_chw,
                           int out_w, int out_h, int dtype, int nhwc, const float* s, const float* b, const uint8_t* flip,
                           uint8_t* out)
{
    if (n <= 0 || (channels != 1 && channels != 3) || !resize_elem_bytes(dtype)) return -1;
    StageTensor t{out, (size_t)channels * out_w * out_h * (size_t)resize_elem_bytes(dtype), out_w, out_h, dtype, nhwc ? 1 : 0, {}, {}};
    for (int k = 0; k < 3; k++) { t.s[k] = s[k]; t.b[k] = b[k]; }
    ResizeParams p{};
    const int rc = stage_batches<RESIZE_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_resize(p, in, wh, pitch, flip, t, 0, f0, m);
        if (channels == 1) return run_dt<false, 1, false>(dtype, p);
        if (in_chw) return nhwc ? run_dt<true, 3, true>(dtype, p) : run_dt<true, 3, false>(dtype, p);
        return nhwc ? run_dt<false, 3, true>(dtype, p) : run_dt<false, 3, false>(dtype, p);
    });
    return rc;
}
