// zj_emu_resize_aa.cpp -- CPU EMULATION of the antialiased resize kernel (zune-jpeg_amd/csrc/zj_resize_aa.hip:
// zj_resize_aa_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_resize: the kernel's ZJ_HD phases (zj_resize_aa.h) built by g++ with ZJ_EMU, every
// workgroup of the launch run phase by phase, each phase for all of its lanes before the next (the kernel's barriers), the
// lanes' running sums kept per lane.  LDS is poisoned before every workgroup.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_resize_aa.h"

#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

extern "C" uint32_t zjea_weight(uint32_t i, uint32_t n, uint32_t m, int j) { return aa_weight(aa_axis(i, n, m), j); }
extern "C" void zjea_axis(uint32_t i, uint32_t n, uint32_t m, int* lo, int* hi, unsigned long long* S)
{
    const AaAxis a = aa_axis(i, n, m);
    *lo = a.lo; *hi = a.hi; *S = a.S;
}

template <bool IN_CHW, int C, int DT, bool NHWC>
static void run(const ResizeParams& p)
{
    AaShared* const s = new AaShared;
    std::vector<AaLane> lanes(AA_NT);
    constexpr int PW = aa_piece_w<IN_CHW, C>();
    const long long img_bytes = (long long)C * p.out_h * p.out_w * resize_elem_bytes(DT);
    for (int img = 0; img < p.nimg; img++)
        for (int by = 0; by * AA_ROWS < p.out_h; by++)
            for (int bx = 0; bx * AA_COLS < p.out_w; bx++) {
                const AaBlock b = aa_block(p, img, bx, by, IN_CHW);
                uint8_t* const out = (uint8_t*)p.out + img * img_bytes;
                memset(s, 0xA5, sizeof(AaShared));
                memset(lanes.data(), 0, lanes.size() * sizeof(AaLane));
                for (int t = 0; t < AA_NT; t++) aa_col_axes_phase(b, *s, t);
                int sx0, sx1;
                aa_span(b, *s, sx0, sx1);
                for (int px0 = sx0; px0 <= sx1; px0 += PW) {
                    const int px1 = sx1 + 1 - px0 < PW ? sx1 + 1 : px0 + PW;
                    for (int t = 0; t < AA_NT; t++) aa_col_count_phase(b, *s, px0, px1, t);
                    for (int t = 0; t < AA_NT; t++) aa_col_offset_phase(b, *s, t);
                    for (int t = 0; t < AA_NT; t++) aa_col_weights_phase(b, *s, t);
                    for (int rr = 0; rr < b.nrows; rr++) {
                        const AaAxis ra = aa_axis((uint32_t)(b.r0 + rr), (uint32_t)b.n_h, (uint32_t)b.oh);
                        const int ntaps = ra.hi - ra.lo + 1;
                        for (int j0 = 0; j0 < ntaps; j0 += AA_NT) {
                            for (int t = 0; t < AA_NT; t++) aa_row_weights_phase(ra, *s, j0, t);
                            for (int t = 0; t < AA_NT; t++)
                                aa_vertical_phase<IN_CHW, C>(b, *s, lanes[t], ra.lo, j0, ntaps - j0 < AA_NT ? ntaps - j0 : AA_NT,
                                                             px0, px1, t);
                        }
                        for (int t = 0; t < AA_NT; t++) aa_vertical_store<IN_CHW, C>(*s, lanes[t], rr, px0, px1, t);
                    }
                    for (int t = 0; t < AA_NT; t++) aa_horizontal_phase<IN_CHW, C>(b, *s, lanes[t], px0, t);
                }
                for (int t = 0; t < AA_NT; t++) aa_store_phase<C, DT, NHWC>(p, b, lanes[t], out, t);
            }
    delete s;
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
extern "C" int zjea_resize(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, int channels, int in_chw,
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
