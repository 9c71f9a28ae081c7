// zj_emu_resize_bicubic.cpp -- CPU EMULATION of the bicubic antialiased resize kernel
// (zune-jpeg_amd/csrc/zj_resize_bicubic.hip: zj_resize_bicubic_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_resize_aa: the kernel's ZJ_HD phases (zj_resize_bicubic.h) built by g++ with
// ZJ_EMU, every workgroup of the launch run phase by phase in the kernel's order, each phase for all of its lanes before the
// next (the kernel's barriers), the lanes' running sums kept per lane.  LDS is poisoned before every workgroup.  Never
// linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_resize_bicubic.h"

#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

#define LANES(...) for (int t = 0; t < AA_NT; t++) { __VA_ARGS__; }

extern "C" void zjeb_axis(uint32_t i, uint32_t n, uint32_t m, int* lo, int* hi)
{
    const BcAxis a = bc_axis(i, n, m);
    *lo = a.lo; *hi = a.hi;
}

// K'_j of every tap of destination index i, and their sum S
extern "C" long long zjeb_K(uint32_t i, uint32_t n, uint32_t m, int* Kp)
{
    const BcAxis a = bc_axis(i, n, m);
    long long S = 0;
    for (int j = a.lo; j <= a.hi; j++) S += (Kp[j - a.lo] = bc_K(a, j));
    return S;
}

extern "C" int zjeb_R(long long Cp, long long S) { return bc_R(Cp, S); }
extern "C" int zjeb_lds_bytes() { return (int)sizeof(BcShared); }

// stats[0]: final values clamped at 0, stats[1]: clamped at 255 x 2^16 (over every lane's live sums)
static long long g_clamped[2];

template <bool IN_CHW, int C, int DT, bool NHWC>
static void run(const ResizeParams& p)
{
    BcShared* const sp = new BcShared;
    BcShared& s = *sp;
    std::vector<BcLane> lanes(AA_NT);
    constexpr int PW = bc_piece_w<IN_CHW, C>();
    const long long img_bytes = (long long)C * p.out_h * p.out_w * resize_elem_bytes(DT);
    for (int img = 0; img < p.nimg; img++)
        for (int by = 0; by * AA_ROWS < p.out_h; by++)
            for (int bx = 0; bx * AA_COLS < p.out_w; bx++) {
                const AaBlock b = aa_block(p, img, bx, by, IN_CHW);
                uint8_t* const out = (uint8_t*)p.out + img * img_bytes;
                memset(sp, 0xA5, sizeof(BcShared));
                memset(lanes.data(), 0, lanes.size() * sizeof(BcLane));
                LANES(bc_axes_phase(b, s, t));
                LANES(bc_sum_phase(s.col, s.cpart, b.ncols, t); bc_sum_phase(s.row, s.rpart, b.nrows, t));
                LANES(bc_S_phase(s.col, s.cpart, b.ncols, t); bc_S_phase(s.row, s.rpart, b.nrows, t));
                int sx0, sx1;
                bc_span(b, s, sx0, sx1);
                const int rtaps = bc_row_taps(b, s);
                for (int px0 = sx0; px0 <= sx1; px0 += PW) {
                    const int px1 = sx1 + 1 - px0 < PW ? sx1 + 1 : px0 + PW;
                    LANES(bc_col_window_phase(b, s, px0, px1, t));
                    LANES(bc_col_offset_phase(b, s, t); bc_sum_phase(s.col, s.cpart, b.ncols, t));
                    LANES(bc_weights_phase(s.col, s.cpart, s.cw, b.ncols, t));
                    for (int j0 = 0; j0 < rtaps; j0 += BC_RCH) {
                        LANES(bc_row_window_phase(b, s, j0, t));
                        LANES(bc_sum_phase(s.row, s.rpart, b.nrows, t));
                        LANES(bc_weights_phase(s.row, s.rpart, s.rw, b.nrows, t));
                        LANES(for (int rr = 0; rr < b.nrows; rr++)
                                  bc_vertical_phase<IN_CHW, C>(b, s, lanes[t].v[rr], rr, px0, px1, t));
                    }
                    LANES(bc_vertical_store<IN_CHW, C>(b, s, lanes[t], px0, px1, t));
                    LANES(bc_carry_phase(s.col, s.cpart, b.ncols, t); bc_horizontal_phase<IN_CHW, C>(b, s, lanes[t], px0, t));
                }
                for (int t = 0; t < AA_NT; t++) {
                    int rr, k0;
                    const int cnt = aa_item(b, t, rr, k0);
                    for (int q = 0; q < cnt * C; q++) {
                        const long long v = (lanes[t].h[q] + 32) >> 6;
                        g_clamped[0] += v < 0;
                        g_clamped[1] += v > (255ll << 16);
                    }
                }
                LANES(bc_store_phase<C, DT, NHWC>(p, b, lanes[t], out, t));
            }
    delete sp;
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

// n images as the launches of the library's call (RESIZE_BATCH images each); wh: w, h pairs; s / b: the kernel's factors (s_c = scale_c * 2^-16);
// clamped (may be null): how many output values the final clamp cut at 0 and at 255 x 2^16
extern "C" int zjeb_resize(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, int channels, int in_chw,
                           int out_w, int out_h, int dtype, int nhwc, const float* s, const float* b, const uint8_t* flip,
                           uint8_t* out, long long* clamped)
{
    if (n <= 0 || (channels != 1 && channels != 3) || !resize_elem_bytes(dtype)) return -1;
    StageTensor t{out, (size_t)channels * out_w * out_h * (size_t)resize_elem_bytes(dtype), out_w, out_h, dtype, nhwc ? 1 : 0, {}, {}};
    for (int k = 0; k < 3; k++) { t.s[k] = s[k]; t.b[k] = b[k]; }
    ResizeParams p{};
    g_clamped[0] = g_clamped[1] = 0;
    const int rc = stage_batches<RESIZE_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_resize(p, in, wh, pitch, flip, t, 0, f0, m);
        if (channels == 1) return run_dt<false, 1, false>(dtype, p);
        if (in_chw) return nhwc ? run_dt<true, 3, true>(dtype, p) : run_dt<true, 3, false>(dtype, p);
        return nhwc ? run_dt<false, 3, true>(dtype, p) : run_dt<false, 3, false>(dtype, p);
    });
    if (clamped) { clamped[0] = g_clamped[0]; clamped[1] = g_clamped[1]; }
    return rc;
}
