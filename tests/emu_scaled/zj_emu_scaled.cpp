// zj_emu_scaled.cpp -- CPU EMULATION of the reduced-size decode's kernel (zj_scaled.hip: zj_scaled_kernel) and of its plan
// (zj_plan.h: make_scaled_plan, fill_scaled_params, prescale_pick, prescale_window).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_crop: every workgroup of a launch runs its phases thread by thread with the
// barriers between them, LDS being a host buffer filled with a poison first.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_plan.h"

using namespace zj;

template <int HS, int VS, int OUT, int SL>
static void run_scaled(const ScaledParams& p, uint8_t poison)
{
    using C = ScaledCfg<HS, VS, OUT, SL>;
    std::vector<char> mem(C::LDS + 32);
    char* lds = (char*)(((uintptr_t)mem.data() + 15) & ~(uintptr_t)15);
    for (int fz = 0; fz < p.nframes; fz++)
        for (int by = 0; by < p.nrows; by++)
            for (int bx = 0; bx < p.ncols; bx++) {
                ScaledTile t;
                if (!scaled_locate<C>(p, fz, by, bx, t)) continue;
                memset(lds, poison, C::LDS); // LDS holds whatever it held: what is copied must have been written
                std::vector<ScaledLoc> L(C::NT);
                std::vector<U4> raw((size_t)C::NT * 8);
                for (int tid = 0; tid < C::NT; tid++) {
                    L[tid] = scaled_block_loc<C, HS, VS>(p, t, tid, lds);
                    scaled_load<C>(L[tid], &raw[(size_t)tid * 8]);
                    scaled_setup<C>(p, tid, lds);
                }
                for (int tid = 0; tid < C::NT; tid++) scaled_finish<C, HS, VS>(L[tid], &raw[(size_t)tid * 8], lds, p.clamp_dc);
                for (int tid = 0; tid < C::NT; tid++) scaled_color<C, OUT>(t, tid, lds);
                for (int tid = 0; tid < C::NT; tid++) scaled_copyout<C>(p, t, tid, lds);
            }
}

static int dispatch(const Plan& pl, int sl, const ScaledParams& p, uint8_t poison)
{
#define ZJ_CASE1(H, V, O, L) if (pl.hs == H && pl.vs == V && pl.out == O && sl == L) { run_scaled<H, V, O, L>(p, poison); return ZJ_OK; }
#define ZJ_CASE(H, V, O) ZJ_CASE1(H, V, O, 1) ZJ_CASE1(H, V, O, 2) ZJ_CASE1(H, V, O, 3)
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR) ZJ_CASE(1, 1, OUT_RGB_CHW)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR) ZJ_CASE(2, 1, OUT_RGB_CHW)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR) ZJ_CASE(1, 2, OUT_RGB_CHW)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
#undef ZJ_CASE1
    return ZJ_ERR_UNSUPPORTED;
}

extern "C" int zjes_scaled_size(const zj_frame_desc* d, int sl, unsigned* w, unsigned* h)
{
    Plan pl;
    ScaledPlan sp;
    const int rc = make_scaled_plan(d, sl, pl, sp);
    if (rc) return rc;
    *w = (unsigned)sp.rw; *h = (unsigned)sp.rh;
    return ZJ_OK;
}

extern "C" size_t zjes_out_len(const zj_frame_desc* d, int sl, unsigned w, unsigned h, unsigned out_pitch)
{
    Plan pl;
    ScaledPlan sp;
    if (make_scaled_plan(d, sl, pl, sp)) return 0;
    return scaled_window_len(sp, 0, 0, w, h, out_pitch);
}

// zj_decode_crops_scaled_device's host side (argument checks, launches of up to SCATTER_MAX frames) over the emulated kernel
extern "C" int zjes_decode(const zj_frame_desc* d, size_t nframes, const int16_t* const* y, const int16_t* const* cb,
                           const int16_t* const* cr, int sl, const unsigned* win, uint8_t* const* out, unsigned out_pitch,
                           int poison)
{
    Plan pl;
    ScaledPlan sp;
    int rc = make_scaled_plan(d, sl, pl, sp);
    if (rc) return rc;
    if (nframes == 0) return ZJ_ERR_ARG;
    for (size_t f = 0; f < nframes; f++) {
        const unsigned whole[4] = {0, 0, (unsigned)sp.rw, (unsigned)sp.rh};
        const unsigned* w = win ? win + 4 * f : whole;
        if (!scaled_window_len(sp, w[0], w[1], w[2], w[3], out_pitch)) return ZJ_ERR_ARG;
    }
    if (sp.zero) {
        for (size_t f = 0; f < nframes; f++) {
            const int w = win ? (int)win[4 * f + 2] : sp.rw, h = win ? (int)win[4 * f + 3] : sp.rh;
            const size_t pitch = out_pitch ? out_pitch : (size_t)w * sp.bpp;
            for (int r = 0; r < h * sp.nplanes; r++) memset(out[f] + r * pitch, 0, (size_t)w * sp.bpp);
        }
        return ZJ_OK;
    }
    const bool chroma = pl.out != OUT_GRAY;
    for (size_t f0 = 0; f0 < nframes; f0 += SCATTER_MAX) {
        const int n = (int)(nframes - f0 < (size_t)SCATTER_MAX ? nframes - f0 : (size_t)SCATTER_MAX);
        static ScaledParams p;
        fill_scaled_params(d, pl, sp, y, chroma ? cb : nullptr, chroma ? cr : nullptr, out, win, out_pitch, f0, n, p);
        if ((rc = dispatch(pl, sl, p, (uint8_t)poison))) return rc;
    }
    return ZJ_OK;
}

extern "C" int zjes_prescale_pick(unsigned w, unsigned h, unsigned out_w, unsigned out_h, int max_log2)
{
    return prescale_pick(w, h, out_w, out_h, max_log2);
}

extern "C" void zjes_prescale_window(const unsigned full[4], int k, unsigned width, unsigned height, unsigned red[4])
{
    prescale_window(full, k, width, height, red);
}
