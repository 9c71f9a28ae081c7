// zj_emu_crop_tensor.cpp -- CPU EMULATION of the crop-to-tensor kernels (zj_crop_tensor.hip: zj_fused_crop_tensor_kernel,
// zj_crop_zero_tensor_kernel) over the launch arguments the library's host side builds (zj_crop_tensor.h, zj_plan.h).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_crop: every workgroup of a launch runs its phases thread by thread with the
// barriers between them, LDS and the staging being host buffers filled with a poison first.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_mixed.h"
#include "../../zune-jpeg_amd/csrc/zj_crop_tensor.h"

using namespace zj;

// one crop workgroup's tile decode into the staging (the kernel up to its last barrier; tests/emu_crop)
template <int HS, int VS, int OUT>
static void tile_to_stage(const Params& p, const TileId& t, char* lds)
{
    using C = Cfg<HS, VS, OUT>;
    constexpr bool NEED_Y16 = OUT == OUT_RGB;
    memset(lds, 0x7B, C::LDS_PACKED);
    for (int tid = 0; tid < C::NT; tid++) phase_setup<C, HS, VS, GEN_PACKED>(p, tid, lds);
    const int nblock_lanes = C::HALO_PURE ? C::HALO_T0 : C::NT;
    for (int tid = 0; tid < nblock_lanes; tid++) {
        const BlockLoc L = locate<C, GEN_PACKED>(p, t, tid, lds);
        U4 raw[8];
        load_block(L, raw);
        finish_block<C, GEN_PACKED, NEED_Y16>(L, raw, lds, 0, p.clamp_dc);
    }
    if (C::HALO_PURE) {
        HaloLane H[64];
        for (int hl = 0; hl < 64; hl++) {
            H[hl] = halo_locate<C>(p, t, hl, lds);
            int32_t s8[8];
            halo_load(H[hl], s8);
            halo_pass1<C>(H[hl], s8, lds);
        }
        for (int hl = 0; hl < 64; hl++) halo_pass2<C>(H[hl], lds, p.clamp_dc);
        for (int hl = 0; hl < 64; hl++) halo_filter<C, HS, VS>(p, t, hl, lds);
    }
    if (NEED_Y16 && *lds_flag<C>(lds) != 0) {
        memset(lds, 0x7B, C::LDS_PACKED);
        for (int tid = 0; tid < C::NT; tid++) phase_setup<C, HS, VS, GEN_WIDE>(p, tid, lds);
        for (int tid = 0; tid < C::NT; tid++) {
            const BlockLoc L = locate<C, GEN_WIDE>(p, t, tid, lds);
            U4 raw[8];
            load_block(L, raw);
            finish_block<C, GEN_WIDE, false>(L, raw, lds, 0, p.clamp_dc);
        }
        for (int tid = 0; tid < C::NT; tid++) phase_color<C, HS, VS, OUT, GEN_WIDE, false, false, false>(p, t, tid, lds);
        return;
    }
    for (int tid = 0; tid < C::NT; tid++) phase_color<C, HS, VS, OUT, GEN_PACKED, false, false, false>(p, t, tid, lds);
}

// zj_fused_crop_tensor_kernel over a grid of ncols x nstrips x (nrec << shift): blockIdx.z >> shift picks the record of the
// table, the low bits the frame in it
template <int HS, int VS, int OUT>
static void run_crop_tensor(const CropTensorParams* tab, int nrec, int shift, int ncols, int nstrips, uint8_t stage_poison)
{
    using C = Cfg<HS, VS, OUT>;
    using S = CropStage<HS, VS, OUT>;
    std::vector<char> lds_mem(C::LDS_PACKED + 32), stage_mem(S::BYTES + 32);
    char* lds = (char*)(((uintptr_t)lds_mem.data() + 15) & ~(uintptr_t)15);
    uint8_t* stage = (uint8_t*)(((uintptr_t)stage_mem.data() + 15) & ~(uintptr_t)15);
    for (int bz = 0; bz < (nrec << shift); bz++)
        for (int sy = 0; sy < nstrips; sy++)
            for (int sx = 0; sx < ncols; sx++) {
                const CropTensorParams& tp = tab[bz >> shift];
                const int fz = bz & ((1 << shift) - 1);
                const CropParams& cp = tp.cp;
                const Params& p = cp.p;
                CropSpan s;
                if (!crop_locate<HS, VS, OUT>(cp, fz, sy, sx, s)) continue;
                memset(stage, stage_poison, S::BYTES); // LDS holds whatever it held: what is converted must have been written
                TileId t;
                t.frame = s.frame; t.strip = s.strip; t.tile = s.tile;
                t.y = (const int16_t*)p.fptr[fz][0]; t.cb = (const int16_t*)p.fptr[fz][1]; t.cr = (const int16_t*)p.fptr[fz][2];
                t.out = crop_stage_base<HS, VS, OUT>(stage, s);
                tile_to_stage<HS, VS, OUT>(p, t, lds);
                uint8_t* const img = (uint8_t*)p.fptr[fz][3];
                const CropTensorOut o = crop_tensor_out(tp, fz);
                if (s.b0 < s.b1)
                    for (int tid = 0; tid < C::NT; tid++) crop_copyout_tensor<HS, VS, OUT>(o, s, tid, C::NT, stage, img);
                if (s.c0 < s.c1) {
                    s.b0 = s.c0; s.b1 = s.c1;
                    for (int tid = 0; tid < C::NT; tid++) crop_copyout_tensor<HS, VS, OUT>(o, s, tid, C::NT, stage, img);
                }
            }
}

// zj_crop_zero_tensor_kernel over a grid of max_rows x max_frames x nrec
static void run_zero_tensor(const CropTensorZero* tab, int nrec, int max_rows, int max_frames)
{
    for (int bz = 0; bz < nrec; bz++)
        for (int fr = 0; fr < max_frames; fr++)
            for (int bx = 0; bx < max_rows; bx++) {
                const CropTensorZero& z = tab[bz];
                if (fr >= z.nframes) continue;
                for (int tid = 0; tid < 256; tid++) crop_tensor_zero(z, fr, z.rmin + bx, tid, 256);
            }
}

static int dispatch(int hs, int vs, int out, const CropTensorParams* tab, int nrec, int shift, int ncols, int nstrips, uint8_t poison)
{
#define ZJ_CASE(H, V, O) if (hs == H && vs == V && out == O) { run_crop_tensor<H, V, O>(tab, nrec, shift, ncols, nstrips, poison); return ZJ_OK; }
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR)
#undef ZJ_CASE
    return ZJ_ERR_UNSUPPORTED;
}

// the zero launch's grid over its records (zj_api.cpp: crop_tensor_submit)
static void zero_launch(const std::vector<CropTensorZero>& zeros)
{
    int rows = 0, frames = 0;
    for (const CropTensorZero& z : zeros) {
        if (z.h - z.rmin > rows) rows = z.h - z.rmin;
        if (z.nframes > frames) frames = z.nframes;
    }
    if (!zeros.empty()) run_zero_tensor(zeros.data(), (int)zeros.size(), rows, frames);
}

extern "C" size_t zject_out_len(const zj_frame_desc* d, unsigned w, unsigned h, int dtype)
{
    Plan pl;
    CropPlan cp;
    if (!crop_tensor_desc_ok(d) || make_crop_plan(d, w, h, 0, pl, cp) != ZJ_OK) return 0;
    return crop_tensor_len(resize_channels(d), w, h, dtype);
}

// zj_decode_crops_tensor_device's host side (crop_tensor_fill, launches of up to SCATTER_MAX frames) over the emulated
// kernels; stage_poison: what the staging holds before a tile writes it.  scale / bias: the kernel's factors, 3 each.
extern "C" int zject_decode_crops_tensor(const zj_frame_desc* d, size_t nframes, const int16_t* const* y, const int16_t* const* cb,
                                         const int16_t* const* cr, const unsigned* origins, unsigned w, unsigned h, int dtype,
                                         int nhwc, const float* scale, const float* bias, const uint8_t* flip, uint8_t* out,
                                         int stage_poison)
{
    Plan pl;
    CropPlan cp;
    if (!crop_tensor_desc_ok(d)) return ZJ_ERR_UNSUPPORTED;
    int rc = make_crop_plan(d, w, h, 0, pl, cp);
    if (rc) return rc;
    const size_t img = crop_tensor_len(resize_channels(d), w, h, dtype);
    if (!img || !origins || nframes == 0) return ZJ_ERR_ARG;
    for (size_t f = 0; f < nframes; f++) {
        int s0, s1, k0, k1;
        if ((rc = crop_window(d, pl, cp, origins[2 * f], origins[2 * f + 1], s0, s1, k0, k1))) return rc;
    }
    // one record per SCATTER_MAX frames, all of them one launch (zj_api.cpp: crop_tensor_launches)
    const size_t nrec = (nframes + SCATTER_MAX - 1) / SCATTER_MAX;
    std::vector<CropTensorParams> recs(nrec);
    std::vector<CropTensorZero> zeros;
    int gx = 0, gy = 0;
    for (size_t r = 0; r < nrec; r++) {
        const size_t f0 = r * SCATTER_MAX;
        const int n = (int)(nframes - f0 < (size_t)SCATTER_MAX ? nframes - f0 : (size_t)SCATTER_MAX);
        CropTensorZero z;
        if (crop_tensor_fill(d, pl, cp, y, cb, cr, out, img, origins, dtype, nhwc, scale, bias, flip, f0, n, recs[r], z)) zeros.push_back(z);
        if (recs[r].cp.ncols > gx) gx = recs[r].cp.ncols;
        if (recs[r].cp.nstrips > gy) gy = recs[r].cp.nstrips;
    }
    zero_launch(zeros);
    return dispatch(pl.hs, pl.vs, pl.out, recs.data(), (int)nrec, CROP_TENSOR_SHIFT, gx, gy, (uint8_t)stage_poison);
}

// zj_decode_crops_tensor_mixed_device's host side (zj_api.cpp: crops_tensor_mixed_impl) over the emulated kernels: every
// frame its own descriptor, one record per frame, the frames of one kernel in one run of the table
extern "C" int zject_decode_crops_tensor_mixed(const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                               const int16_t* const* cb, const int16_t* const* cr, const unsigned* origins, unsigned w,
                                               unsigned h, int dtype, int nhwc, const float* scale, const float* bias,
                                               const uint8_t* flip, uint8_t* out, int stage_poison)
{
    if (!descs || !origins || nframes == 0 || !mixed_descs_agree(descs, nframes)) return ZJ_ERR_ARG;
    std::vector<Plan> pls(nframes);
    std::vector<CropPlan> cps(nframes);
    size_t img = 0;
    for (size_t f = 0; f < nframes; f++) {
        if (!crop_tensor_desc_ok(&descs[f])) return ZJ_ERR_UNSUPPORTED;
        int rc = make_crop_plan(&descs[f], w, h, 0, pls[f], cps[f]);
        if (rc) return rc;
        if (!(img = crop_tensor_len(resize_channels(&descs[f]), w, h, dtype))) return ZJ_ERR_ARG;
        int s0, s1, k0, k1;
        if ((rc = crop_window(&descs[f], pls[f], cps[f], origins[2 * f], origins[2 * f + 1], s0, s1, k0, k1))) return rc;
    }
    std::vector<CropTensorParams> recs(nframes);
    std::vector<CropTensorZero> zeros;
    struct Run { int hs, vs, out, gx, gy; size_t first; int n; };
    std::vector<Run> runs;
    size_t at = 0;
    for (int mode = 0; mode < 4; mode++)
        for (int gray = 0; gray < 2; gray++) {
            const int hs = 1 + (mode & 1), vs = 1 + (mode >> 1);
            Run run{hs, vs, 0, 0, 0, at, 0};
            for (size_t f = 0; f < nframes; f++) {
                const Plan& pl = pls[f];
                if (pl.hs != hs || pl.vs != vs || (pl.out == OUT_GRAY) != (gray != 0)) continue;
                CropTensorZero z;
                if (crop_tensor_fill(&descs[f], pl, cps[f], y, cb, cr, out, img, origins, dtype, nhwc, scale, bias, flip, f, 1, recs[at], z))
                    zeros.push_back(z);
                run.out = pl.out;
                if (recs[at].cp.ncols > run.gx) run.gx = recs[at].cp.ncols;
                if (recs[at].cp.nstrips > run.gy) run.gy = recs[at].cp.nstrips;
                run.n++; at++;
            }
            if (run.n) runs.push_back(run);
        }
    zero_launch(zeros);
    for (const Run& r : runs) {
        const int rc = dispatch(r.hs, r.vs, r.out, recs.data() + r.first, r.n, 0, r.gx, r.gy, (uint8_t)stage_poison);
        if (rc) return rc;
    }
    return ZJ_OK;
}

// crop_copyout_tensor by itself over a staging the caller fills: the bytes of h window rows (rows: h x 3w, RGB, tile 0 of
// strip 0 of a 4:2:0 frame, window at the origin) cut at cuts[0] < cuts[1] < ... into spans of one workgroup each.  The cuts
// may fall inside a pixel, which no real plan's spans do: the copy-out's partial-pixel items are exercised here alone.
extern "C" int zject_copyout_spans(int w, int h, const int* cuts, int ncuts, int dtype, int nhwc, int flip, const float* scale,
                                   const float* bias, const uint8_t* rows, uint8_t* out)
{
    using C = Cfg<2, 2, OUT_RGB>;
    using S = CropStage<2, 2, OUT_RGB>;
    if (w < 1 || w > C::TWY || h < 1 || h > C::SH || !resize_elem_bytes(dtype)) return ZJ_ERR_ARG;
    std::vector<uint8_t> stage_mem(S::BYTES + 32, 0x5C);
    uint8_t* stage = (uint8_t*)(((uintptr_t)stage_mem.data() + 15) & ~(uintptr_t)15);
    for (int r = 0; r < h; r++) memcpy(stage + r * S::PITCH + S::MARGIN, rows + (size_t)r * 3 * w, (size_t)3 * w);
    CropTensorOut o;
    for (int k = 0; k < 3; k++) { o.scale[k] = scale[k]; o.bias[k] = bias[k]; }
    o.w = w; o.h = h; o.dtype = dtype; o.nhwc = nhwc != 0; o.flip = flip != 0;
    int lo = 0;
    for (int i = 0; i <= ncuts; i++) {
        const int hi = i < ncuts ? cuts[i] : 3 * w;
        if (hi < lo || hi > 3 * w) return ZJ_ERR_ARG;
        CropSpan s{};
        s.r0 = 0; s.r1 = h; s.b0 = lo; s.b1 = hi;
        if (lo < hi)
            for (int tid = 0; tid < C::NT; tid++) crop_copyout_tensor<2, 2, OUT_RGB>(o, s, tid, C::NT, stage, out);
        lo = hi;
    }
    return ZJ_OK;
}
