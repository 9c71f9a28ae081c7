// zj_emu_crop_mixed.cpp -- CPU EMULATION of the mixed-geometry kernels (zj_crop_mixed.hip: zj_fused_crop_mixed_kernel,
// zj_crop_zero_mixed_kernel; zj_scaled_mixed.hip: zj_scaled_mixed_kernel) over the tables the library's host side builds
// (zj_mixed.h: mixed_frame_plan, mixed_frame_window, mixed_fill_tables).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_crop and tests/emu_scaled: every workgroup of a launch -- blockIdx.z picks the
// frame's record from the table, the grid is the launch's widest range -- runs its phases thread by thread with the barriers
// between them, LDS and the staging being host buffers filled with a poison first.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_mixed.h"
#include "../../zune-jpeg_amd/csrc/zj_rzgroup.h"

using namespace zj;

// one crop workgroup's tile decode into the staging (the kernel up to its last barrier; tests/emu_crop)
template <int HS, int VS, int OUT>
static void tile_to_stage(const Params& p, const TileId& t, char* lds)
{
    using C = Cfg<HS, VS, OUT>;
    constexpr bool NEED_Y16 = OUT == OUT_RGB || OUT == OUT_RGBA || OUT == OUT_RGB_CHW;
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

// zj_fused_crop_mixed_kernel over a grid of ncols x nstrips x n: the record of blockIdx.z, used with frame index 0
template <int HS, int VS, int OUT>
static void run_crop_mixed(const CropParams* tab, int n, int ncols, int nstrips, uint8_t stage_poison)
{
    using C = Cfg<HS, VS, OUT>;
    using S = CropStage<HS, VS, OUT>;
    std::vector<char> lds_mem(C::LDS_PACKED + 32), stage_mem(S::BYTES + 32);
    char* lds = (char*)(((uintptr_t)lds_mem.data() + 15) & ~(uintptr_t)15);
    uint8_t* stage = (uint8_t*)(((uintptr_t)stage_mem.data() + 15) & ~(uintptr_t)15);
    for (int bz = 0; bz < n; bz++)
        for (int sy = 0; sy < nstrips; sy++)
            for (int sx = 0; sx < ncols; sx++) {
                const CropParams& cp = tab[bz];
                const Params& p = cp.p;
                CropSpan s;
                if (!crop_locate<HS, VS, OUT>(cp, 0, sy, sx, s)) continue;
                memset(stage, stage_poison, S::BYTES);
                TileId t;
                t.frame = 0; t.strip = s.strip; t.tile = s.tile;
                t.y = (const int16_t*)p.fptr[0][0]; t.cb = (const int16_t*)p.fptr[0][1]; t.cr = (const int16_t*)p.fptr[0][2];
                t.out = crop_stage_base<HS, VS, OUT>(stage, s);
                tile_to_stage<HS, VS, OUT>(p, t, lds);
                uint8_t* const out = (uint8_t*)p.fptr[0][3];
                if (s.b0 < s.b1)
                    for (int tid = 0; tid < C::NT; tid++) crop_copyout<HS, VS, OUT>(cp, s, tid, C::NT, stage, out);
                if (s.c0 < s.c1) {
                    s.b0 = s.c0; s.b1 = s.c1;
                    for (int tid = 0; tid < C::NT; tid++) crop_copyout<HS, VS, OUT>(cp, s, tid, C::NT, stage, out);
                }
            }
}

// zj_crop_zero_mixed_kernel over a grid of max_h x max_planes x n
static void run_zero_mixed(const MixedZero* tab, int n, int max_h, int max_planes)
{
    for (int bz = 0; bz < n; bz++)
        for (int pl = 0; pl < max_planes; pl++)
            for (int r = 0; r < max_h; r++) {
                const MixedZero& z = tab[bz];
                if (pl >= z.nplanes || r >= z.h || z.y0 + r < z.rows_covered) continue;
                memset((uint8_t*)z.out + ((long long)pl * z.h + r) * z.nbytes, 0, (size_t)z.nbytes);
            }
}

// zj_scaled_mixed_kernel over a grid of ncols x nrows x n
template <int HS, int VS, int OUT, int SL>
static void run_scaled_mixed(const ScaledParams* tab, int n, int ncols, int nrows, uint8_t poison)
{
    using C = ScaledCfg<HS, VS, OUT, SL>;
    std::vector<char> mem(C::LDS + 32);
    char* lds = (char*)(((uintptr_t)mem.data() + 15) & ~(uintptr_t)15);
    for (int bz = 0; bz < n; bz++)
        for (int by = 0; by < nrows; by++)
            for (int bx = 0; bx < ncols; bx++) {
                const ScaledParams& p = tab[bz];
                ScaledTile t;
                if (!scaled_locate<C>(p, 0, by, bx, t)) continue;
                memset(lds, poison, C::LDS);
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

static int dispatch_crop(const MixedLaunch& l, const uint8_t* tab, uint8_t poison)
{
#define ZJ_CASE(H, V, O) if (l.hs == H && l.vs == V && l.out == O) { run_crop_mixed<H, V, O>((const CropParams*)(tab + l.off), l.n, l.gx, l.gy, poison); return ZJ_OK; }
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR) ZJ_CASE(1, 1, OUT_RGB_CHW)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR) ZJ_CASE(2, 1, OUT_RGB_CHW)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR) ZJ_CASE(1, 2, OUT_RGB_CHW)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
    return ZJ_ERR_UNSUPPORTED;
}

static int dispatch_scaled(const MixedLaunch& l, const uint8_t* tab, uint8_t poison)
{
#define ZJ_CASE1(H, V, O, L) if (l.hs == H && l.vs == V && l.out == O && l.sl == L) { run_scaled_mixed<H, V, O, L>((const ScaledParams*)(tab + l.off), l.n, l.gx, l.gy, poison); return ZJ_OK; }
#define ZJ_CASE(H, V, O) ZJ_CASE1(H, V, O, 1) ZJ_CASE1(H, V, O, 2) ZJ_CASE1(H, V, O, 3)
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR) ZJ_CASE(1, 1, OUT_RGB_CHW)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR) ZJ_CASE(2, 1, OUT_RGB_CHW)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR) ZJ_CASE(1, 2, OUT_RGB_CHW)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
#undef ZJ_CASE1
    return ZJ_ERR_UNSUPPORTED;
}

// the frame checks of zj_decode_crops_resized_mixed_device (zj_mixed.h: mixed_check_frames; no planes here to check)
static int plan_all(const zj_frame_desc* descs, size_t n, const unsigned* windows, unsigned out_w, unsigned out_h, int max_k,
                    const uint8_t* orientation, std::vector<MixedFrame>& fr)
{
    if (!descs || !windows || n == 0 || max_k < 0 || max_k > 3) return ZJ_ERR_ARG;
    fr.resize(n);
    const int out_rc = resized_len(resize_channels(&descs[0]), out_w, out_h, ZJ_DTYPE_U8) ? ZJ_OK : ZJ_ERR_ARG;
    return mixed_check_frames(descs, n, windows, orientation, out_rc, out_w, out_h, max_k, [](size_t, bool) { return (int)ZJ_OK; },
                              fr.data());
}

// The plan alone: status, and per frame info[6f ..] = scale k, the crop-stage window x, y, w, h, the orientation
extern "C" int zjem_plan(const zj_frame_desc* descs, size_t n, const unsigned* windows, unsigned out_w, unsigned out_h, int max_k,
                         const uint8_t* orientation, int* info)
{
    std::vector<MixedFrame> fr;
    const int rc = plan_all(descs, n, windows, out_w, out_h, max_k, orientation, fr);
    if (rc) return rc;
    for (size_t f = 0; f < n && info; f++) {
        info[6 * f] = fr[f].k;
        for (int i = 0; i < 4; i++) info[6 * f + 1 + i] = (int)fr[f].cwin[i];
        info[6 * f + 5] = fr[f].o;
    }
    return ZJ_OK;
}

// The crop stage of ONE group: the tables, then every launch the library makes, emulated.  out[f]: frame f's tight crop.
// counts[3] (optional): the crop, reduced and zero launches made.
extern "C" int zjem_crops(const zj_frame_desc* descs, size_t n, const int16_t* const* y, const int16_t* const* cb,
                          const int16_t* const* cr, const unsigned* windows, unsigned out_w, unsigned out_h, int max_k,
                          const uint8_t* orientation, uint8_t* const* out, int poison, int* counts)
{
    std::vector<MixedFrame> fr;
    int rc = plan_all(descs, n, windows, out_w, out_h, max_k, orientation, fr);
    if (rc) return rc;
    std::vector<uint8_t> mem(mixed_table_bytes(fr.data(), n) + MIXED_TAB_ALIGN);
    uint8_t* const tab = (uint8_t*)(((uintptr_t)mem.data() + MIXED_TAB_ALIGN - 1) & ~(uintptr_t)(MIXED_TAB_ALIGN - 1));
    MixedTables t;
    mixed_fill_tables(descs, fr.data(), n, y, cb, cr, out, tab, t);
    if (t.bytes > mixed_table_bytes(fr.data(), n)) return ZJ_ERR_HIP; // (the bound the library sizes its staging by)
    if (t.zero.n) run_zero_mixed((const MixedZero*)(tab + t.zero.off), t.zero.n, t.zero.gx, t.zero.gy);
    for (const MixedLaunch& l : t.crop)
        if ((rc = dispatch_crop(l, tab, (uint8_t)poison))) return rc;
    for (const MixedLaunch& l : t.scaled)
        if ((rc = dispatch_scaled(l, tab, (uint8_t)poison))) return rc;
    if (counts) { counts[0] = (int)t.crop.size(); counts[1] = (int)t.scaled.size(); counts[2] = t.zero.n ? 1 : 0; }
    return ZJ_OK;
}

// The library's group planner (zj_rzgroup.h) over n frames of wh[2f], wh[2f + 1] and orientation o[f] at `cap` (0: the
// library's RZ_GROUP_CAP).  Returns the scratch bytes of the call; group[f]: the index of frame f's group; place[8f ..]: the
// crop's offset, w, h, pitch, then the same of the image the resize reads; gbytes[g]: group g's bytes (n entries).
extern "C" size_t zjem_rz_groups(const unsigned* wh, const uint8_t* o, size_t n, int channels, int chw, size_t cap, int* group,
                                 unsigned long long* place, unsigned long long* gbytes)
{
    if (!cap) cap = RZ_GROUP_CAP;
    std::vector<RzFrame> fr(n);
    for (size_t f = 0; f < n; f++) fr[f] = RzFrame{wh[2 * f], wh[2 * f + 1], o[f]};
    std::vector<RzPlace> pl(n);
    size_t g = 0;
    for (size_t g0 = 0, g1; g0 < n; g0 = g1, g++) {
        size_t bytes = 0;
        g1 = rz_group_next(fr.data(), n, g0, channels, chw != 0, cap, pl.data(), &bytes);
        gbytes[g] = bytes;
        for (size_t f = g0; f < g1; f++) {
            group[f] = (int)g;
            const RzImage im[2] = {pl[f].crop, pl[f].in};
            for (int k = 0; k < 2; k++) {
                place[8 * f + 4 * k] = im[k].off; place[8 * f + 4 * k + 1] = im[k].w;
                place[8 * f + 4 * k + 2] = im[k].h; place[8 * f + 4 * k + 3] = im[k].pitch;
            }
        }
    }
    return rz_scratch_need(fr.data(), n, channels, chw != 0, cap);
}

extern "C" size_t zjem_record_bytes(int which) { return which == 0 ? sizeof(CropParams) : which == 1 ? sizeof(ScaledParams) : sizeof(MixedZero); }
