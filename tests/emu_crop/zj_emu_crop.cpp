// zj_emu_crop.cpp -- CPU EMULATION of the crop-window kernels (zj_kernels.hip: zj_fused_crop_kernel, zj_crop_zero_kernel)
// and of the crop plan (zj_plan.h: make_crop_plan, crop_window, fill_crop_params).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu: every workgroup of a crop launch runs its phases thread by thread with the
// barriers between them, the staging area being a host buffer.  Never linked into libzjhip.so.
#define ZJ_EMU 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_plan.h"

using namespace zj;

// one crop workgroup's tile decode into `stage` (the kernel up to its last barrier)
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
    if (NEED_Y16 && *lds_flag<C>(lds) != 0) { // Q1 value outside a byte: the tile again, wide
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

template <int HS, int VS, int OUT>
static void run_crop(const CropParams& cp, uint8_t stage_poison)
{
    using C = Cfg<HS, VS, OUT>;
    using S = CropStage<HS, VS, OUT>;
    std::vector<char> lds_mem(C::LDS_PACKED + 32), stage_mem(S::BYTES + 32);
    char* lds = (char*)(((uintptr_t)lds_mem.data() + 15) & ~(uintptr_t)15);
    uint8_t* stage = (uint8_t*)(((uintptr_t)stage_mem.data() + 15) & ~(uintptr_t)15);
    const Params& p = cp.p;
    for (int fz = 0; fz < p.nframes; fz++)
        for (int sy = 0; sy < cp.nstrips; sy++)
            for (int sx = 0; sx < cp.ncols; sx++) {
                CropSpan s;
                if (!crop_locate<HS, VS, OUT>(cp, fz, sy, sx, s)) continue;
                memset(stage, stage_poison, S::BYTES); // LDS holds whatever it held: what is copied must have been written
                TileId t;
                t.frame = s.frame; t.strip = s.strip; t.tile = s.tile;
                t.y = (const int16_t*)p.fptr[fz][0]; t.cb = (const int16_t*)p.fptr[fz][1]; t.cr = (const int16_t*)p.fptr[fz][2];
                t.out = crop_stage_base<HS, VS, OUT>(stage, s);
                tile_to_stage<HS, VS, OUT>(p, t, lds);
                uint8_t* const out = (uint8_t*)p.fptr[fz][3];
                if (s.b0 < s.b1)
                    for (int tid = 0; tid < C::NT; tid++) crop_copyout<HS, VS, OUT>(cp, s, tid, C::NT, stage, out);
                if (s.c0 < s.c1) {
                    s.b0 = s.c0; s.b1 = s.c1;
                    for (int tid = 0; tid < C::NT; tid++) crop_copyout<HS, VS, OUT>(cp, s, tid, C::NT, stage, out);
                }
            }
}

static void run_zero(const CropZero& z)
{
    for (int fr = 0; fr < z.nframes; fr++)
        for (int pl = 0; pl < z.nplanes; pl++)
            for (int r = 0; r < z.crop_h; r++) {
                if ((int)z.y0[fr] + r < z.rows_covered) continue;
                memset((uint8_t*)z.fptr[fr] + pl * z.crop_plane + (long long)r * z.out_pitch, 0, (size_t)z.nbytes);
            }
}

static int dispatch(const Plan& pl, const CropParams& cp, uint8_t poison)
{
#define ZJ_CASE(H, V, O) if (pl.hs == H && pl.vs == V && pl.out == O) { run_crop<H, V, O>(cp, poison); return ZJ_OK; }
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR)
    ZJ_CASE(1, 1, OUT_RGBA) ZJ_CASE(2, 1, OUT_RGBA) ZJ_CASE(1, 2, OUT_RGBA) ZJ_CASE(2, 2, OUT_RGBA)
    ZJ_CASE(1, 1, OUT_RGB_CHW) ZJ_CASE(2, 1, OUT_RGB_CHW) ZJ_CASE(1, 2, OUT_RGB_CHW) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
    return ZJ_ERR_UNSUPPORTED;
}

extern "C" size_t zjec_crop_out_len(const zj_frame_desc* d, unsigned w, unsigned h, unsigned out_pitch)
{
    Plan pl;
    CropPlan cp;
    return make_crop_plan(d, w, h, out_pitch, pl, cp) == ZJ_OK ? cp.out_len : 0;
}

// zj_decode_crops_device's host side (argument checks, launches of up to SCATTER_MAX frames) over the emulated kernels;
// stage_poison: what the staging holds before a tile writes it
extern "C" int zjec_decode_crops(const zj_frame_desc* d, size_t nframes, const int16_t* const* y, const int16_t* const* cb,
                                 const int16_t* const* cr, const unsigned* origins, unsigned w, unsigned h, uint8_t* const* out,
                                 unsigned out_pitch, int stage_poison)
{
    Plan pl;
    CropPlan cp;
    int rc = make_crop_plan(d, w, h, out_pitch, pl, cp);
    if (rc) return rc;
    if (!origins || nframes == 0) return ZJ_ERR_ARG;
    for (size_t f = 0; f < nframes; f++) {
        int s0, s1, k0, k1;
        if ((rc = crop_window(d, pl, cp, origins[2 * f], origins[2 * f + 1], s0, s1, k0, k1))) return rc;
    }
    const bool chroma = pl.out != OUT_GRAY;
    for (size_t f0 = 0; f0 < nframes; f0 += SCATTER_MAX) {
        const int n = (int)(nframes - f0 < (size_t)SCATTER_MAX ? nframes - f0 : (size_t)SCATTER_MAX);
        static CropParams p; // (1.9 KB: not on the stack)
        int nstrips, ncols;
        fill_crop_params(d, pl, cp, y, chroma ? cb : nullptr, chroma ? cr : nullptr, out, origins, f0, n, p, nstrips, ncols);
        CropZero z{};
        z.rows_covered = pl.rows_covered; z.crop_h = cp.h; z.nbytes = cp.w * cp.bpp; z.out_pitch = (int)cp.out_pitch;
        z.nplanes = cp.nplanes; z.crop_plane = (long long)cp.out_pitch * cp.h; z.nframes = n;
        for (int f = 0; f < n; f++) { z.fptr[f] = (uint64_t)(uintptr_t)out[f0 + f]; z.y0[f] = origins[2 * (f0 + f) + 1]; }
        run_zero(z);
        if ((rc = dispatch(pl, p, (uint8_t)stage_poison))) return rc;
    }
    return ZJ_OK;
}

// the plan for one window: strips [s0, s1), tile columns [k0, k1) and every column's first owned byte (own[0 .. tiles])
extern "C" int zjec_crop_window(const zj_frame_desc* d, unsigned x, unsigned y, unsigned w, unsigned h, int out4[4], int* own, int own_cap)
{
    Plan pl;
    CropPlan cp;
    int rc = make_crop_plan(d, w, h, 0, pl, cp);
    if (rc) return rc;
    if ((rc = crop_window(d, pl, cp, x, y, out4[0], out4[1], out4[2], out4[3]))) return rc;
    for (int k = 0; k <= pl.tiles_per_row && k < own_cap; k++) own[k] = crop_own(cp, k);
    return pl.tiles_per_row;
}

// Brute force for the plan tests: which tile column writes each byte of a frame row (strip 0, frame 0), found by decoding
// every column k >= k_lo of strip 0 into the staging twice, over two different poisons (a byte is written where both agree).
// owner[b] = column, -1 = nobody, -2 = more than one column, -3 = not examined: b left of column k_lo's natural range.  (A
// column writes nothing right of its own natural range, so the writers of every byte from there on are among the columns
// decoded, k_lo - 1 on.)
// Returns the number of columns.
template <int HS, int VS, int OUT>
static void owners_t(const Params& p, const Plan& pl, int k_lo, int* owner)
{
    using C = Cfg<HS, VS, OUT>;
    using S = CropStage<HS, VS, OUT>;
    std::vector<char> lds_mem(C::LDS_PACKED + 32);
    char* lds = (char*)(((uintptr_t)lds_mem.data() + 15) & ~(uintptr_t)15);
    std::vector<uint8_t> a(S::BYTES + 32), b(S::BYTES + 32);
    const int rb = (int)pl.row_bytes;
    for (int i = 0; i < rb; i++) owner[i] = i < k_lo * C::TWY * S::BPP ? -3 : -1;
    for (int k = k_lo > 0 ? k_lo - 1 : 0; k < pl.tiles_per_row; k++) {
        CropSpan s{};
        s.frame = 0; s.strip = 0; s.tile = k;
        uint8_t* st[2] = {(uint8_t*)(((uintptr_t)a.data() + 15) & ~(uintptr_t)15), (uint8_t*)(((uintptr_t)b.data() + 15) & ~(uintptr_t)15)};
        for (int v = 0; v < 2; v++) {
            memset(st[v], v ? 0xff : 0x00, S::BYTES);
            TileId t;
            t.frame = 0; t.strip = 0; t.tile = k;
            t.y = p.y; t.cb = p.cb; t.cr = p.cr;
            t.out = crop_stage_base<HS, VS, OUT>(st[v], s);
            tile_to_stage<HS, VS, OUT>(p, t, lds);
        }
        const int base = k * C::TWY * S::BPP - S::MARGIN;
        for (int i = 0; i < S::PITCH; i++) {
            const int bb = base + i;
            if (bb < 0 || bb >= rb || owner[bb] == -3 || st[0][i] != st[1][i]) continue; // (row 0 of the staging)
            owner[bb] = owner[bb] == -1 ? k : -2;
        }
    }
}

extern "C" int zjec_row_owners(const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr, int k_lo, int* owner)
{
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (pl.n_strips < 1) return ZJ_ERR_ARG;
    Params p;
    fill_params(d, pl, 1, y, cb, cr, nullptr, 1, p);
#define ZJ_CASE(H, V, O) if (pl.hs == H && pl.vs == V && pl.out == O) { using S = CropStage<H, V, O>; p.out_pitch = S::PITCH; p.plane_stride = (long long)S::PITCH * Cfg<H, V, O>::SH; owners_t<H, V, O>(p, pl, k_lo, owner); return pl.tiles_per_row; }
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR)
    ZJ_CASE(1, 1, OUT_RGBA) ZJ_CASE(2, 1, OUT_RGBA) ZJ_CASE(1, 2, OUT_RGBA) ZJ_CASE(2, 2, OUT_RGBA)
    ZJ_CASE(1, 1, OUT_RGB_CHW) ZJ_CASE(2, 1, OUT_RGB_CHW) ZJ_CASE(1, 2, OUT_RGB_CHW) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
    return ZJ_ERR_UNSUPPORTED;
}

// The plan's side of the write map: owner[b] = the tile column whose owned bytes (zj_plan.h: crop_spans) hold byte b
// of a frame row, -1 = no column, -2 = more than one.  Returns the number of columns.
extern "C" int zjec_plan_owners(const zj_frame_desc* d, int* owner)
{
    Plan pl;
    CropPlan cp;
    int rc = make_crop_plan(d, 1, 1, 0, pl, cp);
    if (rc) return rc;
    for (int b = 0; b < cp.row_bytes; b++) owner[b] = -1;
    for (int k = 0; k < pl.tiles_per_row; k++) {
        int a0, a1, c0, c1;
        crop_spans(cp, k, a0, a1, c0, c1);
        for (int b = a0; b < a1; b++) owner[b] = owner[b] == -1 ? k : -2;
        for (int b = c0; b < c1; b++) owner[b] = owner[b] == -1 ? k : -2;
    }
    return pl.tiles_per_row;
}
