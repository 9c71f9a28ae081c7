// zj_plan.h -- host-side geometry/launch planning shared by the product library (zj_api.cpp) and the
// CPU emulation harness used by the CPU test-suite (tests/emu).  No device code here.  The pure size and window rules are
// zj_geom.h's.
//
// Geometry follows src/headers.rs:306-339 (mcu_x, mcu_y, width_stride) and the strip loop of
// src/mcu_prog.rs:132-246 / src/mcu.rs:139-230 (paths relative to the reference tree).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/zjhip.h"
#include "zj_device.h"
#include "zj_geom.h"
#include "zj_scaled.h"

namespace zj {

struct Plan {
    int hs, vs;          // luma sampling factors
    int out;             // OUT_RGB / OUT_GRAY / OUT_YCBCR / OUT_RGBA / OUT_RGB_CHW
    int plain;           // OUT_RGB with ZJ_FLAG_PLAIN_TAIL
    int clamp_dc;        // ZJ_FLAG_CLAMP_DC
    int edge_rep;        // ZJ_FLAG_EDGE_REPLICATE (meaningful when hs == 2)
    int mcu_x, mcu_y;
    int n_strips;        // strips the reference's zip() would process
    int strip_rows;      // luma rows per strip
    int tiles_per_row;
    int nt;              // threads per workgroup
    size_t y_len, c_len; // i16 elements per plane
    size_t out_len;      // bytes per frame (out_pitch x height, CHW: x 3)
    size_t row_bytes;    // bytes of one output row (CHW: of a plane's row): width x components
    size_t out_pitch;    // bytes between rows: zj_frame_desc.out_pitch, or row_bytes when that is 0
    int ncomp_out;
    bool fast;           // aligned fast path (W % 16 == 0, W >= 32)
    int regular_px;      // !fast: pixels of a row made of ordinary 16-pixel groups; 0: the generic kernels (see make_plan)
    int rows_covered;    // n_strips * strip_rows; rows below stay 0 in the reference (Q6)
};

template <int HS, int VS>
inline void plan_geo(Plan& pl, bool chroma)
{
    if (chroma) {
        using C = Cfg<HS, VS, OUT_RGB>;
        pl.strip_rows = C::SH; pl.tiles_per_row = (pl.mcu_x + C::TWC - 1) / C::TWC; pl.nt = C::NT;
    } else {
        using C = Cfg<HS, VS, OUT_GRAY>;
        pl.strip_rows = C::SH; pl.tiles_per_row = (pl.mcu_x + C::TWC - 1) / C::TWC; pl.nt = C::NT;
    }
}

// Returns ZJ_OK or an error status.
inline int make_plan(const zj_frame_desc* d, Plan& pl)
{
    if (!d || d->width == 0 || d->height == 0) return ZJ_ERR_ARG;
    if (!((d->h_max == 1 || d->h_max == 2) && (d->v_max == 1 || d->v_max == 2))) return ZJ_ERR_ARG;
    if (d->in_components != 1 && d->in_components != 3) return ZJ_ERR_ARG;
    if (d->width > 65535 || d->height > 65535) return ZJ_ERR_ARG; // u16 in the reference (decoder.rs:652)
    const int nout = ncomp_of(d->out_colorspace);
    if (nout == 0) return ZJ_ERR_ARG;
    // grayscale JPEG with a down-sampled component (mcu.rs:170-196) is reset to (1,1) by the
    // reference with a warning; callers must pass (1,1) here.
    if (d->in_components == 1 && (d->h_max != 1 || d->v_max != 1)) return ZJ_ERR_UNSUPPORTED;
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 64; k++)
            if (d->qt[c][k] < 0 || d->qt[c][k] > 255) return ZJ_ERR_UNSUPPORTED; // 8-bit DQT only
    pl.hs = (int)d->h_max;
    pl.vs = (int)d->v_max;
    if (d->out_colorspace == ZJ_CS_GRAYSCALE) pl.out = OUT_GRAY;
    else if (d->out_colorspace == ZJ_CS_RGB && d->in_components == 3) pl.out = OUT_RGB;
    else if (d->out_colorspace == ZJ_CS_YCBCR && d->in_components == 3) pl.out = OUT_YCBCR;
    // RGBA/RGBX are malformed in the reference itself; here they are an extension: R G B 255
    else if ((d->out_colorspace == ZJ_CS_RGBA || d->out_colorspace == ZJ_CS_RGBX) && d->in_components == 3) pl.out = OUT_RGBA;
    else return ZJ_ERR_UNSUPPORTED; // CMYK/YCCK are no-ops in the reference
    if (d->flags & ~(uint32_t)ZJ_FLAG_CORRECTED) return ZJ_ERR_ARG;
    pl.clamp_dc = (d->flags & ZJ_FLAG_CLAMP_DC) ? 1 : 0;
    pl.edge_rep = ((d->flags & ZJ_FLAG_EDGE_REPLICATE) && pl.hs == 2) ? 1 : 0;
    pl.plain = (pl.out == OUT_RGB && (d->flags & ZJ_FLAG_PLAIN_TAIL)) ? 1 : 0;
    if (d->out_layout == ZJ_LAYOUT_CHW) {
        if (pl.out == OUT_RGB) pl.out = OUT_RGB_CHW;            // planar u8 tensor layout, every pixel at its own place
        else if (pl.out != OUT_GRAY) return ZJ_ERR_UNSUPPORTED; // (one plane: CHW == HWC)
        pl.plain = 0;
    } else if (d->out_layout != ZJ_LAYOUT_HWC) return ZJ_ERR_ARG;
    pl.ncomp_out = nout;
    pl.mcu_x = (int)((d->width + 8 * d->h_max - 1) / (8 * d->h_max));  // headers.rs:317
    pl.mcu_y = (int)((d->height + 8 * d->v_max - 1) / (8 * d->v_max)); // headers.rs:319
    pl.y_len = (size_t)pl.mcu_x * 64 * d->v_max * d->h_max * pl.mcu_y; // mcu_prog.rs:76
    pl.c_len = d->in_components == 3 ? (size_t)pl.mcu_x * 64 * pl.mcu_y : 0;
    // rows may be laid out wider than they are (a pitch that is a multiple of 128 bytes keeps every tile's row segment on
    // whole cache lines: DESIGN.md 4.0 "row pitch"); the reference's own layout is the tight one
    pl.row_bytes = pl.out == OUT_RGB_CHW ? (size_t)d->width : (size_t)d->width * nout;
    pl.out_pitch = d->out_pitch ? (size_t)d->out_pitch : pl.row_bytes;
    if (pl.out_pitch < pl.row_bytes || pl.out_pitch > OUT_PITCH_MAX) return ZJ_ERR_ARG;
    pl.out_len = pl.out_pitch * d->height * (pl.out == OUT_RGB_CHW ? 3 : 1);
    const bool chroma = pl.out != OUT_GRAY;
    if (pl.hs == 1 && pl.vs == 1) plan_geo<1, 1>(pl, chroma);
    else if (pl.hs == 2 && pl.vs == 1) plan_geo<2, 1>(pl, chroma);
    else if (pl.hs == 1 && pl.vs == 2) plan_geo<1, 2>(pl, chroma);
    else plan_geo<2, 2>(pl, chroma);
    // strips: (2,1) and (2,2) take two MCU rows per strip, an odd last MCU row is dropped by
    // chunks_exact (mcu_prog.rs:191-205; mcu.rs:145-156 `mcu_y / 2`)
    const int mcu_rows_per_strip = (pl.hs == 2) ? 2 : 1;
    pl.n_strips = pl.mcu_y / mcu_rows_per_strip;
    // the zip with out_chunks (mcu_prog.rs:188-189) can only cut it shorter on absurd aspect ratios
    const size_t interleaved = (pl.hs != 1 || pl.vs != 1) ? 1 : 0;
    const size_t total = ((size_t)d->width + 8) * ((size_t)d->height + 8) * nout + interleaved * 128 * d->height * nout;
    const size_t chunk = (size_t)d->width * nout * 8 * d->h_max * d->v_max;
    if (total / chunk < (size_t)pl.n_strips) pl.n_strips = (int)(total / chunk);
    pl.fast = (d->width % 16 == 0) && d->width >= 32;
    if (pl.fast && (pl.out_pitch & 15)) return ZJ_ERR_ARG; // the aligned kernels store 16 bytes per lane at 16-byte-aligned addresses
    // A ragged width (the reference's own medium images are 2500 pixels wide, tests/medium_images.rs) is irregular only
    // at the END of its rows: the last two 8-pixel units are written early (Q5), what lies between them and the padded
    // width is never converted, the row is clipped at 3W (worker.rs:143-251).  The tail region starts at most 61 bytes
    // below 48 * elements (elements = P/16 - 1, worker.rs:171), so every 16-pixel group G <= elements - 3 is an ordinary
    // one: 48 bytes at 48 * G, all inside the row.  Those groups take the aligned fast path (the staged, lane-contiguous
    // stores; a row may start at any byte, global stores take any alignment); the few groups beyond them take the generic
    // stores, by the lanes that hold them, in the same launch (the RAG instantiations, zj_device.h: phase_color).
    pl.regular_px = 0;
    if (!pl.fast && d->width >= 64) {
        const int P = pl.mcu_x * 8 * pl.hs, elements = P / 16 - 1;
        if (elements > 2) pl.regular_px = 16 * (elements - 2); // groups 0 .. elements - 3
    }
    if (pl.out == OUT_GRAY && pl.n_strips > 0) {
        // ycbcr_to_grayscale re-derives the row count as len/width (color_convert/scalar.rs:97-99);
        // when padding makes that exceed the real row count it walks off its output chunk and panics.
        const size_t P = (size_t)pl.mcu_x * 8 * d->h_max, rows = (size_t)pl.strip_rows;
        if (rows * P / d->width != rows) return ZJ_ERR_PANIC;
    }
    pl.rows_covered = pl.n_strips * pl.strip_rows;
    return ZJ_OK;
}

// i16 elements of one strip of the plan's luma plane (yrow) and of each chroma plane (crow): a plane is its strips one after
// the other, so strips [s0, s1) are the elements [s0 * row, s1 * row)
inline void plan_strip_elems(const Plan& pl, size_t& yrow, size_t& crow)
{
    yrow = (size_t)pl.mcu_x * pl.hs * 64 * (pl.strip_rows / 8);
    crow = (size_t)pl.mcu_x * 64 * (pl.strip_rows / (8 * pl.vs));
}

// Byte ranges of one frame's output that the strips never reach (rows below the last complete strip,
// Q6: the reference leaves them 0).  HWC: one range; CHW: one per plane.  Returns the number of ranges.
inline int uncovered_ranges(const zj_frame_desc* d, const Plan& pl, size_t off[3], size_t len[3])
{
    // (whole rows of out_pitch bytes: with a padded pitch the padding of THESE rows is zeroed along with them)
    const size_t H = d->height, Pb = pl.out_pitch;
    const size_t covered = (size_t)pl.rows_covered < H ? (size_t)pl.rows_covered : H;
    if (covered >= H) return 0;
    if (pl.out == OUT_RGB_CHW) {
        for (int c = 0; c < 3; c++) { off[c] = (size_t)c * Pb * H + covered * Pb; len[c] = (H - covered) * Pb; }
        return 3;
    }
    off[0] = covered * Pb;
    len[0] = pl.out_len - off[0];
    return 1;
}

// the launch grid: nframes x n_strips x tiles_per_row workgroups, and the multipliers tile_from_id divides with
inline void set_grid(Params& p, int nframes, int n_strips, int tiles_per_row)
{
    p.nframes = nframes; p.n_strips = n_strips; p.tiles_per_row = tiles_per_row;
    p.total_tiles = nframes * n_strips * tiles_per_row;
    const Magic gt = magic_u31((uint32_t)(tiles_per_row > 0 ? tiles_per_row : 1)), gs = magic_u31((uint32_t)(n_strips > 0 ? n_strips : 1));
    p.tpr_magic = gt.m; p.tpr_shift = gt.s; p.ns_magic = gs.m; p.ns_shift = gs.s;
    p.stagger_wgs = p.stagger_delay = 0; p.stagger_magic = p.stagger_shift = 0;
}

inline void fill_params(const zj_frame_desc* d, const Plan& pl, size_t nframes, const int16_t* y,
                        const int16_t* cb, const int16_t* cr, uint8_t* out, int zero_fill, Params& p)
{
    p.y = y; p.cb = cb; p.cr = cr; p.out = out;
    // the tables travel in the kernel arguments (no device copy to order against other streams); the reference
    // snapshots them per component at SOF time (headers.rs:327), d->qt is that snapshot
    for (int c = 0; c < 3; c++) build_table(d->qt[c], p.tab + TAB_DW * c);
    p.y_frame_stride = (long long)pl.y_len;
    p.c_frame_stride = (long long)pl.c_len;
    p.out_frame_stride = (long long)pl.out_len;
    p.width = (int)d->width; p.height = (int)d->height;
    p.mcu_x = pl.mcu_x; p.zero_fill = zero_fill;
    set_grid(p, (int)nframes, pl.n_strips, pl.tiles_per_row);
#if defined(ZJ_ABLATION)
    p.debug = 0;
#endif
    p.plain = pl.plain;
    p.clamp_dc = pl.clamp_dc;
    p.edge_rep = pl.edge_rep;
    p.out_pitch = (int)pl.out_pitch;
    p.plane_stride = (long long)pl.out_pitch * d->height;
    p.regular_px = pl.regular_px;
}

// which family of fused kernels a plan launches: 0 generic stores (any width), 1 aligned fast path, 2 ragged fast path
// (RAG).  The wide generation (variant 1) has no RAG form: its ragged frames take the generic kernels.
inline int launch_mode(const Plan& pl, int variant) { return pl.fast ? 1 : ((pl.regular_px > 0 && variant != 1) ? 2 : 0); }

// frames [f0, f0 + n) of a scattered batch: their addresses into a launch's table, y | cb | cr | out (n <= SCATTER_MAX)
inline void set_frame_ptrs(uint64_t (&fptr)[SCATTER_MAX][4], const int16_t* const* y, const int16_t* const* cb,
                           const int16_t* const* cr, uint8_t* const* out, size_t f0, int n)
{
    for (int f = 0; f < SCATTER_MAX; f++) {
        const bool in = f < n;
        fptr[f][0] = in ? (uint64_t)(uintptr_t)y[f0 + f] : 0;
        fptr[f][1] = in && cb ? (uint64_t)(uintptr_t)cb[f0 + f] : 0;
        fptr[f][2] = in && cr ? (uint64_t)(uintptr_t)cr[f0 + f] : 0;
        fptr[f][3] = in ? (uint64_t)(uintptr_t)out[f0 + f] : 0;
    }
}
inline void set_scatter(Params& p, const int16_t* const* y, const int16_t* const* cb, const int16_t* const* cr,
                        uint8_t* const* out, size_t f0, int n)
{
    p.y = nullptr; p.cb = nullptr; p.cr = nullptr; p.out = nullptr; // y == nullptr marks the launch as scattered (decode_tile)
    set_frame_ptrs(p.fptr, y, cb, cr, out, f0, n);
}

// ---- crop windows (zj_decode_crops_device; zj_device.h: CropParams) -------------------------------------------------
struct CropPlan {
    int w, h;             // window, pixels
    int bpp;              // bytes per pixel of a frame row (CHW: 1, per plane)
    int nplanes;          // 3 for CHW, else 1
    int twy, sh;          // tile width (pixels) and strip height of the crop kernel (the generic fused kernel's tiles)
    int row_bytes;        // bytes of a frame row (CHW: of one plane's row)
    int tile_bytes;       // bpp x twy: a tile column's natural byte range in a row
    int cut_tile[2], cut_lo[2]; // ownership exceptions: the tiles holding the row's two early-written RGB units (Q5)
    int hole_tile, hole_lo, hole_hi; // ... and the bytes [hole_lo, hole_hi) that tile writes inside a later tile's range
    size_t out_pitch;     // bytes between crop rows (CHW: of a plane)
    size_t out_len;       // bytes of one crop (x 3 planes for CHW)
};

// first byte of a frame row that tile column k owns (zj_device.h: crop_own_lo)
inline int crop_own(const CropPlan& cp, int k) { return crop_own_lo(k, cp.tile_bytes, cp.row_bytes, cp.cut_tile[0], cp.cut_lo[0], cp.cut_tile[1], cp.cut_lo[1]); }

template <int HS, int VS>
inline void crop_geo(CropPlan& cp, bool chroma)
{
    if (chroma) { using C = Cfg<HS, VS, OUT_RGB>; cp.twy = C::TWY; cp.sh = C::SH; }
    else { using C = Cfg<HS, VS, OUT_GRAY>; cp.twy = C::TWY; cp.sh = C::SH; }
}

// The crop's geometry for a window of w x h pixels whose rows lie out_pitch bytes apart (0: tight).  The frame's own
// out_pitch must be 0: a crop's layout is its own.
inline int make_crop_plan(const zj_frame_desc* d, unsigned w, unsigned h, unsigned out_pitch, Plan& pl, CropPlan& cp)
{
    int rc = make_plan(d, pl);
    if (rc) return rc;
    const WindowLayout g = window_layout(d, w, h, out_pitch);
    if (d->out_pitch != 0 || !window_inside(g, 0, 0, w, h, d->width, d->height) || !window_pitch_ok(g)) return ZJ_ERR_ARG;
    cp.w = (int)w; cp.h = (int)h;
    cp.nplanes = g.nplanes; cp.bpp = g.bpp;
    cp.out_pitch = g.pitch; cp.out_len = g.len;
    if (pl.hs == 1 && pl.vs == 1) crop_geo<1, 1>(cp, pl.out != OUT_GRAY);
    else if (pl.hs == 2 && pl.vs == 1) crop_geo<2, 1>(cp, pl.out != OUT_GRAY);
    else if (pl.hs == 1 && pl.vs == 2) crop_geo<1, 2>(cp, pl.out != OUT_GRAY);
    else crop_geo<2, 2>(cp, pl.out != OUT_GRAY);
    cp.row_bytes = (int)pl.row_bytes;
    cp.tile_bytes = cp.bpp * cp.twy;
    // Who writes the end of a row (store_unit_generic, the rules of the crop kernel's stores): the last two 8-pixel units
    // of an RGB row under the early-tail quirk (Q5) are written at p' and p' + 24, up to 88 bytes left of their own tile,
    // and the zeros after them (Q6) by the last unit's tile.  Every other byte belongs to the tile its pixel lies in.
    // Where the row ends 1 to 15 bytes past `position` (diff > 48), the two units end before `position`: the bytes
    // [p' + 48, position) are the ordinary unit's below `position`.  When that unit's tile ends at or before p' (the tail
    // starts on a tile boundary: 4:2:2 / 4:2:0 widths W = 1..5 mod 256, W > 256), they are a hole in the tail tile's
    // range [p', ...) that the previous tile owns.
    cp.cut_tile[0] = cp.cut_tile[1] = -1;
    cp.cut_lo[0] = cp.cut_lo[1] = 0;
    cp.hole_tile = -1; cp.hole_lo = cp.hole_hi = cp.row_bytes;
    const int W = (int)d->width;
    if (pl.out == OUT_RGB && !pl.plain && W >= 16) {
        const long long P = (long long)pl.mcu_x * 8 * pl.hs, units = P >> 3;
        long long elems = P / 16 - 1; if (elems < 0) elems = 0;
        const long long position = 48 * elems;
        long long diff = 64 - (3ll * W - position); if (diff < 0) diff = 0;
        const long long pp = position > diff ? position - diff : 0;
        cp.cut_tile[0] = (int)(8 * (units - 2) / cp.twy); cp.cut_lo[0] = (int)pp;
        cp.cut_tile[1] = (int)(8 * (units - 1) / cp.twy); cp.cut_lo[1] = (int)(pp + 24);
        const int k = (int)((pp + 48) / cp.tile_bytes); // the tile of the ordinary unit under [p' + 48, position)
        if (pp + 48 < position && crop_own(cp, k + 1) <= pp + 48) {
            cp.hole_tile = k; cp.hole_lo = (int)(pp + 48); cp.hole_hi = (int)position;
        }
    }
    return ZJ_OK;
}

// The window of an ALL-ZERO output (zj_geom.h: zero_output).  No tile is decoded: the crop is zeros, laid out as every
// window is (window_layout).
inline int make_zero_crop(const zj_frame_desc* d, unsigned w, unsigned h, unsigned out_pitch, CropPlan& cp)
{
    const int nc = d ? ncomp_of(d->out_colorspace) : 0;
    if (!nc || d->width == 0 || d->height == 0 || d->width > 65535 || d->height > 65535) return ZJ_ERR_ARG;
    const WindowLayout g = window_layout(d, w, h, out_pitch);
    if (d->out_pitch != 0 || !window_inside(g, 0, 0, w, h, d->width, d->height) || !window_pitch_ok(g)) return ZJ_ERR_ARG;
    cp = CropPlan{};
    cp.w = (int)w; cp.h = (int)h;
    cp.bpp = g.bpp; cp.nplanes = g.nplanes;
    cp.out_pitch = g.pitch; cp.out_len = g.len;
    cp.row_bytes = (int)d->width * cp.bpp;
    cp.cut_tile[0] = cp.cut_tile[1] = -1;
    cp.hole_tile = -1; cp.hole_lo = cp.hole_hi = cp.row_bytes;
    return ZJ_OK;
}

// the bytes of a frame row tile column k owns: [a0, a1) and [c0, c1) (zj_device.h: crop_own_spans)
inline void crop_spans(const CropPlan& cp, int k, int& a0, int& a1, int& c0, int& c1)
{
    crop_own_spans(k, crop_own(cp, k), crop_own(cp, k + 1), cp.hole_tile, cp.hole_lo, cp.hole_hi, a0, a1, c0, c1);
}

// A window at (x, y) of a frame of plan pl: is it inside the frame, and which strips [s0, s1) and tile columns [k0, k1)
// does it need (strips clipped to the ones that exist: the window's rows at or below rows_covered are zeros, Q6)
inline int crop_window(const zj_frame_desc* d, const Plan& pl, const CropPlan& cp, unsigned x, unsigned y, int& s0, int& s1, int& k0, int& k1)
{
    if ((size_t)x + cp.w > d->width || (size_t)y + cp.h > d->height) return ZJ_ERR_ARG;
    s0 = (int)(y / cp.sh);
    s1 = (int)((y + cp.h + cp.sh - 1) / cp.sh);
    if (s1 > pl.n_strips) s1 = pl.n_strips;
    if (s0 > s1) s0 = s1;
    // the columns that own a byte of the window.  They are consecutive: a row's owners rise byte by byte except in the
    // hole, whose owner is the column just before the tail's.
    const int wb0 = (int)x * cp.bpp, wb1 = ((int)x + cp.w) * cp.bpp;
    k0 = k1 = 0;
    for (int k = 0; k < pl.tiles_per_row; k++) {
        int a0, a1, c0, c1;
        crop_spans(cp, k, a0, a1, c0, c1);
        const bool in_a = (a0 > wb0 ? a0 : wb0) < (a1 < wb1 ? a1 : wb1), in_c = (c0 > wb0 ? c0 : wb0) < (c1 < wb1 ? c1 : wb1);
        if (!in_a && !in_c) continue;
        if (k1 == 0) k0 = k;
        k1 = k + 1;
    }
    return ZJ_OK;
}

// the launch's arguments for frames [f0, f0 + n) of a crop batch; strips / columns: the grid (the largest ranges).
// win: per frame x, y (stride 2: every window cp.w x cp.h, the crop's pitch cp.out_pitch) or x, y, w, h (stride 4: each
// crop tight at its own size, CropParams.out_pitch 0)
inline void fill_crop_params_win(const zj_frame_desc* d, const Plan& pl, const CropPlan& cp, const int16_t* const* y,
                                 const int16_t* const* cb, const int16_t* const* cr, uint8_t* const* out, const unsigned* win,
                                 const int stride, size_t f0, int n, CropParams& c, int& nstrips, int& ncols)
{
    fill_params(d, pl, (size_t)n, nullptr, nullptr, nullptr, nullptr, 1, c.p);
    set_scatter(c.p, y, cb, cr, out, f0, n);
    // the tile decode writes the staging (zj_device.h: CropStage), rows at the staging's pitch
    const int pitch = crop_stage_pitch(pl.out, cp.twy);
    c.p.out_pitch = pitch;
    c.p.plane_stride = (long long)pitch * cp.sh;
    c.p.out_frame_stride = 0;
    c.crop_w = cp.w; c.crop_h = cp.h;
    c.out_pitch = stride == 4 ? 0 : (int)cp.out_pitch;
    c.bpp = cp.bpp; c.row_bytes = cp.row_bytes; c.tile_bytes = cp.tile_bytes;
    for (int i = 0; i < 2; i++) { c.cut_tile[i] = cp.cut_tile[i]; c.cut_lo[i] = cp.cut_lo[i]; }
    c.hole_tile = cp.hole_tile; c.hole_lo = cp.hole_lo; c.hole_hi = cp.hole_hi;
    c.crop_plane = (long long)cp.out_pitch * cp.h;
    nstrips = ncols = 0;
    for (int f = 0; f < SCATTER_MAX; f++) {
        c.origin[f] = c.first[f] = c.size[f] = 0;
        if (f >= n) continue;
        const unsigned* const wf = win + (size_t)stride * (f0 + f);
        const unsigned x = wf[0], yy = wf[1];
        CropPlan cw = cp;
        if (stride == 4) { cw.w = (int)wf[2]; cw.h = (int)wf[3]; }
        int s0 = 0, s1 = 0, k0 = 0, k1 = 0;
        crop_window(d, pl, cw, x, yy, s0, s1, k0, k1); // (checked by the caller)
        c.origin[f] = x | (yy << 16);
        c.first[f] = (uint32_t)k0 | ((uint32_t)s0 << 16);
        c.size[f] = (uint32_t)cw.w | ((uint32_t)cw.h << 16);
        if (s1 - s0 > nstrips) nstrips = s1 - s0;
        if (k1 - k0 > ncols) ncols = k1 - k0;
    }
    c.nstrips = nstrips; c.ncols = ncols;
}

// ... every window cp.w x cp.h at origins[2f], origins[2f + 1] (zj_decode_crops_device)
inline void fill_crop_params(const zj_frame_desc* d, const Plan& pl, const CropPlan& cp, const int16_t* const* y,
                             const int16_t* const* cb, const int16_t* const* cr, uint8_t* const* out, const unsigned* origins,
                             size_t f0, int n, CropParams& c, int& nstrips, int& ncols)
{
    fill_crop_params_win(d, pl, cp, y, cb, cr, out, origins, 2, f0, n, c, nstrips, ncols);
}

// ---- reduced-size decode (zj_decode_crops_scaled_device; zj_scaled.h: ScaledParams) -------------------
struct ScaledPlan {
    int sl;               // scale_log2: 1, 2, 3
    int rw, rh;           // the reduced frame: ceil(W / s) x ceil(H / s)
    int bpp, nplanes;     // bytes per pixel of a row (CHW: 1, per plane); 3 planes for CHW
    int mw, mh, tm;       // reduced pixels per MCU, MCUs per tile (zj_scaled.h: ScaledCfg)
    bool zero;            // a single-component frame with a colour output: zeros (zero_output)
};

// The reduced frame of d.  RGBA / RGBX: ZJ_ERR_UNSUPPORTED; the frame's own out_pitch must be 0.  (The reduced decode has
// no strips: the grayscale widths the reference panics on, make_plan's ZJ_ERR_PANIC, decode like every other.)
inline int make_scaled_plan(const zj_frame_desc* d, int scale_log2, Plan& pl, ScaledPlan& sp)
{
    if (!d || scale_log2 < 1 || scale_log2 > 3) return ZJ_ERR_ARG;
    if (d->out_colorspace == ZJ_CS_RGBA || d->out_colorspace == ZJ_CS_RGBX) return ZJ_ERR_UNSUPPORTED;
    sp = ScaledPlan{};
    sp.sl = scale_log2;
    sp.zero = zero_output(d);
    if (sp.zero) {
        CropPlan cp;
        const int rc = make_zero_crop(d, 1, 1, 0, cp);
        if (rc) return rc;
        sp.bpp = cp.bpp; sp.nplanes = cp.nplanes;
        pl = Plan{};
        pl.hs = pl.vs = 1;
    } else {
        const int rc = make_plan(d, pl);
        if (rc && rc != ZJ_ERR_PANIC) return rc;
        if (d->out_pitch != 0) return ZJ_ERR_ARG;
        sp.nplanes = pl.out == OUT_RGB_CHW ? 3 : 1;
        sp.bpp = pl.out == OUT_RGB_CHW ? 1 : pl.ncomp_out;
    }
    sp.rw = (int)reduced_dim(d->width, scale_log2); sp.rh = (int)reduced_dim(d->height, scale_log2);
    const int ln = 8 >> scale_log2, ypm = pl.hs * pl.vs;
    sp.mw = ln * pl.hs; sp.mh = ln * pl.vs;
    sp.tm = pl.out != OUT_GRAY ? (ypm == 4 ? 32 : 64) : 256 / ypm;
    return ZJ_OK;
}

// a window of the reduced frame whose rows lie out_pitch bytes apart (0: tight): its bytes, 0 = not a valid window
inline size_t scaled_window_len(const ScaledPlan& sp, unsigned x, unsigned y, unsigned w, unsigned h, unsigned out_pitch)
{
    const WindowLayout g = window_layout(sp.bpp, sp.nplanes, w, h, out_pitch);
    return window_inside(g, x, y, w, h, (unsigned)sp.rw, (unsigned)sp.rh) && window_pitch_ok(g) ? g.len : 0;
}

// the launch's arguments for frames [f0, f0 + n): win = x, y, w, h per frame in reduced pixels (checked by the caller),
// nullptr = the whole reduced frame
inline void fill_scaled_params(const zj_frame_desc* d, const Plan& pl, const ScaledPlan& sp, const int16_t* const* y,
                               const int16_t* const* cb, const int16_t* const* cr, uint8_t* const* out, const unsigned* win,
                               unsigned out_pitch, size_t f0, int n, ScaledParams& p)
{
    p.mcu_x = pl.mcu_x; p.rw = sp.rw; p.rh = sp.rh;
    p.out_pitch = (int)out_pitch; p.clamp_dc = pl.clamp_dc; p.nframes = n;
    for (int c = 0; c < 3; c++) build_table(d->qt[c], p.tab + TAB_DW * c);
    p.ncols = p.nrows = 0;
    set_frame_ptrs(p.fptr, y, cb, cr, out, f0, n);
    for (int f = 0; f < SCATTER_MAX; f++) {
        p.origin[f] = p.size[f] = p.first[f] = 0;
        if (f >= n) continue;
        const unsigned* const wf = win ? win + 4 * (f0 + f) : nullptr;
        const int x = wf ? (int)wf[0] : 0, yy = wf ? (int)wf[1] : 0, w = wf ? (int)wf[2] : sp.rw, h = wf ? (int)wf[3] : sp.rh;
        const int m0 = x / sp.mw, m1 = (x + w + sp.mw - 1) / sp.mw, r0 = yy / sp.mh, r1 = (yy + h + sp.mh - 1) / sp.mh;
        p.origin[f] = (uint32_t)x | ((uint32_t)yy << 16);
        p.size[f] = (uint32_t)w | ((uint32_t)h << 16);
        p.first[f] = (uint32_t)m0 | ((uint32_t)r0 << 16);
        const int nc = (m1 - m0 + sp.tm - 1) / sp.tm;
        if (nc > p.ncols) p.ncols = nc;
        if (r1 - r0 > p.nrows) p.nrows = r1 - r0;
    }
}

} // namespace zj
