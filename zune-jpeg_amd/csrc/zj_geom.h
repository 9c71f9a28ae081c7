// zj_geom.h -- the pure size and window rules of the output modes: what a window of a frame, a reduced frame or a resized
// crop measures and whether it is one.  Nothing of HIP here: zj_plan.h builds the launch plans on these rules, and the
// JPEG front-end (zj_jpeg.cpp), whose CPU-only builds link without the device half of the library, checks its arguments
// with the same ones.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/zjhip.h"

namespace zj {

constexpr size_t OUT_PITCH_MAX = (size_t)1 << 20; // bytes between the rows of an output
constexpr int RESIZE_MAX_OUT = 8192;              // out_w, out_h of a resized output

inline int ncomp_of(int cs)
{
    switch (cs) {
    case ZJ_CS_RGB: case ZJ_CS_YCBCR: return 3;
    case ZJ_CS_GRAYSCALE: return 1;
    case ZJ_CS_CMYK: case ZJ_CS_YCCK: case ZJ_CS_RGBA: case ZJ_CS_RGBX: return 4;
    default: return 0;
    }
}

// An ALL-ZERO output: a single-component frame asked for a colour output, which the reference converts nothing of and
// returns as zeros (worker.rs:131; the decoder's finish path)
inline bool zero_output(const zj_frame_desc* d) { return d && d->in_components == 1 && d->out_colorspace != ZJ_CS_GRAYSCALE; }

// channels of the resized or reduced output of descriptor d: 3 (RGB, YCbCr), 1 (GRAYSCALE), 0 (no such output: RGBA / RGBX)
inline int resize_channels(const zj_frame_desc* d)
{
    if (!d) return 0;
    if (d->out_colorspace == ZJ_CS_RGB || d->out_colorspace == ZJ_CS_YCBCR) return 3;
    return d->out_colorspace == ZJ_CS_GRAYSCALE ? 1 : 0;
}

// ZJ_FLAG_GRAY_TO_RGB, which the resized-crop calls alone honour.  gray_to_rgb: d is a one-component frame
// that the flag turns into an RGB image with R = G = B.  gray_to_rgb_refused: the flag on a one-component frame asked for
// YCbCr, which has no such form.  resized_stage_desc: the descriptor the stages in front of the resize run with -- the flag
// stripped (every plan refuses an unknown bit), a gray_to_rgb frame decoded as GRAYSCALE; anything else as it is.
inline bool gray_to_rgb(const zj_frame_desc* d)
{
    return d && (d->flags & ZJ_FLAG_GRAY_TO_RGB) && d->in_components == 1 && d->out_colorspace == ZJ_CS_RGB;
}
inline bool gray_to_rgb_refused(const zj_frame_desc* d)
{
    return d && (d->flags & ZJ_FLAG_GRAY_TO_RGB) && d->in_components == 1 && d->out_colorspace == ZJ_CS_YCBCR;
}
inline zj_frame_desc resized_stage_desc(const zj_frame_desc* d)
{
    zj_frame_desc e = *d;
    e.flags &= ~(uint32_t)ZJ_FLAG_GRAY_TO_RGB;
    if (gray_to_rgb(d)) e.out_colorspace = ZJ_CS_GRAYSCALE;
    return e;
}

// ---- windows --------------------------------------------------------------------------------------------------------
// A window of w x h pixels of an output of d's format, its rows out_pitch bytes apart (0: tight), laid out by zj_out_len's
// arithmetic: rows of w x bpp bytes, CHW RGB: w bytes in each of 3 planes.
struct WindowLayout {
    int bpp, nplanes;   // bytes per pixel of a row (CHW: 1, per plane); 3 planes for CHW, else 1
    size_t tight;       // bytes of a row
    size_t pitch;       // bytes between rows
    size_t len;         // bytes of the window, all planes
};

inline WindowLayout window_layout(int bpp, int nplanes, unsigned w, unsigned h, unsigned out_pitch)
{
    WindowLayout g;
    g.bpp = bpp; g.nplanes = nplanes;
    g.tight = (size_t)w * bpp;
    g.pitch = out_pitch ? (size_t)out_pitch : g.tight;
    g.len = g.pitch * h * nplanes;
    return g;
}

inline WindowLayout window_layout(const zj_frame_desc* d, unsigned w, unsigned h, unsigned out_pitch)
{
    const bool chw = d->out_layout == ZJ_LAYOUT_CHW && d->out_colorspace == ZJ_CS_RGB;
    return window_layout(chw ? 1 : ncomp_of(d->out_colorspace), chw ? 3 : 1, w, h, out_pitch);
}

// is x, y, w, h at layout g a window of a frame of fw x fh pixels (its pitch at least a row; window_pitch_ok: and no more
// than an output's may be)
inline bool window_inside(const WindowLayout& g, unsigned x, unsigned y, unsigned w, unsigned h, unsigned fw, unsigned fh)
{
    return w != 0 && h != 0 && g.pitch >= g.tight && (size_t)x + w <= fw && (size_t)y + h <= fh;
}
inline bool window_pitch_ok(const WindowLayout& g) { return g.pitch >= g.tight && g.pitch <= OUT_PITCH_MAX; }

// ---- reduced-size decode ----------------------------------------------------------------------------
// a side of the frame reduced by 2^k: ceil(n / 2^k)
inline unsigned reduced_dim(unsigned n, int k) { return (n + (1u << k) - 1) >> k; }

// the scale of one image under a resize to out_w x out_h: the largest k <= max_log2 with floor(w / 2^k) >= out_w and
// floor(h / 2^k) >= out_h (0: none) -- the resize that follows never enlarges
inline int prescale_pick(unsigned w, unsigned h, unsigned out_w, unsigned out_h, int max_log2)
{
    int k = 0;
    for (int c = 1; c <= max_log2; c++)
        if ((w >> c) >= out_w && (h >> c) >= out_h) k = c;
    return k;
}
// the window of the reduced frame that covers the full-resolution window x, y, w, h:
// [floor(x / s), ceil((x + w) / s)) x [floor(y / s), ceil((y + h) / s)), clipped to the reduced frame
inline void prescale_window(const unsigned full[4], int k, unsigned width, unsigned height, unsigned red[4])
{
    const unsigned rw = reduced_dim(width, k), rh = reduced_dim(height, k);
    unsigned x1 = reduced_dim(full[0] + full[2], k), y1 = reduced_dim(full[1] + full[3], k);
    if (x1 > rw) x1 = rw;
    if (y1 > rh) y1 = rh;
    red[0] = full[0] >> k; red[1] = full[1] >> k;
    red[2] = x1 - red[0]; red[3] = y1 - red[1];
}

// ---- EXIF orientation -------------------------------------------------------------------------------
// o = 1..8 turns the stored image S (h rows of w pixels) into the displayed one D.  D[r][c] = S[sr][sc] with (a, b) =
// (c, r) for the transposing orientations 5..8, else (r, c); sr = a or h - 1 - a, sc = b or w - 1 - b:
//   o            1  2  3  4  5  6  7  8
//   transposes   .  .  .  .  x  x  x  x
//   rows turned  .  .  x  x  .  x  x  .      (sr = h - 1 - a)
//   cols turned  .  x  x  .  .  .  x  x      (sc = w - 1 - b)
// (constexpr: the kernel calls them too)
constexpr bool orient_valid(const int o) { return o >= 1 && o <= 8; }
constexpr bool orient_transposes(const int o) { return o >= 5; }
constexpr bool orient_turns_rows(const int o) { return o == 3 || o == 4 || o == 6 || o == 7; }
constexpr bool orient_turns_cols(const int o) { return o == 2 || o == 3 || o == 7 || o == 8; }

// size of D for a stored w x h
inline bool orient_size(int o, unsigned w, unsigned h, unsigned* ow, unsigned* oh)
{
    if (!orient_valid(o)) return false;
    *ow = orient_transposes(o) ? h : w;
    *oh = orient_transposes(o) ? w : h;
    return true;
}

// the window x, y, w, h of D (a stored frame of fw x fh) as a window of S: orienting that stored window gives exactly
// D[y : y + h, x : x + w].  false: not an orientation, or not a window of D
inline bool orient_window(int o, unsigned fw, unsigned fh, const unsigned win[4], unsigned stored[4])
{
    unsigned dw, dh;
    if (!orient_size(o, fw, fh, &dw, &dh)) return false;
    const unsigned x = win[0], y = win[1], w = win[2], h = win[3];
    if (w == 0 || h == 0 || (size_t)x + w > dw || (size_t)y + h > dh) return false;
    // displayed columns run along the stored b axis (the stored rows, when transposing), displayed rows along a
    const unsigned b0 = orient_transposes(o) ? y : x, nb = orient_transposes(o) ? h : w;
    const unsigned a0 = orient_transposes(o) ? x : y, na = orient_transposes(o) ? w : h;
    stored[0] = orient_turns_cols(o) ? fw - b0 - nb : b0;
    stored[1] = orient_turns_rows(o) ? fh - a0 - na : a0;
    stored[2] = nb; stored[3] = na;
    return true;
}

// ---- resized outputs --------------------------------------------------------------------------------
// bytes of an element of ZJ_DTYPE_* dt, 0: no such dtype (constexpr: the kernels call it with their template argument)
constexpr int resize_elem_bytes(const int dt)
{
    return dt == ZJ_DTYPE_F32 ? 4 : (dt == ZJ_DTYPE_F16 || dt == ZJ_DTYPE_BF16) ? 2 : (dt == ZJ_DTYPE_U8 ? 1 : 0);
}

// bytes of one image of a resized output, 0: not a valid size (1..RESIZE_MAX_OUT each way), dtype or channel count
inline size_t resized_len(int channels, unsigned out_w, unsigned out_h, int dtype)
{
    if (channels <= 0 || out_w == 0 || out_h == 0 || out_w > (unsigned)RESIZE_MAX_OUT || out_h > (unsigned)RESIZE_MAX_OUT) return 0;
    return (size_t)channels * out_w * out_h * resize_elem_bytes(dtype);
}

} // namespace zj
