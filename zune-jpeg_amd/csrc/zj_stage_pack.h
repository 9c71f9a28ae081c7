// zj_stage_pack.h -- the host side of the u8 and tensor stages' launches: how a call's images are cut into
// launches, how each launch's record is packed, and the argument rules in front of that -- sizes, pointers, pitches, the
// tensor factors, the planes call's ratios and phases, the warp's fill.  THE one place of each: zj_api.cpp launches the
// records these functions pack, the emulations under tests/emu_* run their lanes over the same records, and
// tests/fuzz/stage_pack_main.cpp checks the records field by field.  Nothing of HIP is called here and no kernel file
// includes it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "zj_cmyk.h"
#include "zj_color.h"
#include "zj_orient.h"
#include "zj_planes.h"
#include "zj_to_tensor.h"
#include "zj_tone.h"
#include "zj_warp.h"

namespace zj {

// f(f0, m) for each launch of a call of n images: images [f0, f0 + m), m <= BATCH; stops at the first status that is not 0
template <int BATCH, class F>
int stage_batches(size_t n, F&& f)
{
    for (size_t f0 = 0; f0 < n; f0 += BATCH) {
        const int m = (int)(n - f0 < (size_t)BATCH ? n - f0 : (size_t)BATCH);
        if (const int rc = f(f0, m)) return rc;
    }
    return 0;
}

/* ---- the slots of a record: slot i < m is image f0 + i of the call, every slot from m on is `tail` ---- */
inline uint64_t stage_ptr(const void* p) { return (uint64_t)(uintptr_t)p; }
inline uint32_t stage_wh(const unsigned* wh, size_t f) { return wh[2 * f] | (wh[2 * f + 1] << 16); }

template <class D, size_t N, class S>
void stage_slots(D (&d)[N], const S* a, size_t step, size_t f0, int m, D tail = D{})
{
    int i = 0;
    for (; i < m; i++) d[i] = (D)a[step * (f0 + i)];
    for (; i < (int)N; i++) d[i] = tail;
}
template <size_t N>
void stage_ptrs(uint64_t (&d)[N], const uint8_t* const* a, size_t step, size_t f0, int m)
{
    int i = 0;
    for (; i < m; i++) d[i] = stage_ptr(a[step * (f0 + i)]);
    for (; i < (int)N; i++) d[i] = 0;
}
template <size_t N>
void stage_whs(uint32_t (&d)[N], const unsigned* wh, size_t f0, int m)
{
    int i = 0;
    for (; i < m; i++) d[i] = stage_wh(wh, f0 + i);
    for (; i < (int)N; i++) d[i] = 0;
}
// a bit set: cleared, then bit i set where flags[f0 + i] (flags nullptr: none)
template <size_t N>
void stage_bits(uint32_t (&d)[N], const uint8_t* flags, size_t f0, int m)
{
    for (size_t k = 0; k < N; k++) d[k] = 0;
    for (int i = 0; flags && i < m; i++)
        if (flags[f0 + i]) d[i >> 5] |= 1u << (i & 31);
}
// what the orient, expand and colour records share: in -> out, w x h, a pitch on each side
template <class P>
void stage_in_out(P& p, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, const uint8_t* const* out,
                  const unsigned* out_pitch, size_t f0, int m)
{
    stage_ptrs(p.in, in, 1, f0, m); stage_ptrs(p.out, out, 1, f0, m);
    stage_whs(p.wh, wh, f0, m);
    stage_slots(p.in_pitch, in_pitch, 1, f0, m); stage_slots(p.out_pitch, out_pitch, 1, f0, m);
}

/* ---- the records: images [f0, f0 + m) of a call whose arrays are indexed by image, the pitches resolved ---- */
// wh: STORED w, h pairs; every o[f] 1..8
inline void pack_orient(OrientParams& p, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, const uint8_t* o,
                        const uint8_t* const* out, const unsigned* out_pitch, size_t f0, int m)
{
    p.nimg = m;
    stage_in_out(p, in, wh, in_pitch, out, out_pitch, f0, m);
    stage_slots(p.o, o, 1, f0, m, (uint8_t)1);
}

inline void pack_expand(ExpandParams& p, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch,
                        const uint8_t* const* out, const unsigned* out_pitch, size_t f0, int m)
{
    p.nimg = m;
    stage_in_out(p, in, wh, in_pitch, out, out_pitch, f0, m);
}

// q: 12 integers per image (color_fixed)
inline void pack_color(ColorParams& p, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, const int32_t* q,
                       const uint8_t* const* out, const unsigned* out_pitch, size_t f0, int m)
{
    p.nimg = m;
    stage_in_out(p, in, wh, in_pitch, out, out_pitch, f0, m);
    for (int i = 0; i < COLOR_BATCH; i++)
        for (int k = 0; k < 12; k++) p.q[i][k] = 0;
    for (int i = 0; i < m; i++)
        for (int k = 0; k < 12; k++) p.q[i][k] = q[12 * (f0 + i) + k];
}

// the tone stages.  hist[f]: image f's table, uint32 [channels][256]
inline void pack_hist(HistParams& p, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, const uint8_t* const* hist,
                      size_t f0, int m)
{
    p.nimg = m;
    stage_ptrs(p.in, in, 1, f0, m); stage_ptrs(p.hist, hist, 1, f0, m);
    stage_whs(p.wh, wh, f0, m);
    stage_slots(p.pitch, pitch, 1, f0, m);
}

// ops: op, param pairs; hist (nullptr: no op needs one): uint32 [n][channels][256], luts: uint8 [n][channels][256] of the call
inline void pack_tone_lut(ToneLutParams& p, const int32_t* ops, const uint32_t* hist, uint8_t* luts, int channels, size_t f0, int m)
{
    p.nimg = m; p.channels = channels;
    p.hist = hist ? stage_ptr(hist + f0 * (size_t)channels * 256) : 0;
    p.luts = stage_ptr(luts + f0 * (size_t)channels * 256);
    stage_slots(p.op, ops, 2, f0, m); stage_slots(p.param, ops + 1, 2, f0, m);
}

// luts: uint8 [n][channels][256] of the call
inline void pack_lut(LutParams& p, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, const uint8_t* luts,
                     int channels, const uint8_t* const* out, const unsigned* out_pitch, size_t f0, int m)
{
    p.nimg = m;
    stage_in_out(p, in, wh, in_pitch, out, out_pitch, f0, m);
    p.luts = stage_ptr(luts + f0 * (size_t)channels * 256);
}

// inverted[f] != 0: the samples are used as stored, else complemented first
inline void pack_cmyk(CmykParams& p, const uint8_t* const* a, const uint8_t* const* k, const unsigned* wh, const unsigned* a_pitch,
                      const unsigned* k_pitch, const uint8_t* inverted, const uint8_t* const* out, const unsigned* out_pitch,
                      size_t f0, int m)
{
    p.nimg = m;
    stage_ptrs(p.a, a, 1, f0, m); stage_ptrs(p.k, k, 1, f0, m); stage_ptrs(p.out, out, 1, f0, m);
    stage_whs(p.wh, wh, f0, m);
    stage_slots(p.a_pitch, a_pitch, 1, f0, m); stage_slots(p.k_pitch, k_pitch, 1, f0, m); stage_slots(p.out_pitch, out_pitch, 1, f0, m);
    stage_bits(p.inverted, inverted, f0, m);
}

// planes[c][step * f]: component c's plane of image f (three arrays: step 1; one array of three per image: step 3); pitch:
// three per image; wh: w, h pairs of the outputs; geo[f]: planes_component of the three components, c in bits 8c .. 8c + 7
inline void pack_planes(PlanesParams& p, const uint8_t* const* const planes[3], size_t step, const unsigned* pitch, const unsigned* wh,
                        const uint32_t* geo, const uint8_t* const* out, const unsigned* out_pitch, size_t f0, int m)
{
    p.nimg = m;
    for (int c = 0; c < 3; c++) {
        stage_ptrs(p.p[c], planes[c], step, f0, m);
        stage_slots(p.pitch[c], pitch + c, 3, f0, m);
    }
    stage_ptrs(p.out, out, 1, f0, m);
    stage_slots(p.out_pitch, out_pitch, 1, f0, m);
    stage_whs(p.wh, wh, f0, m);
    stage_slots(p.geo, geo, 1, f0, m);
}

// The dense tensor a resize, to-tensor or warp call writes: image i of the call at out + i * img_bytes, out_w x out_h of
// dtype (RZ_*), NHWC or NCHW, under the kernel's factors (kernel_factors)
struct StageTensor {
    uint8_t* out;
    size_t img_bytes;
    int out_w, out_h, dtype, nhwc;
    float s[3], b[3];
};

// into images [first + f0, first + f0 + m) of the tensor; flip[f] (nullptr: none): image f's columns mirrored
inline void pack_resize(ResizeParams& p, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, const uint8_t* flip,
                        const StageTensor& t, size_t first, size_t f0, int m)
{
    p.nimg = m;
    p.out_w = t.out_w; p.out_h = t.out_h;
    for (int k = 0; k < 3; k++) { p.scale[k] = t.s[k]; p.bias[k] = t.b[k]; }
    p.groups = (t.out_w + RESIZE_GROUP - 1) / RESIZE_GROUP;
    p.rows = RESIZE_ITEMS / p.groups;
    if (p.rows < 1) p.rows = 1;
    if (p.rows > t.out_h) p.rows = t.out_h;
    p.out = stage_ptr(t.out + (first + f0) * t.img_bytes);
    stage_ptrs(p.in, in, 1, f0, m);
    stage_whs(p.wh, wh, f0, m);
    stage_slots(p.pitch, pitch, 1, f0, m);
    stage_bits(p.flip, flip, f0, m);
}

// images of t.out_w x t.out_h and cin channels each into cout channels
inline void pack_to_tensor(ToTensorParams& p, const uint8_t* const* in, const unsigned* pitch, const uint8_t* flip, int cin, int cout,
                           const StageTensor& t, size_t f0, int m)
{
    p.nimg = m;
    p.w = t.out_w; p.h = t.out_h; p.cin = cin; p.cout = cout; p.dtype = t.dtype; p.nhwc = t.nhwc;
    for (int k = 0; k < 3; k++) { p.scale[k] = t.s[k]; p.bias[k] = t.b[k]; }
    p.out = stage_ptr(t.out + f0 * t.img_bytes);
    stage_ptrs(p.in, in, 1, f0, m);
    stage_slots(p.pitch, pitch, 1, f0, m);
    stage_bits(p.flip, flip, f0, m);
}

// q: six integers per image (warp_fixed); fill: warp_fill.  wh[2f] == 0: no image at all -- every tap of the output is
// outside (fill mode alone): the record is a 1 x 1 image that no lane loads from, under a map that sends every pixel to x0 = -4
inline void pack_warp(WarpParams& p, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, const int64_t* q,
                      uint32_t fill, int edge, const StageTensor& t, size_t first, size_t f0, int m)
{
    p.nimg = m;
    p.out_w = t.out_w; p.out_h = t.out_h; p.dtype = t.dtype; p.nhwc = t.nhwc;
    p.fill = fill; p.edge = edge;
    for (int k = 0; k < 3; k++) { p.scale[k] = t.s[k]; p.bias[k] = t.b[k]; }
    p.out = stage_ptr(t.out + (first + f0) * t.img_bytes);
    for (int i = 0; i < WARP_BATCH; i++) {
        const size_t f = f0 + i;
        WarpImage& im = p.img[i];
        im = WarpImage{};
        if (i >= m) continue;
        if (wh[2 * f] == 0) {
            im.in = stage_ptr(t.out); // (never loaded from)
            im.wh = 1u | 1u << 16; im.pitch = 1;
            im.m[2] = im.m[5] = -((int64_t)4 << WARP_Q);
            continue;
        }
        im.in = stage_ptr(in[f]);
        im.wh = stage_wh(wh, f);
        im.pitch = pitch[f];
        for (int k = 0; k < 6; k++) im.m[k] = q[6 * f + k];
    }
}

/* ---- the argument rules; false: the call is refused ---- */
inline bool finite_f32(float v) { return v - v == 0.f; }

// The per-channel factors of the tensor kernels from the caller's scale / bias (nullptr: 1, 0; read for the first `channels`
// only): s_c = scale_c * 2^-16 -- exact: a power of two, above float32's smallest normal for every |scale| >= 2^-110 -- and
// b_c = bias_c.  false: a factor that is not finite.
inline bool kernel_factors(const float* scale, const float* bias, int channels, float s[3], float b[3])
{
    for (int k = 0; k < 3; k++) {
        const float sc = scale && k < channels ? scale[k] : 1.f, bi = bias && k < channels ? bias[k] : 0.f;
        if (!finite_f32(sc) || !finite_f32(bi)) return false;
        s[k] = sc * (1.f / 65536.f);
        b[k] = bi;
    }
    return true;
}

// THE size / pointer / pitch rule of the stage calls.  An image is 1..65535 pixels each way ...
inline bool stage_size(unsigned w, unsigned h) { return w != 0 && h != 0 && w <= 65535 && h <= 65535; }
inline bool stage_sizes(size_t n, const unsigned* wh)
{
    for (size_t f = 0; f < n; f++)
        if (!stage_size(wh[2 * f], wh[2 * f + 1])) return false;
    return true;
}
// ... rows of `row` bytes lie pitch[f] bytes apart (pitch nullptr or 0: tight), from a row up to 2^24 ...
inline bool stage_pitch(const unsigned* pitch, size_t f, size_t row, unsigned& resolved)
{
    resolved = pitch && pitch[f] ? pitch[f] : (unsigned)row;
    return resolved >= row && resolved <= (1u << 24);
}
// ... and one side of a call -- its inputs, its outputs, one of its planes -- has a pointer for every image and resolves
// its pitches against the rows row(f)
template <class Row>
bool stage_side(size_t n, const uint8_t* const* ptr, const unsigned* pitch, Row&& row, std::vector<unsigned>& resolved)
{
    resolved.resize(n);
    for (size_t f = 0; f < n; f++)
        if (!ptr[f] || !stage_pitch(pitch, f, row(f), resolved[f])) return false;
    return true;
}
// (rows of wh[2f] pixels of row_channels bytes)
inline bool stage_side(size_t n, const uint8_t* const* ptr, const unsigned* pitch, const unsigned* wh, int row_channels,
                       std::vector<unsigned>& resolved)
{
    return stage_side(n, ptr, pitch, [=](size_t f) { return (size_t)wh[2 * f] * row_channels; }, resolved);
}
// (the images a call reads: their sizes and that side)
inline bool stage_images(size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, int row_channels,
                         std::vector<unsigned>& resolved)
{
    return stage_sizes(n, wh) && stage_side(n, in, pitch, wh, row_channels, resolved);
}

// A component of the planes call in an image w wide: ratios rx, ry of 1, 2 or 4, phases px < rx, py < ry (x mod rx, y mod ry
// of the image's first pixel).  pw: the samples of a row that the image shows; geo: the component's byte of PlanesParams::geo
inline bool planes_component(unsigned w, unsigned rx, unsigned ry, unsigned px, unsigned py, unsigned& pw, uint32_t& geo)
{
    if ((rx != 1 && rx != 2 && rx != 4) || (ry != 1 && ry != 2 && ry != 4) || px >= rx || py >= ry) return false;
    pw = (px + w + rx - 1) / rx;
    geo = planes_geo((int)rx >> 1, (int)ry >> 1, (int)px, (int)py); // (log2 of 1, 2, 4: 0, 1, 2)
    return true;
}

// the warp's fill bytes as the record takes them: fill[c] << 8 c (nullptr: 0)
inline uint32_t warp_fill(const uint8_t* fill, int channels)
{
    uint32_t v = 0;
    for (int k = 0; fill && k < channels; k++) v |= (uint32_t)fill[k] << (8 * k);
    return v;
}

} // namespace zj
