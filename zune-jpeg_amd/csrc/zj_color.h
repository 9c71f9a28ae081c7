// zj_color.h -- a 3-channel u8 image under a per-image colour matrix (zj_color_device): brightness, contrast,
// saturation, hue, grayscale, a channel order -- any affine map of (R, G, B), in exact integers:
//   v = q[c][0] R + q[c][1] G + q[c][2] B + q[c][3],   out[c] = clamp((v + 32768) >> 16, 0, 255)   (arithmetic shift)
// with q[c][k] = floor(m[c][k] 65536 + 1/2) (color_fixed).  |q[c][0..2]| <= 2^20 fits a 24-bit operand, and
// |v| <= 3 x 255 x 2^20 + 2^28 + 2^15 < 2^31: plain 32-bit arithmetic.
//
// The launch's arguments and one lane's work as ZJ_HD functions, shared by the kernel (zj_color.hip) and its CPU emulation
// (tests/emu_color, a g++ ZJ_EMU build that runs them lane by lane).
//   color_fixed    (zj_color_fixed.h, host) the 12 integers of a matrix of doubles, or false: an entry the stage refuses
//   ColorParams    one launch: up to COLOR_BATCH images of their own sizes, pitches and destinations, 12 integers each
//   color_item     the run a lane owns: COLOR_RUN consecutive pixels of one row (the last run of a row: what is left)
//   color_pixel    one channel of one pixel
//   cmyk_get       (zj_cmyk.h) nb bytes of a run into dwords, never a byte outside the run
//   expand_put     (zj_expand.h) the run's bytes stored the same way; never a byte outside the run's own
// A lane reads the whole of its run before it stores any of it, and no other lane touches those bytes: the output may be the
// input itself (same address, same pitch).  The image is the grid's z: its 12 integers are the same over a workgroup and stay
// in scalar registers.  No LDS, no lane talks to another.
#pragma once
#include "zj_cmyk.h" // cmyk_get; zj_expand.h: expand_put
#include "zj_color_fixed.h" // color_fixed, color_is_identity: the host side

namespace zj {

constexpr int COLOR_RUN = 16;    // pixels of one row per lane: 48 bytes loaded, 48 stored
constexpr int COLOR_NT = 256;    // threads per workgroup
constexpr int COLOR_BATCH = 48;  // images per launch: 76 bytes of kernel arguments each

struct ColorParams {
    uint64_t in[COLOR_BATCH], out[COLOR_BATCH];
    uint32_t wh[COLOR_BATCH];                                 // w | h << 16
    uint32_t in_pitch[COLOR_BATCH], out_pitch[COLOR_BATCH];   // bytes between rows (CHW: of a plane's rows)
    int32_t q[COLOR_BATCH][12];                               // q[c][k] at 4 c + k
    int nimg;
};
static_assert(sizeof(ColorParams) <= 4096, "kernel arguments: 4 KB");
static_assert(sizeof(ColorParams) == 76 * COLOR_BATCH + 8, "76 bytes an image");

ZJ_HD int color_runs(const int w) { return (w + COLOR_RUN - 1) / COLOR_RUN; }
ZJ_HD int color_grid(const ColorParams& p)
{
    long long most = 1;
    for (int i = 0; i < p.nimg; i++) {
        const long long items = (long long)color_runs((int)(p.wh[i] & 0xffffu)) * (long long)(p.wh[i] >> 16);
        if (items > most) most = items;
    }
    return (int)((most + COLOR_NT - 1) / COLOR_NT);
}

struct ColorItem {
    uint64_t src, dst;            // the run's first byte of the input and of the output (CHW: of plane 0)
    uint64_t in_plane, out_plane; // CHW: bytes between the planes
    int n;                        // pixels of the run, 0: this lane owns nothing
};

// item `id` (workgroup x COLOR_NT + lane) of image img: run id % runs of row id / runs
template <bool CHW>
ZJ_HD ColorItem color_item(const ColorParams& p, const int img, const uint32_t id)
{
    ColorItem it;
    const int w = (int)(p.wh[img] & 0xffffu), h = (int)(p.wh[img] >> 16);
    const uint32_t runs = (uint32_t)color_runs(w);
    it.src = it.dst = it.in_plane = it.out_plane = 0; it.n = 0;
    if (runs == 0) return it;
    const uint32_t row = id / runs, x0 = (id - row * runs) * COLOR_RUN;
    if (row >= (uint32_t)h) return it;
    it.n = w - (int)x0 < COLOR_RUN ? w - (int)x0 : COLOR_RUN;
    it.src = p.in[img] + (uint64_t)row * p.in_pitch[img] + (uint64_t)x0 * (CHW ? 1 : 3);
    it.dst = p.out[img] + (uint64_t)row * p.out_pitch[img] + (uint64_t)x0 * (CHW ? 1 : 3);
    it.in_plane = (uint64_t)p.in_pitch[img] * (uint64_t)h;
    it.out_plane = (uint64_t)p.out_pitch[img] * (uint64_t)h;
    return it;
}

// q x + acc, q within 24 bits signed and x a byte: v_mad_i32_i24
ZJ_HD int32_t color_mad(const int32_t q, const uint32_t x, const int32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(q, (int32_t)x) + acc;
#else
    return q * (int32_t)x + acc;
#endif
}

// one channel of one pixel: q = its row's three factors and its offset with the rounding half already in it (q3 + 32768)
ZJ_HD uint32_t color_pixel(const int32_t q0, const int32_t q1, const int32_t q2, const int32_t q3h, const uint32_t r, const uint32_t g,
                           const uint32_t b)
{
    // clamp((v + 32768) >> 16, 0, 255) as clamp(v + 32768, 0, 2^24 - 1) >> 16: the same value for every v, and the byte is
    // bits 16..23 of one v_med3_i32 (clamping after the shift, the compiler packs pairs with v_ashr_pk_u8_i32 and then ORs
    // the other bytes into that register's upper half, which the instruction does not clear)
    const int32_t t = color_mad(q0, r, color_mad(q1, g, color_mad(q2, b, q3h)));
    return (uint32_t)(t < 0 ? 0 : t > 0x00ffffff ? 0x00ffffff : t) >> 16;
}

// byte k of the dwords v
template <int ND>
ZJ_HD uint32_t color_byte(const uint32_t (&v)[ND], const int k) { return (v[k >> 2] >> (8 * (k & 3))) & 255u; }

// One lane's work: its run loaded, every pixel mapped, and stored
template <bool CHW>
ZJ_HD void color_lane(const ColorParams& p, const int img, const uint32_t id)
{
    const ColorItem it = color_item<CHW>(p, img, id);
    if (it.n == 0) return;
    int32_t q[12];
#pragma unroll
    for (int k = 0; k < 12; k++) q[k] = p.q[img][k] + ((k & 3) == 3 ? 32768 : 0);
    if (CHW) {
        uint32_t a[3][4], o[3][4];
#pragma unroll
        for (int c = 0; c < 3; c++) cmyk_get<4>(it.src + (uint64_t)c * it.in_plane, a[c], it.n); // (all read before any is stored)
#pragma unroll
        for (int c = 0; c < 3; c++) {
#pragma unroll
            for (int i = 0; i < 4; i++) o[c][i] = 0;
        }
#pragma unroll
        for (int i = 0; i < COLOR_RUN; i++) {
            const uint32_t r = color_byte<4>(a[0], i), g = color_byte<4>(a[1], i), b = color_byte<4>(a[2], i);
#pragma unroll
            for (int c = 0; c < 3; c++)
                o[c][i >> 2] |= color_pixel(q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3], r, g, b) << (8 * (i & 3));
        }
#pragma unroll
        for (int c = 0; c < 3; c++) expand_put<4>(it.dst + (uint64_t)c * it.out_plane, o[c], it.n);
    } else {
        uint32_t a[12], o[12];
        cmyk_get<12>(it.src, a, 3 * it.n);
#pragma unroll
        for (int i = 0; i < 12; i++) o[i] = 0;
#pragma unroll
        for (int i = 0; i < COLOR_RUN; i++) {
            const uint32_t r = color_byte<12>(a, 3 * i), g = color_byte<12>(a, 3 * i + 1), b = color_byte<12>(a, 3 * i + 2);
#pragma unroll
            for (int c = 0; c < 3; c++)
                o[(3 * i + c) >> 2] |= color_pixel(q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3], r, g, b) << (8 * ((3 * i + c) & 3));
        }
        expand_put<12>(it.dst, o, 3 * it.n);
    }
}

} // namespace zj
