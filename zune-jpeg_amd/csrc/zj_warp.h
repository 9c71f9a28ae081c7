// zj_warp.h -- affine-warped u8 images into one normalised tensor (zj_warp_device).
//
// The launch's arguments and one lane's work as ZJ_HD functions, shared by the kernel (zj_warp.hip) and its CPU emulation
// (tests/emu_warp, a g++ ZJ_EMU build that runs them lane by lane, with a write map and a check of every load).
//   WarpImage    one image of a launch: its first byte, size, pitch and the six integers of its matrix (Q24)
//   WarpParams   one launch: up to WARP_BATCH images of their own sizes into consecutive images of the tensor
//   warp_pos     one axis of one output pixel: U -> the first tap's index (clamped to just outside the image) and the
//                weight in 1/256
//   warp_lane    the item a lane owns: WARP_GROUP consecutive output pixels of one row, every channel; the groups of a
//                row are shifted so that a full group starts on a store boundary of the DESTINATION; the pixels in front
//                of a row's first full group and behind its last go out element by element
// The value of an element is zj_resize.h's resize_value over the four taps, its conversion that header's too.  No LDS, no
// lane talks to another.  dtype, layout and edge mode are switches that are uniform over a workgroup.
#pragma once
#include "zj_resize.h" // ZJ_HD, ZJ_RZ_GLOBAL, resize_value, the conversions, resize_elem

namespace zj {

constexpr int WARP_Q = 24;       // fraction bits of the matrix's integers
constexpr int WARP_GROUP = 8;    // output pixels of one row per lane
constexpr int WARP_NT = 256;     // threads per workgroup
constexpr int WARP_BX = 8;       // groups of a row per workgroup: 64 pixels ...
constexpr int WARP_BY = 32;      // ... by 32 rows, a block whose source footprint stays small under any rotation
constexpr int WARP_BATCH = 48;   // images per launch (64 bytes of kernel arguments each)
static_assert(WARP_BX * WARP_BY == WARP_NT, "one lane per group of the block");
enum { WARP_FILL = 0, WARP_REPLICATE = 1 };

struct WarpImage {
    uint64_t in;        // first byte
    uint32_t wh;        // w | h << 16 (1..65535 each)
    uint32_t pitch;     // bytes between rows
    int64_t m[6];       // A, B, C0, D, E, F0: Ux = A X + B Y + C0, Uy = D X + E Y + F0 (units of 2^-24 pixel)
};
static_assert(sizeof(WarpImage) == 64, "the per-image record");

struct WarpParams {
    WarpImage img[WARP_BATCH];
    uint64_t out;               // the launch's first image of the tensor
    float scale[3], bias[3];    // per channel: s_c = scale_c * 2^-16, bias_c (zj_resize.h: ResizeParams)
    uint32_t fill;              // fill[c] << 8 c
    int out_w, out_h, nimg;
    int dtype;                  // ZJ_DTYPE_*
    int nhwc;                   // 1: [h, w, C], 0: [C, h, w]
    int edge;                   // WARP_FILL, WARP_REPLICATE
};
static_assert(sizeof(WarpParams) <= 4096, "kernel arguments: 4 KB");

struct alignas(16) WarpV4 { uint32_t x, y, z, w; };
struct alignas(8) WarpV2 { uint32_t x, y; };

// a store and a load of the kernel (the emulation counts the stores in its write map and checks the loads here)
#if !defined(ZJ_WP_PUT)
#define ZJ_WP_PUT(T, addr, v) (*ZJ_RZ_GLOBAL(T, addr) = (v))
#endif
#if !defined(ZJ_WP_GET)
#define ZJ_WP_GET(T, addr) (*ZJ_RZ_GLOBAL(const T, addr))
#endif

// groups of a row: the first may hold a single pixel in front of the first boundary
ZJ_HD uint32_t warp_row_groups(const int out_w) { return ((uint32_t)out_w + WARP_GROUP - 1) / WARP_GROUP + 1; }
// the launch's grid: blocks along a row (x), blocks of rows (y); the images are z
ZJ_HD uint32_t warp_grid_x(const int out_w) { return (warp_row_groups(out_w) + WARP_BX - 1) / WARP_BX; }
ZJ_HD uint32_t warp_grid_y(const int out_h) { return ((uint32_t)out_h + WARP_BY - 1) / WARP_BY; }

// One axis: U (units of 2^-24) -> u = U >> 16 (a floor: 1/256 pixel), the first tap i0 = u >> 8, f = u & 255.  i0 is
// clamped to [-2, n]: at -2 and at n both taps i0, i0 + 1 lie outside [0, n) as they do for every index beyond.
ZJ_HD int warp_pos(const int64_t U, const int n, uint32_t& f)
{
    const int64_t u = U >> 16;
    f = (uint32_t)u & 255u;
    const int64_t i = u >> 8;
    return i < -2 ? -2 : (i > (int64_t)n ? n : (int)i);
}

ZJ_HD int warp_clamp(const int i, const int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the pixels of a row that lie in front of its first full group, 0..7: the smallest k with the element of pixel k on a
// store boundary.  a: address of the row's first element; E: bytes of an element; m: elements of a pixel in the run (NHWC:
// C, else 1).  The boundary is 16 bytes, or the group's own 8 bytes for one-byte pixels, and 8 for three-byte ones (their
// groups of 24 bytes go out as three 8-byte stores).  m is 1 or 3, its own inverse modulo 4 and 8.
ZJ_HD int warp_lead(const uint64_t a, const int E, const int m)
{
    const uint32_t q = E == 4 ? 4u : 8u;                      // elements between boundaries
    const uint32_t r = (uint32_t)(a / (uint64_t)E) & (q - 1u); // the row's first element, counted from a boundary
    return (int)(((q - r) * (uint32_t)m) & (q - 1u));
}

// NW dwords of converted elements to dst: whole (cnt == WARP_GROUP pixels) with the widest stores the address allows,
// else the first nel elements one by one
template <int E, int NW>
ZJ_HD void warp_store(const uint64_t dst, const uint32_t (&w)[NW], const bool whole, const int nel)
{
    if (whole && NW % 4 == 0 && (dst & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < NW / 4; k++) ZJ_WP_PUT(WarpV4, dst + 16 * k, (WarpV4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]}));
    } else if (whole && NW % 2 == 0 && (dst & 7u) == 0) {
#pragma unroll
        for (int k = 0; k < NW / 2; k++) ZJ_WP_PUT(WarpV2, dst + 8 * k, (WarpV2{w[2 * k], w[2 * k + 1]}));
    } else if (whole && (dst & 3u) == 0) {
#pragma unroll
        for (int k = 0; k < NW; k++) ZJ_WP_PUT(uint32_t, dst + 4 * k, w[k]);
    } else {
#pragma unroll
        for (int k = 0; k < NW * 4 / E; k++) {
            if (k >= nel) continue;
            const uint32_t x = w[k * E / 4] >> (8 * ((k * E) % 4));
            if (E == 1) ZJ_WP_PUT(uint8_t, dst + k, (uint8_t)x);
            else if (E == 2) ZJ_WP_PUT(uint16_t, dst + 2 * k, (uint16_t)x);
            else ZJ_WP_PUT(uint32_t, dst + 4 * k, x);
        }
    }
}

// the values v[k * C + c] of cnt pixels (pixel k of the lane, channel c) converted and stored: pixel k is column x0 + k of
// row r of the image at img_out
template <int C, int DT, bool NHWC>
ZJ_HD void warp_emit(const WarpParams& p, const uint32_t (&v)[WARP_GROUP * C], const uint64_t img_out, const int r, const int x0,
                     const int cnt)
{
    constexpr int G = WARP_GROUP, E = resize_elem_bytes(DT);
    constexpr int RUNS = NHWC ? 1 : C, RUN = NHWC ? G * C : G, NW = RUN * E / 4;
#pragma unroll
    for (int q = 0; q < RUNS; q++) {
        uint32_t w[NW];
#pragma unroll
        for (int wi = 0; wi < NW; wi++) {
            if (DT == RZ_F32) {
                const int c = NHWC ? wi % C : q;
                w[wi] = f32_bits(resize_f32(v[NHWC ? wi : wi * C + q], p.scale[c], p.bias[c]));
            } else if (DT == RZ_U8) {
                uint32_t d = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) d |= resize_u8(v[NHWC ? 4 * wi + b : (4 * wi + b) * C + q]) << (8 * b);
                w[wi] = d;
            } else {
                const int j0 = 2 * wi, j1 = 2 * wi + 1;
                const int c0 = NHWC ? j0 % C : q, c1 = NHWC ? j1 % C : q;
                const float a = resize_f32(v[NHWC ? j0 : j0 * C + q], p.scale[c0], p.bias[c0]);
                const float b = resize_f32(v[NHWC ? j1 : j1 * C + q], p.scale[c1], p.bias[c1]);
                w[wi] = resize_pack2<DT>(a, b);
            }
        }
        const uint64_t dst = img_out + (uint64_t)(resize_elem<C, NHWC>(NHWC ? 0 : q, r, x0, p.out_w, p.out_h) * E);
        warp_store<E, NW>(dst, w, cnt == G, NHWC ? cnt * C : cnt);
    }
}

// One lane's work: group g of output row r of image z.  The group's pixels are columns [G g - G + lead, G g + lead) cut to
// the row, lead computed from the address of the row's first element.  A pixel outside the row is never written; its
// taps are those of the group's last pixel again (skipping them per pixel was tried: the branches cost the three-channel
// kernel 224 VGPRs in place of 134).  A tap outside the image is never loaded.
template <int C>
ZJ_HD void warp_lane_c(const WarpParams& p, const int z, const int r, const uint32_t g)
{
    constexpr int G = WARP_GROUP;
    const int ow = p.out_w, oh = p.out_h;
    if (r >= oh || g >= warp_row_groups(ow)) return;
    const bool nhwc = p.nhwc != 0 || C == 1;
    const int E = resize_elem_bytes(p.dtype);
    const uint64_t img_out = p.out + (uint64_t)z * (uint64_t)C * (uint64_t)ow * (uint64_t)oh * (uint64_t)E;
    const uint64_t row = img_out + (uint64_t)((long long)r * ow * (nhwc ? C : 1)) * (uint64_t)E;
    const int lead = warp_lead(row, E, nhwc ? C : 1);
    int x0 = G * (int)g - G + lead, x1 = x0 + G;
    if (x0 < 0) x0 = 0; // (lead == 0: group 0 is empty)
    if (x1 > ow) x1 = ow;
    if (x0 >= x1) return;
    const int cnt = x1 - x0;
    const WarpImage& im = p.img[z];
    const int w = (int)(im.wh & 0xffffu), h = (int)(im.wh >> 16);
    const bool rep = p.edge == WARP_REPLICATE;
    const uint32_t fill[3] = {p.fill & 255u, (p.fill >> 8) & 255u, (p.fill >> 16) & 255u};
    int64_t Ux = im.m[0] * x0 + im.m[1] * r + im.m[2];
    int64_t Uy = im.m[3] * x0 + im.m[4] * r + im.m[5];
    uint32_t v[G * C];
#pragma unroll
    for (int k = 0; k < G; k++) {
        uint32_t fx, fy;
        int xa = warp_pos(Ux, w, fx), ya = warp_pos(Uy, h, fy);
        int xb = xa + 1, yb = ya + 1;
        if (k + 1 < cnt) { Ux += im.m[0]; Uy += im.m[3]; } // (past the group's end: the last pixel again)
        bool inxa = true, inxb = true, inya = true, inyb = true;
        if (rep) {
            xa = warp_clamp(xa, w); xb = warp_clamp(xb, w); ya = warp_clamp(ya, h); yb = warp_clamp(yb, h);
        } else {
            inxa = xa >= 0 && xa < w; inxb = xb >= 0 && xb < w; inya = ya >= 0 && ya < h; inyb = yb >= 0 && yb < h;
        }
        const uint64_t ra = im.in + (uint64_t)((long long)ya * im.pitch), rb = im.in + (uint64_t)((long long)yb * im.pitch);
#pragma unroll
        for (int c = 0; c < C; c++) {
            const uint32_t p00 = inya && inxa ? ZJ_WP_GET(uint8_t, ra + (uint64_t)(xa * C + c)) : fill[c];
            const uint32_t p01 = inya && inxb ? ZJ_WP_GET(uint8_t, ra + (uint64_t)(xb * C + c)) : fill[c];
            const uint32_t p10 = inyb && inxa ? ZJ_WP_GET(uint8_t, rb + (uint64_t)(xa * C + c)) : fill[c];
            const uint32_t p11 = inyb && inxb ? ZJ_WP_GET(uint8_t, rb + (uint64_t)(xb * C + c)) : fill[c];
            v[k * C + c] = resize_value(p00, p01, p10, p11, fx, fy);
        }
    }
    // (a one-channel tensor: the two layouts are one)
    if (nhwc) {
        switch (p.dtype) {
        case RZ_F32: warp_emit<C, RZ_F32, true>(p, v, img_out, r, x0, cnt); break;
        case RZ_F16: warp_emit<C, RZ_F16, true>(p, v, img_out, r, x0, cnt); break;
        case RZ_BF16: warp_emit<C, RZ_BF16, true>(p, v, img_out, r, x0, cnt); break;
        default: warp_emit<C, RZ_U8, true>(p, v, img_out, r, x0, cnt); break;
        }
    } else {
        switch (p.dtype) {
        case RZ_F32: warp_emit<C, RZ_F32, false>(p, v, img_out, r, x0, cnt); break;
        case RZ_F16: warp_emit<C, RZ_F16, false>(p, v, img_out, r, x0, cnt); break;
        case RZ_BF16: warp_emit<C, RZ_BF16, false>(p, v, img_out, r, x0, cnt); break;
        default: warp_emit<C, RZ_U8, false>(p, v, img_out, r, x0, cnt); break;
        }
    }
}

// lane t of workgroup (bx, by) of image z: group bx * WARP_BX + t % WARP_BX of row by * WARP_BY + t / WARP_BX
template <int C>
ZJ_HD void warp_lane(const WarpParams& p, const int z, const uint32_t bx, const uint32_t by, const uint32_t t)
{
    warp_lane_c<C>(p, z, (int)(by * WARP_BY + t / WARP_BX), bx * WARP_BX + t % WARP_BX);
}

} // namespace zj
