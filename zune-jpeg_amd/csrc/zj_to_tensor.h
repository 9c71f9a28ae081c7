// zj_to_tensor.h -- u8 images in HBM to one normalised tensor, not resized (zj_to_tensor_device).
//
// The launch's arguments and one lane's work as ZJ_HD functions, shared by the kernel (zj_to_tensor.hip) and its CPU emulation
// (tests/emu_to_tensor, a g++ ZJ_EMU build that runs them lane by lane, with a write map and a check of every load).
//   ToTensorParams   one launch: up to TT_BATCH images of ONE size, their own bases and pitches, into consecutive images of
//                    the tensor
//   tt_lane          the item a lane owns: one block of TT_RUN elements, aligned in the DESTINATION, of one run of contiguous
//                    tensor elements (NHWC: a row's C * w, NCHW: a row of one channel plane); the elements in front of a
//                    run's first aligned block and behind its last go out one by one
//   tt_load8         the 8 source bytes of a block whose bytes lie side by side in the source, as whole dwords of the row
//                    shifted into place; single bytes where a dword would leave the row
//   tt_run           the block's bytes converted (zj_resize.h: resize_f32, resize_pack2) and stored
// The conversion is crop_tensor_run's (zj_crop_tensor.h): the value of the byte p is resize_*(p << 16).  No LDS, no lane
// talks to another.  dtype, layout, flip and the channel counts are switches that are uniform over a workgroup.
#pragma once
#include "zj_resize.h" // ZJ_HD, ZJ_RZ_GLOBAL, the conversions, resize_elem

namespace zj {

constexpr int TT_RUN = 8;      // elements of one lane's block: 16 bytes of a 16-bit type, 32 of float32, 8 of u8
constexpr int TT_NT = 256;     // threads per workgroup
constexpr int TT_BATCH = 128;  // images per launch (12 bytes of kernel arguments each)

struct ToTensorParams {
    uint64_t in[TT_BATCH];          // per image: its first byte
    uint32_t pitch[TT_BATCH];       // per image: bytes between rows
    uint32_t flip[TT_BATCH / 32];   // per image: a bit, its columns mirrored
    uint64_t out;                   // the launch's first image of the tensor
    float scale[3], bias[3];        // per channel: s_c = scale_c * 2^-16, bias_c (zj_resize.h: ResizeParams)
    int w, h, nimg;
    int cin, cout;                  // channels of the images (interleaved) and of the tensor: 1 -> 1, 1 -> 3, 3 -> 3
    int dtype;                      // ZJ_DTYPE_*
    int nhwc;                       // 1: [h, w, C], 0: [C, h, w]
};
static_assert(sizeof(ToTensorParams) <= 4096, "kernel arguments: 4 KB");

struct alignas(16) ToTensorV4 { uint32_t x, y, z, w; };
struct alignas(8) ToTensorV2 { uint32_t x, y; };

// a store and a load of the kernel (the emulation counts the stores in its write map and checks the loads here)
#if !defined(ZJ_TT_PUT)
#define ZJ_TT_PUT(T, addr, v) (*ZJ_RZ_GLOBAL(T, addr) = (v))
#endif
#if !defined(ZJ_TT_GET)
#define ZJ_TT_GET(T, addr) (*ZJ_RZ_GLOBAL(const T, addr))
#endif

// one channel: the two layouts are one; a row is then one run of cout * w elements, else cout runs of w
ZJ_HD bool tt_rows_whole(const ToTensorParams& p) { return p.cout == 1 || p.nhwc != 0; }
// the aligned blocks a run of n elements touches, at most: its first element may be a block's last
ZJ_HD uint32_t tt_blocks(const uint32_t n) { return (n + TT_RUN - 1) / TT_RUN + 1; }
// items (run, block) of an image row
ZJ_HD uint32_t tt_row_items(const ToTensorParams& p)
{
    return tt_rows_whole(p) ? tt_blocks((uint32_t)(p.cout * p.w)) : (uint32_t)p.cout * tt_blocks((uint32_t)p.w);
}
// the launch's grid: the workgroups of one image (x), the images (z); every image of a launch has the same items
ZJ_HD uint32_t tt_grid(const ToTensorParams& p)
{
    const uint64_t items = (uint64_t)tt_row_items(p) * (uint64_t)p.h;
    return (uint32_t)((items + TT_NT - 1) / TT_NT);
}

// channel c's factor of three, c a per-lane value (crop_tensor_pick's reason: a select between values)
ZJ_HD float tt_pick(const float v0, const float v1, const float v2, const int c) { return c == 0 ? v0 : (c == 1 ? v1 : v2); }

// the dword at a (a multiple of 4), of which only the bytes inside [lo, hi) are read (the others: 0)
ZJ_HD uint32_t tt_dword(const uint64_t a, const uint64_t lo, const uint64_t hi)
{
    if (a >= lo && a + 4 <= hi) return ZJ_TT_GET(uint32_t, a);
    uint32_t d = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (a + b >= lo && a + b < hi) d |= (uint32_t)ZJ_TT_GET(uint8_t, a + b) << (8 * b);
    return d;
}

// bytes [pos, pos + 8) of the row of rb bytes at srow (pos < rb), byte k in px[k]; what lies behind the row's end: 0
ZJ_HD void tt_load8(const uint64_t srow, const int rb, const int pos, uint32_t (&px)[TT_RUN])
{
    const uint64_t s = srow + (uint64_t)pos, a = s & ~(uint64_t)3, hi = srow + (uint64_t)rb;
    const int sh = 8 * (int)(s & 3u);
    const uint32_t d0 = tt_dword(a, srow, hi);
    const uint32_t d1 = a + 4 < hi ? tt_dword(a + 4, srow, hi) : 0u;
    const uint32_t d2 = sh != 0 && a + 8 < hi ? tt_dword(a + 8, srow, hi) : 0u;
    const uint32_t q0 = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh), q1 = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
#pragma unroll
    for (int k = 0; k < 4; k++) { px[k] = (q0 >> (8 * k)) & 255u; px[4 + k] = (q1 >> (8 * k)) & 255u; }
}

// One lane's block: cnt (1..8) consecutive DESTINATION elements of one run, the first at dst.  pos: the first element's
// place in its run -- whole rows: element index (column * CO + channel), else the column of channel plane cf.  srow: the
// image row's first byte.  Element k is the conversion of the byte of source pixel (flip ? w - 1 - column : column),
// channel c (a one-channel source: its one byte).  What depends on the lane -- the first element's channel -- is settled
// once, as the factors of the channels in the block's own order; element k takes entry k % CO, a compile-time index.
// A full block (cnt == 8) starts on a boundary of its own size in the destination and goes out with the widest stores, a
// shorter one element by element.  No byte outside the row's w * CI is read, none outside the cnt elements is written.
template <int CI, int CO>
ZJ_HD void tt_run(const ToTensorParams& p, const bool whole, const bool flip, const uint64_t srow, const uint64_t dst, const int cnt,
                  const int pos, const int cf)
{
    constexpr int G = TT_RUN;
    const int w = p.w;
    const int c0 = whole ? pos % CO : cf;
    float sr[CO], br[CO];
    int ch[CO];
#pragma unroll
    for (int j = 0; j < CO; j++) {
        int c = whole ? c0 + j : cf;
        c -= c >= CO ? CO : 0;
        ch[j] = c;
        sr[j] = tt_pick(p.scale[0], p.scale[1], p.scale[2], c);
        br[j] = tt_pick(p.bias[0], p.bias[1], p.bias[2], c);
    }
    uint32_t px[G];
    if (!flip && (whole ? CI == CO : CI == 1)) {
        tt_load8(srow, w * CI, pos, px); // the block's bytes lie side by side
    } else {
        int at[G];
#pragma unroll
        for (int k = 0; k < G; k++) {
            if (whole && CI == CO) at[k] = CO * (w - 1) - (pos + k) + 2 * ch[k % CO]; // (mirrored: the case above took the other)
            else if (whole) { const int col = (int)((uint32_t)(pos + k) / (uint32_t)CO); at[k] = flip ? w - 1 - col : col; }
            else at[k] = (flip ? w - 1 - (pos + k) : pos + k) * CI + (CI == 3 ? cf : 0);
        }
#pragma unroll
        for (int k = 0; k < G; k++) px[k] = ZJ_TT_GET(uint8_t, srow + (uint64_t)(k < cnt ? at[k] : at[0])); // (past the block: its first byte again)
    }
    float f[G];
#pragma unroll
    for (int k = 0; k < G; k++) f[k] = resize_f32(px[k] << 16, sr[k % CO], br[k % CO]);
    if (p.dtype == RZ_F32) {
        uint32_t wd[G];
#pragma unroll
        for (int k = 0; k < G; k++) wd[k] = f32_bits(f[k]);
        if (cnt == G) {
            ZJ_TT_PUT(ToTensorV4, dst, (ToTensorV4{wd[0], wd[1], wd[2], wd[3]}));
            ZJ_TT_PUT(ToTensorV4, dst + 16, (ToTensorV4{wd[4], wd[5], wd[6], wd[7]}));
        } else {
#pragma unroll
            for (int k = 0; k < G; k++)
                if (k < cnt) ZJ_TT_PUT(uint32_t, dst + (uint64_t)(4 * k), wd[k]);
        }
    } else if (p.dtype == RZ_U8) {
        if (cnt == G) {
            ZJ_TT_PUT(ToTensorV2, dst, (ToTensorV2{px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24, px[4] | px[5] << 8 | px[6] << 16 | px[7] << 24}));
        } else {
#pragma unroll
            for (int k = 0; k < G; k++)
                if (k < cnt) ZJ_TT_PUT(uint8_t, dst + (uint64_t)k, (uint8_t)px[k]);
        }
    } else {
        uint32_t wd[G / 2];
#pragma unroll
        for (int k = 0; k < G / 2; k++)
            wd[k] = p.dtype == RZ_BF16 ? resize_pack2<RZ_BF16>(f[2 * k], f[2 * k + 1]) : resize_pack2<RZ_F16>(f[2 * k], f[2 * k + 1]);
        if (cnt == G) {
            ZJ_TT_PUT(ToTensorV4, dst, (ToTensorV4{wd[0], wd[1], wd[2], wd[3]}));
        } else {
#pragma unroll
            for (int k = 0; k < G; k++)
                if (k < cnt) ZJ_TT_PUT(uint16_t, dst + (uint64_t)(2 * k), (uint16_t)(wd[k >> 1] >> (16 * (k & 1))));
        }
    }
}

// item `id` (workgroup x TT_NT + lane) of image img: block id % blocks of run (id / blocks) % runs of row id / (runs x blocks)
template <int CI, int CO>
ZJ_HD void tt_lane_c(const ToTensorParams& p, const int img, const uint32_t id)
{
    constexpr int G = TT_RUN;
    const int w = p.w, h = p.h;
    const bool whole = tt_rows_whole(p);
    const bool flip = ((p.flip[img >> 5] >> (img & 31)) & 1u) != 0;
    const int E = resize_elem_bytes(p.dtype);
    const uint32_t n = whole ? (uint32_t)(CO * w) : (uint32_t)w; // elements of a run
    const uint32_t nblk = tt_blocks(n), per = (whole ? 1u : (uint32_t)CO) * nblk;
    const uint32_t row = id / per;
    if (row >= (uint32_t)h) return;
    const uint32_t q = id - row * per, run = q / nblk, bq = q - run * nblk;
    // the run's first element, counted from the launch's first image
    const long long e0 = (long long)img * CO * w * h
                         + (whole ? resize_elem<CO, true>(0, (int)row, 0, w, h) : resize_elem<CO, false>((int)run, (int)row, 0, w, h));
    const uint64_t a0 = p.out + (uint64_t)e0 * (uint64_t)E;
    // elements of the run's first aligned block that lie in front of the run
    const int lead = (int)(a0 & (uint64_t)(G * E - 1)) / E;
    int k0 = G * (int)bq - lead, k1 = k0 + G;
    if (k0 < 0) k0 = 0;
    if (k1 > (int)n) k1 = (int)n;
    if (k0 >= k1) return;
    tt_run<CI, CO>(p, whole, flip, p.in[img] + (uint64_t)row * p.pitch[img], a0 + (uint64_t)k0 * (uint64_t)E, k1 - k0, k0, (int)run);
}

// One lane's work
ZJ_HD void tt_lane(const ToTensorParams& p, const int img, const uint32_t id)
{
    if (p.cin == 3) tt_lane_c<3, 3>(p, img, id);
    else if (p.cout == 3) tt_lane_c<1, 3>(p, img, id);
    else tt_lane_c<1, 1>(p, img, id);
}

} // namespace zj
