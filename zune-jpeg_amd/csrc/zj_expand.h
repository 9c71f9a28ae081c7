// zj_expand.h -- one u8 plane to a 3-channel u8 image with R = G = B (zj_gray_to_rgb_device).
//
// The launch's arguments and one lane's work as ZJ_HD functions, shared by the kernel (zj_expand.hip) and its CPU emulation
// (tests/emu_expand, a g++ ZJ_EMU build that runs them lane by lane).
//   ExpandParams     one launch: up to EXPAND_BATCH planes of their own sizes, pitches and destinations
//   expand_item      the run a lane owns: EXPAND_RUN consecutive pixels of one row (the last run of a row: what is left)
//   expand_load      the run's bytes: one 16-byte load, four dwords or single bytes, as the address allows; never a byte
//                    outside the run
//   expand_store     HWC: the 3n bytes g g g ..., CHW: the n bytes into each of three planes -- 16-byte stores, dwords or
//                    single bytes, as the address and the length allow (resize_store's dispatch, zj_resize.h); never a byte
//                    outside the run's own
// No LDS, no lane talks to another: a wave's lanes own consecutive runs of a row, so its loads and stores are contiguous.
#pragma once
#include "zj_resize.h" // ZJ_HD, ZJ_RZ_GLOBAL

namespace zj {

constexpr int EXPAND_RUN = 16;     // pixels of one row per lane: a 16-byte load, 48 bytes of HWC stores
constexpr int EXPAND_NT = 256;     // threads per workgroup
constexpr int EXPAND_BATCH = 128;  // images per launch (28 bytes of kernel arguments each)

struct ExpandParams {
    uint64_t in[EXPAND_BATCH], out[EXPAND_BATCH];
    uint32_t wh[EXPAND_BATCH];                                // w | h << 16
    uint32_t in_pitch[EXPAND_BATCH], out_pitch[EXPAND_BATCH]; // bytes between rows (CHW output: of a plane's rows)
    int nimg;
};
static_assert(sizeof(ExpandParams) <= 4096, "kernel arguments: 4 KB");

// 16 bytes moved at once
struct alignas(16) ExpandV4 { uint32_t x, y, z, w; };

// a store of the kernel (the emulation counts them in its write map here)
#if !defined(ZJ_EXPAND_PUT)
#define ZJ_EXPAND_PUT(T, addr, v) (*ZJ_RZ_GLOBAL(T, addr) = (v))
#endif

// runs of a row of w pixels, and the launch's grid: the workgroups of the image with the most runs (x), the images (z)
ZJ_HD int expand_runs(const int w) { return (w + EXPAND_RUN - 1) / EXPAND_RUN; }
ZJ_HD int expand_grid(const ExpandParams& p)
{
    long long most = 1;
    for (int i = 0; i < p.nimg; i++) {
        const long long items = (long long)expand_runs((int)(p.wh[i] & 0xffffu)) * (long long)(p.wh[i] >> 16);
        if (items > most) most = items;
    }
    return (int)((most + EXPAND_NT - 1) / EXPAND_NT);
}

struct ExpandItem {
    uint64_t src, dst;   // the run's first input byte / first output byte (CHW: of plane 0)
    uint64_t plane;      // CHW: bytes between the output's planes
    int n;               // pixels of the run, 0: this lane owns nothing
};

// item `id` (workgroup x EXPAND_NT + lane) of image img: run id % runs of row id / runs
template <bool OUT_CHW>
ZJ_HD ExpandItem expand_item(const ExpandParams& p, const int img, const uint32_t id)
{
    ExpandItem it;
    const int w = (int)(p.wh[img] & 0xffffu), h = (int)(p.wh[img] >> 16);
    const uint32_t runs = (uint32_t)expand_runs(w);
    it.src = it.dst = it.plane = 0; it.n = 0;
    if (runs == 0) return it;
    const uint32_t row = id / runs, x0 = (id - row * runs) * EXPAND_RUN;
    if (row >= (uint32_t)h) return it;
    it.n = w - (int)x0 < EXPAND_RUN ? w - (int)x0 : EXPAND_RUN;
    it.src = p.in[img] + (uint64_t)row * p.in_pitch[img] + x0;
    it.dst = p.out[img] + (uint64_t)row * p.out_pitch[img] + (uint64_t)x0 * (OUT_CHW ? 1 : 3);
    it.plane = (uint64_t)p.out_pitch[img] * (uint64_t)h;
    return it;
}

// the run's pixels, pixel k in byte k of g (the bytes past n: 0)
ZJ_HD void expand_load(const ExpandItem& it, uint32_t (&g)[4])
{
    if (it.n == EXPAND_RUN && (it.src & 15u) == 0) {
        const ExpandV4 v = *ZJ_RZ_GLOBAL(const ExpandV4, it.src);
        g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
    } else if (it.n == EXPAND_RUN && (it.src & 3u) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = *ZJ_RZ_GLOBAL(const uint32_t, it.src + (uint64_t)(4 * k));
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = 0;
#pragma unroll
        for (int k = 0; k < EXPAND_RUN; k++)
            if (k < it.n) g[k >> 2] |= (uint32_t)*ZJ_RZ_GLOBAL(const uint8_t, it.src + (uint64_t)k) << (8 * (k & 3));
    }
}

// byte i of the result is byte (sel >> 8i & 3) of s: v_perm_b32 with both sources s
ZJ_HD uint32_t expand_perm(const uint32_t s, const uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(s, s, sel);
#else
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) r |= ((s >> (8 * ((sel >> (8 * i)) & 3u))) & 255u) << (8 * i);
    return r;
#endif
}

// the interleaved form of the 4 pixels b0 b1 b2 b3 of s: b0 b0 b0 b1 | b1 b1 b2 b2 | b2 b3 b3 b3
ZJ_HD void expand_rgb(const uint32_t s, uint32_t& d0, uint32_t& d1, uint32_t& d2)
{
    d0 = expand_perm(s, 0x01000000u); d1 = expand_perm(s, 0x02020101u); d2 = expand_perm(s, 0x03030302u);
}

// the first nb bytes of the ND dwords of v to dst, ND x 4 the most a run has there
template <int ND>
ZJ_HD void expand_put(const uint64_t dst, const uint32_t (&v)[ND], const int nb)
{
    if (nb == 4 * ND && (dst & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < ND / 4; k++) ZJ_EXPAND_PUT(ExpandV4, dst + (uint64_t)(16 * k), (ExpandV4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]}));
    } else if ((dst & 3u) == 0) {
#pragma unroll
        for (int k = 0; k < ND; k++)
            if (4 * k + 4 <= nb) ZJ_EXPAND_PUT(uint32_t, dst + (uint64_t)(4 * k), v[k]);
#pragma unroll
        for (int k = 0; k < 4 * ND; k++)
            if (k >= (nb & ~3) && k < nb) ZJ_EXPAND_PUT(uint8_t, dst + (uint64_t)k, (uint8_t)(v[k >> 2] >> (8 * (k & 3))));
    } else {
#pragma unroll
        for (int k = 0; k < 4 * ND; k++)
            if (k < nb) ZJ_EXPAND_PUT(uint8_t, dst + (uint64_t)k, (uint8_t)(v[k >> 2] >> (8 * (k & 3))));
    }
}

// One lane's work: its run loaded, expanded and stored
template <bool OUT_CHW>
ZJ_HD void expand_lane(const ExpandParams& p, const int img, const uint32_t id)
{
    const ExpandItem it = expand_item<OUT_CHW>(p, img, id);
    if (it.n == 0) return;
    uint32_t g[4];
    expand_load(it, g);
    if (OUT_CHW) {
#pragma unroll
        for (int c = 0; c < 3; c++) expand_put<4>(it.dst + (uint64_t)c * it.plane, g, it.n);
    } else {
        uint32_t d[12];
#pragma unroll
        for (int k = 0; k < 4; k++) expand_rgb(g[k], d[3 * k], d[3 * k + 1], d[3 * k + 2]);
        expand_put<12>(it.dst, d, 3 * it.n);
    }
}

} // namespace zj
