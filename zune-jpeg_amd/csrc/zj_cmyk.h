// zj_cmyk.h -- a 3-channel u8 image and a u8 plane of the same size combined into an RGB image, out[c] = (a[c] * k + 127) / 255
// (zj_cmyk_to_rgb_device): the last step of a four-component (Adobe CMYK / YCCK) JPEG shown as RGB.
//
// The launch's arguments and one lane's work as ZJ_HD functions, shared by the kernel (zj_cmyk.hip) and its CPU emulation
// (tests/emu_cmyk, a g++ ZJ_EMU build that runs them lane by lane).
//   CmykParams     one launch: up to CMYK_BATCH image pairs of their own sizes, pitches and destinations, an `inverted` bit each
//   cmyk_item      the run a lane owns: CMYK_RUN consecutive pixels of one row (the last run of a row: what is left)
//   cmyk_get       nb bytes of a run into dwords: 16-byte loads, dwords or single bytes, as the address and the length allow;
//                  never a byte outside the run
//   cmyk_mul4      four products at once: byte i of a times byte i of k, divided by 255 and rounded
//   expand_put     (zj_expand.h) the run's bytes stored the same way; never a byte outside the run's own
// A lane reads the whole of its run before it stores any of it, and no other lane touches those bytes: the output may be the
// image `a` itself (same address, same pitch).  No LDS, no lane talks to another.
#pragma once
#include "zj_expand.h" // ExpandV4, expand_rgb, expand_put, ZJ_EXPAND_PUT

namespace zj {

constexpr int CMYK_RUN = 16;     // pixels of one row per lane: 48 + 16 bytes loaded, 48 stored
constexpr int CMYK_NT = 256;     // threads per workgroup
constexpr int CMYK_BATCH = 96;   // image pairs per launch: 40 bytes of kernel arguments each (128 of them would be 5 KB)

struct CmykParams {
    uint64_t a[CMYK_BATCH], k[CMYK_BATCH], out[CMYK_BATCH];
    uint32_t wh[CMYK_BATCH];                                                   // w | h << 16
    uint32_t a_pitch[CMYK_BATCH], k_pitch[CMYK_BATCH], out_pitch[CMYK_BATCH];  // bytes between rows (CHW: of a plane's rows)
    uint32_t inverted[CMYK_BATCH / 32];                                        // bit i: image i's samples are used as stored
    int nimg;
};
static_assert(sizeof(CmykParams) <= 4096, "kernel arguments: 4 KB");

ZJ_HD int cmyk_runs(const int w) { return (w + CMYK_RUN - 1) / CMYK_RUN; }
ZJ_HD int cmyk_grid(const CmykParams& p)
{
    long long most = 1;
    for (int i = 0; i < p.nimg; i++) {
        const long long items = (long long)cmyk_runs((int)(p.wh[i] & 0xffffu)) * (long long)(p.wh[i] >> 16);
        if (items > most) most = items;
    }
    return (int)((most + CMYK_NT - 1) / CMYK_NT);
}

struct CmykItem {
    uint64_t a, k, dst;          // the run's first byte of a (CHW: of plane 0), of k, of the output (CHW: of plane 0)
    uint64_t a_plane, out_plane; // CHW: bytes between the planes
    uint32_t flip;               // 0xffffffff: complement the samples first (the image is not `inverted`), else 0
    int n;                       // pixels of the run, 0: this lane owns nothing
};

// item `id` (workgroup x CMYK_NT + lane) of image img: run id % runs of row id / runs
template <bool CHW>
ZJ_HD CmykItem cmyk_item(const CmykParams& p, const int img, const uint32_t id)
{
    CmykItem it;
    const int w = (int)(p.wh[img] & 0xffffu), h = (int)(p.wh[img] >> 16);
    const uint32_t runs = (uint32_t)cmyk_runs(w);
    it.a = it.k = it.dst = it.a_plane = it.out_plane = 0; it.flip = 0; it.n = 0;
    if (runs == 0) return it;
    const uint32_t row = id / runs, x0 = (id - row * runs) * CMYK_RUN;
    if (row >= (uint32_t)h) return it;
    it.n = w - (int)x0 < CMYK_RUN ? w - (int)x0 : CMYK_RUN;
    it.a = p.a[img] + (uint64_t)row * p.a_pitch[img] + (uint64_t)x0 * (CHW ? 1 : 3);
    it.k = p.k[img] + (uint64_t)row * p.k_pitch[img] + x0;
    it.dst = p.out[img] + (uint64_t)row * p.out_pitch[img] + (uint64_t)x0 * (CHW ? 1 : 3);
    it.a_plane = (uint64_t)p.a_pitch[img] * (uint64_t)h;
    it.out_plane = (uint64_t)p.out_pitch[img] * (uint64_t)h;
    it.flip = (p.inverted[img >> 5] >> (img & 31)) & 1u ? 0u : 0xffffffffu;
    return it;
}

// the first nb bytes at src, byte k in byte k of v (the bytes past nb: 0); ND x 4 the most a run has there
template <int ND>
ZJ_HD void cmyk_get(const uint64_t src, uint32_t (&v)[ND], const int nb)
{
    if (nb == 4 * ND && (src & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < ND / 4; k++) {
            const ExpandV4 q = *ZJ_RZ_GLOBAL(const ExpandV4, src + (uint64_t)(16 * k));
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    } else if ((src & 3u) == 0) {
#pragma unroll
        for (int k = 0; k < ND; k++) v[k] = 4 * k + 4 <= nb ? *ZJ_RZ_GLOBAL(const uint32_t, src + (uint64_t)(4 * k)) : 0u;
#pragma unroll
        for (int k = 0; k < 4 * ND; k++)
            if (k >= (nb & ~3) && k < nb) v[k >> 2] |= (uint32_t)*ZJ_RZ_GLOBAL(const uint8_t, src + (uint64_t)k) << (8 * (k & 3));
    } else {
#pragma unroll
        for (int k = 0; k < ND; k++) v[k] = 0;
#pragma unroll
        for (int k = 0; k < 4 * ND; k++)
            if (k < nb) v[k >> 2] |= (uint32_t)*ZJ_RZ_GLOBAL(const uint8_t, src + (uint64_t)k) << (8 * (k & 3));
    }
}

// the two 16-bit halves of x times those of y, each product kept to 16 bits (v_pk_mul_lo_u16)
typedef uint16_t CmykU16x2 __attribute__((vector_size(4)));
ZJ_HD uint32_t cmyk_mul16x2(const uint32_t x, const uint32_t y)
{
    CmykU16x2 a, b;
    uint32_t r;
    __builtin_memcpy(&a, &x, 4); __builtin_memcpy(&b, &y, 4);
    a = a * b;
    __builtin_memcpy(&r, &a, 4);
    return r;
}

// two bytes in 16-bit halves: (a * k + 127) / 255 of each, as t = a * k + 128, (t + (t >> 8)) >> 8 -- equal for every pair of
// bytes (tests/test_cmyk_emu.py runs all 65 536), and t + (t >> 8) <= 65 407 stays inside its half
ZJ_HD uint32_t cmyk_div255x2(const uint32_t a, const uint32_t k)
{
    const uint32_t t = cmyk_mul16x2(a, k) + 0x00800080u;
    return ((t + ((t >> 8) & 0x00ff00ffu)) >> 8) & 0x00ff00ffu;
}

// byte i of the result: (byte i of a * byte i of k + 127) / 255
ZJ_HD uint32_t cmyk_mul4(const uint32_t a, const uint32_t k)
{
    return cmyk_div255x2(a & 0x00ff00ffu, k & 0x00ff00ffu) | (cmyk_div255x2((a >> 8) & 0x00ff00ffu, (k >> 8) & 0x00ff00ffu) << 8);
}

// One lane's work: its run of a and of k loaded, combined and stored
template <bool CHW>
ZJ_HD void cmyk_lane(const CmykParams& p, const int img, const uint32_t id)
{
    const CmykItem it = cmyk_item<CHW>(p, img, id);
    if (it.n == 0) return;
    uint32_t kk[4];
    cmyk_get<4>(it.k, kk, it.n);
#pragma unroll
    for (int i = 0; i < 4; i++) kk[i] ^= it.flip;
    if (CHW) {
        uint32_t a[3][4];
#pragma unroll
        for (int c = 0; c < 3; c++) cmyk_get<4>(it.a + (uint64_t)c * it.a_plane, a[c], it.n); // (all read before any is stored)
#pragma unroll
        for (int c = 0; c < 3; c++) {
#pragma unroll
            for (int i = 0; i < 4; i++) a[c][i] = cmyk_mul4(a[c][i] ^ it.flip, kk[i]);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) expand_put<4>(it.dst + (uint64_t)c * it.out_plane, a[c], it.n);
    } else {
        uint32_t a[12], k3[12];
        cmyk_get<12>(it.a, a, 3 * it.n);
#pragma unroll
        for (int i = 0; i < 4; i++) expand_rgb(kk[i], k3[3 * i], k3[3 * i + 1], k3[3 * i + 2]);
#pragma unroll
        for (int i = 0; i < 12; i++) a[i] = cmyk_mul4(a[i] ^ it.flip, k3[i]);
        expand_put<12>(it.dst, a, 3 * it.n);
    }
}

} // namespace zj
