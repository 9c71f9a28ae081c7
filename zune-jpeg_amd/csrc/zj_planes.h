// zj_planes.h -- three u8 component planes, each at its own resolution, combined into one RGB image
// (zj_planes_to_rgb_device): the last step of a three-component JPEG whose sampling the fused kernels do
// not know (4:1:1, 4:1:0, chroma that is not (1,1) ...) or whose samples are stored RGB.
//
// The launch's arguments and one lane's work as ZJ_HD functions, shared by the kernel (zj_planes.hip) and its CPU emulation
// (tests/emu_planes, a g++ ZJ_EMU build that runs them lane by lane).
//   PlanesParams   one launch: up to PLANES_BATCH images of their own sizes, ratios, phases, pitches and destinations
//   planes_item    the run a lane owns: PLANES_RUN consecutive pixels of one row (the last run of a row: what is left)
//   planes_get     nb bytes of a plane's row into dwords: one 16-byte load, dwords or single bytes, as the address and the
//                  length allow; never a byte outside the samples the run shows
//   planes_fetch   a component's samples replicated to the run's 16 pixels: output pixel j shows sample (j + phase) / ratio
//                  (box replication, integer division), by byte permutes
//   planes_colour  four pixels at once: the full decode's YCbCr -> RGB arithmetic on packed 16-bit halves
//   expand_put     (zj_expand.h) the run's bytes stored; never a byte outside the run's own
// No LDS, no scratch, no lane talks to another.
#pragma once
#include "zj_expand.h" // ExpandV4, expand_put, ZJ_EXPAND_PUT

namespace zj {

constexpr int PLANES_RUN = 16;    // pixels of one row per lane: 16 / 8 (+1) / 4 (+1) bytes loaded per component, 48 stored
constexpr int PLANES_NT = 256;    // threads per workgroup
constexpr int PLANES_BATCH = 72;  // images per launch: 56 bytes of kernel arguments each

struct PlanesParams {
    uint64_t p[3][PLANES_BATCH], out[PLANES_BATCH];
    uint32_t pitch[3][PLANES_BATCH], out_pitch[PLANES_BATCH]; // bytes between rows (CHW output: of a plane's rows)
    uint32_t wh[PLANES_BATCH];                                // w | h << 16 of the output
    uint32_t geo[PLANES_BATCH];                               // component c in bits 8c .. 8c + 7: planes_geo
    int nimg;
};
static_assert(sizeof(PlanesParams) <= 4096, "kernel arguments: 4 KB");

// a component's place in an image: log2 of its ratios (0..2) and the phases x mod rx, y mod ry of the image's first pixel
ZJ_HD uint32_t planes_geo(const int lrx, const int lry, const int px, const int py)
{
    return (uint32_t)(lrx | (lry << 2) | (px << 4) | (py << 6));
}

ZJ_HD int planes_runs(const int w) { return (w + PLANES_RUN - 1) / PLANES_RUN; }
ZJ_HD int planes_grid(const PlanesParams& p)
{
    long long most = 1;
    for (int i = 0; i < p.nimg; i++) {
        const long long items = (long long)planes_runs((int)(p.wh[i] & 0xffffu)) * (long long)(p.wh[i] >> 16);
        if (items > most) most = items;
    }
    return (int)((most + PLANES_NT - 1) / PLANES_NT);
}

struct PlanesItem {
    uint64_t src[3];    // the first sample the run shows, per component
    uint64_t dst;       // the run's first output byte (CHW: of plane 0)
    uint64_t out_plane; // CHW: bytes between the output's planes
    uint32_t geo;
    int n;              // pixels of the run, 0: this lane owns nothing
};

// item `id` (workgroup x PLANES_NT + lane) of image img: run id % runs of row id / runs.  A run starts at a multiple of 16
// pixels, so the phase never carries into its first sample's column: (x0 + px) >> lrx == x0 >> lrx.
template <bool CHW>
ZJ_HD PlanesItem planes_item(const PlanesParams& p, const int img, const uint32_t id)
{
    PlanesItem it;
    const int w = (int)(p.wh[img] & 0xffffu), h = (int)(p.wh[img] >> 16);
    const uint32_t runs = (uint32_t)planes_runs(w);
    it.src[0] = it.src[1] = it.src[2] = it.dst = it.out_plane = 0; it.geo = 0; it.n = 0;
    if (runs == 0) return it;
    const uint32_t row = id / runs, x0 = (id - row * runs) * PLANES_RUN;
    if (row >= (uint32_t)h) return it;
    it.n = w - (int)x0 < PLANES_RUN ? w - (int)x0 : PLANES_RUN;
    it.geo = p.geo[img];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t g = it.geo >> (8 * c);
        const uint32_t lrx = g & 3u, lry = (g >> 2) & 3u, py = (g >> 6) & 3u;
        it.src[c] = p.p[c][img] + (uint64_t)((row + py) >> lry) * p.pitch[c][img] + (x0 >> lrx);
    }
    it.dst = p.out[img] + (uint64_t)row * p.out_pitch[img] + (uint64_t)x0 * (CHW ? 1 : 3);
    it.out_plane = (uint64_t)p.out_pitch[img] * (uint64_t)h;
    return it;
}

// the first nb bytes at src, byte k in byte k of v (the bytes past nb: 0); nb <= 4 x ND
template <int ND>
ZJ_HD void planes_get(const uint64_t src, uint32_t (&v)[ND], const int nb)
{
    if constexpr (ND == 4) {
        if (nb == 16 && (src & 15u) == 0) {
            const ExpandV4 q = *ZJ_RZ_GLOBAL(const ExpandV4, src);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            return;
        }
    }
    if ((src & 3u) == 0) {
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

// byte i of the result is byte (sel >> 8i & 7) of the eight bytes hi:lo (0..3: lo, 4..7: hi): v_perm_b32
ZJ_HD uint32_t planes_perm(const uint32_t hi, const uint32_t lo, const uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t s = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) r |= (uint32_t)((s >> (8 * ((sel >> (8 * i)) & 7u))) & 255u) << (8 * i);
    return r;
#endif
}

// a component's samples for the n pixels of a run, pixel j in byte j of o: sample (j + px) >> lrx of the row at src.
// Ratio 1: the n bytes themselves.  Ratio 2: ((n - 1 + px) >> 1) + 1 <= 9 bytes; the pixels 4q .. 4q + 3 show the bytes
// 2q .. 2q + 2.  Ratio 4: ((n - 1 + px) >> 2) + 1 <= 5 bytes; the pixels 4q .. 4q + 3 show the bytes q and q + 1.
ZJ_HD void planes_fetch(const uint64_t src, const uint32_t lrx, const uint32_t px, const int n, uint32_t (&o)[4])
{
    if (lrx == 0) {
        planes_get<4>(src, o, n);
    } else if (lrx == 1) {
        uint32_t v[3];
        planes_get<3>(src, v, ((n - 1 + (int)px) >> 1) + 1);
        const uint32_t sel = px ? 0x02010100u : 0x01010000u; // (j + px) >> 1 for j = 0..3
        o[0] = planes_perm(v[1], v[0], sel);
        o[1] = planes_perm(v[1], v[0], sel + 0x02020202u);
        o[2] = planes_perm(v[2], v[1], sel);
        o[3] = planes_perm(v[2], v[1], sel + 0x02020202u);
    } else {
        uint32_t v[2];
        planes_get<2>(src, v, ((n - 1 + (int)px) >> 2) + 1);
        const uint32_t sel = px == 0 ? 0u : px == 1 ? 0x01000000u : px == 2 ? 0x01010000u : 0x01010100u; // (j + px) >> 2
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = planes_perm(v[1], v[0], sel + 0x01010101u * (uint32_t)q);
    }
}

// two signed 16-bit halves in a dword
typedef int16_t PlanesI16x2 __attribute__((vector_size(4)));
ZJ_HD PlanesI16x2 planes_pk(const uint32_t x) { PlanesI16x2 r; __builtin_memcpy(&r, &x, 4); return r; }
ZJ_HD uint32_t planes_unpk(const PlanesI16x2 x) { uint32_t r; __builtin_memcpy(&r, &x, 4); return r; }
ZJ_HD PlanesI16x2 planes_splat(const int v) { return PlanesI16x2{(int16_t)v, (int16_t)v}; }
// both halves clamped to 0..255
ZJ_HD PlanesI16x2 planes_clamp(const PlanesI16x2 x)
{
#if defined(__clang__)
    return __builtin_elementwise_min(__builtin_elementwise_max(x, planes_splat(0)), planes_splat(255));
#else
    PlanesI16x2 r;
    for (int i = 0; i < 2; i++) r[i] = x[i] < 0 ? (int16_t)0 : x[i] > 255 ? (int16_t)255 : x[i];
    return r;
#endif
}

// two pixels, their y, cb, cr in the 16-bit halves: the full decode's per-pixel arithmetic (zj_device.h; the oracle's
// ycbcr_to_rgb_px).  With bytes going in no product leaves 16 bits: |113 * (cb - 128)| <= 14 464.
ZJ_HD void planes_colour2(const uint32_t y, const uint32_t cb, const uint32_t cr, uint32_t& r, uint32_t& g, uint32_t& b)
{
    const PlanesI16x2 yy = planes_pk(y), u = planes_pk(cb) - planes_splat(128), v = planes_pk(cr) - planes_splat(128);
    r = planes_unpk(planes_clamp(yy + ((planes_splat(45) * v) >> 5)));
    g = planes_unpk(planes_clamp(yy - ((planes_splat(11) * u + planes_splat(23) * v) >> 5)));
    b = planes_unpk(planes_clamp(yy + ((planes_splat(113) * u) >> 6)));
}

// four pixels, pixel j in byte j of y, cb, cr and of r, g, b
ZJ_HD void planes_colour(const uint32_t y, const uint32_t cb, const uint32_t cr, uint32_t& r, uint32_t& g, uint32_t& b)
{
    const uint32_t m = 0x00ff00ffu;
    uint32_t r0, g0, b0, r1, g1, b1;
    planes_colour2(y & m, cb & m, cr & m, r0, g0, b0);
    planes_colour2((y >> 8) & m, (cb >> 8) & m, (cr >> 8) & m, r1, g1, b1);
    r = r0 | (r1 << 8); g = g0 | (g1 << 8); b = b0 | (b1 << 8);
}

// the interleaved form of four pixels: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
ZJ_HD void planes_weave(const uint32_t r, const uint32_t g, const uint32_t b, uint32_t& d0, uint32_t& d1, uint32_t& d2)
{
    d0 = planes_perm(b, planes_perm(g, r, 0x01000400u), 0x03040100u);
    d1 = planes_perm(b, planes_perm(g, r, 0x06020005u), 0x03020500u);
    d2 = planes_perm(b, planes_perm(g, r, 0x00070300u), 0x07020106u);
}

// One lane's work: its run's samples of the three components loaded, replicated, converted and stored
template <bool CHW, bool STORED_RGB>
ZJ_HD void planes_lane(const PlanesParams& p, const int img, const uint32_t id)
{
    const PlanesItem it = planes_item<CHW>(p, img, id);
    if (it.n == 0) return;
    uint32_t s[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t g = it.geo >> (8 * c);
        planes_fetch(it.src[c], g & 3u, (g >> 4) & 3u, it.n, s[c]);
    }
    if (!STORED_RGB) {
#pragma unroll
        for (int i = 0; i < 4; i++) planes_colour(s[0][i], s[1][i], s[2][i], s[0][i], s[1][i], s[2][i]);
    }
    if (CHW) {
#pragma unroll
        for (int c = 0; c < 3; c++) expand_put<4>(it.dst + (uint64_t)c * it.out_plane, s[c], it.n);
    } else {
        uint32_t d[12];
#pragma unroll
        for (int i = 0; i < 4; i++) planes_weave(s[0][i], s[1][i], s[2][i], d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        expand_put<12>(it.dst, d, 3 * it.n);
    }
}

} // namespace zj
