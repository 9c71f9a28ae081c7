// zj_tone.h -- per-image tone curves of u8 images (zj_tone_device): invert, posterize, solarize, autocontrast
// and equalize, byte for byte Pillow's ImageOps, as three device stages:
//   histogram   (zj_histogram_device)  uint32 hist[image][channel][256], counted through LDS atomics, summed across workgroups
//   table build (zj_tone_luts_device)  uint8 lut[image][channel][256] from an op and, for autocontrast and equalize, the histogram
//   lookup      (zj_lut_device)        out[c] = lut[image][c][in[c]]
// The launches' arguments and the phases of one workgroup as ZJ_HD functions, split at the barriers, shared by the kernels
// (zj_tone.hip) and their CPU emulation (tests/emu_tone, a g++ ZJ_EMU build that runs them lane by lane).
//   HistParams / hist_zero_phase, hist_count_phase, hist_flush_phase
//   ToneLutParams / tone_lut_load_phase, tone_lut_reduce_phase, tone_lut_scan_phase, tone_lut_entry_phase
//   LutParams / lut_table_phase, lut_map_phase
//   cmyk_get       (zj_cmyk.h) nb bytes of a run into dwords, never a byte outside the run
//   expand_put     (zj_expand.h) the run's bytes stored the same way; never a byte outside the run's own
// The only ordering between the three kernels is the kernel boundary on the stream: no flags, no spinning.
#pragma once
#include "zj_cmyk.h" // cmyk_get; zj_expand.h: expand_put
#include "zj_tone_ops.h" // TONE_*, tone_op_valid, tone_needs_hist: the host side

namespace zj {

constexpr int TONE_RUN = 16;  // pixels of one row per lane and step
constexpr int TONE_NT = 256;  // threads per workgroup, of all three kernels: lane i of the table build owns entry i

// the accesses the emulation replaces: an add to a workgroup counter in LDS and to a table entry in device memory (both
// without a returned value), a read of a table, a store of a table entry
#if defined(ZJ_EMU)
#if !defined(ZJ_TONE_GLOBAL_ADD)
#define ZJ_TONE_GLOBAL_ADD(addr, v) (*reinterpret_cast<uint32_t*>((uintptr_t)(addr)) += (v))
#endif
#define ZJ_TONE_LDS_ADD(p, v) (*(p) += (v))
#define ZJ_TONE_LDS_MIN(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define ZJ_TONE_LDS_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#else
#define ZJ_TONE_GLOBAL_ADD(addr, v) ((void)__hip_atomic_fetch_add(ZJ_RZ_GLOBAL(uint32_t, addr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
#define ZJ_TONE_LDS_ADD(p, v) ((void)__hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define ZJ_TONE_LDS_MIN(p, v) ((void)__hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define ZJ_TONE_LDS_MAX(p, v) ((void)__hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#endif
#if !defined(ZJ_TONE_TABLE)
#define ZJ_TONE_TABLE(T, addr) (*ZJ_RZ_GLOBAL(const T, addr))
#endif
#if !defined(ZJ_TONE_TABLE_PUT)
#define ZJ_TONE_TABLE_PUT(addr, v) (*ZJ_RZ_GLOBAL(uint8_t, addr) = (v))
#endif

// byte k of the dwords v
template <int ND>
ZJ_HD uint32_t tone_byte(const uint32_t (&v)[ND], const int k) { return (v[k >> 2] >> (8 * (k & 3))) & 255u; }

/* ---- the histogram ------------------------------------------------------------------------------------------------- */
constexpr int HIST_RUNS = 8;                    // runs a lane takes before the workgroup's counters are flushed
constexpr int HIST_ITEMS = TONE_NT * HIST_RUNS; // runs of one workgroup: 32768 pixels
constexpr int HIST_BATCH = 128;                 // images per launch: 24 bytes of kernel arguments each

struct HistParams {
    uint64_t in[HIST_BATCH], hist[HIST_BATCH]; // the image; its table, uint32 [channels][256], zero before the launch
    uint32_t wh[HIST_BATCH];                   // w | h << 16
    uint32_t pitch[HIST_BATCH];                // bytes between rows (CHW: of a plane's rows)
    int nimg;
};
static_assert(sizeof(HistParams) <= 4096, "kernel arguments: 4 KB");

// the runs of image i, row by row: at most 4096 x 65535 < 2^32
ZJ_HD uint32_t tone_items(const uint32_t wh) { return (uint32_t)cmyk_runs((int)(wh & 0xffffu)) * (wh >> 16); }
ZJ_HD int hist_grid(const HistParams& p)
{
    uint32_t most = 1;
    for (int i = 0; i < p.nimg; i++)
        if (tone_items(p.wh[i]) > most) most = tone_items(p.wh[i]);
    return (int)((most + HIST_ITEMS - 1) / HIST_ITEMS);
}
// workgroup wg has runs of image img (the grid is the largest image's; the same over the workgroup)
ZJ_HD bool hist_block_active(const HistParams& p, const int img, const uint32_t wg)
{
    return (uint64_t)wg * HIST_ITEMS < (uint64_t)tone_items(p.wh[img]);
}

// the workgroup's counters, C x 256 of 32 bits: a workgroup counts at most HIST_ITEMS x TONE_RUN = 2^15 pixels, so one bin of
// one channel holds at most 2^15 -- a flat image puts all of them into one
template <int C>
ZJ_HD void hist_zero_phase(uint32_t* lds, const int tid)
{
    for (int i = tid; i < C * 256; i += TONE_NT) lds[i] = 0;
}

// The n values of one channel of a run -- byte first + STRIDE i of the dwords a, i < n, n >= 1 -- into that channel's 256
// counters.  MERGE: a stretch of equal neighbours is ONE add of its length, so a lane's run of one value costs one LDS atomic
// in place of 16 (flat regions: sky, borders); without it every byte is an add of 1.  The sums are the same.
template <int ND, int STRIDE, bool MERGE>
ZJ_HD void hist_add(uint32_t* bins, const uint32_t (&a)[ND], const int first, const int n)
{
    if (!MERGE) {
#pragma unroll
        for (int i = 0; i < TONE_RUN; i++)
            if (i < n) ZJ_TONE_LDS_ADD(bins + tone_byte<ND>(a, first + STRIDE * i), 1u);
        return;
    }
    uint32_t prev = tone_byte<ND>(a, first), count = 1;
#pragma unroll
    for (int i = 1; i < TONE_RUN; i++) {
        const uint32_t b = tone_byte<ND>(a, first + STRIDE * i);
        if (i < n && b != prev) {
            ZJ_TONE_LDS_ADD(bins + prev, count);
            prev = b; count = 0;
        }
        count += i < n ? 1u : 0u;
    }
    ZJ_TONE_LDS_ADD(bins + prev, count);
}

constexpr bool HIST_MERGE = true; // (the A/B of both ways: lab/zj_hist_ab.hip, profiles/tone.txt)

// HIST_RUNS runs per lane, run r of the workgroup's step s at item wg x HIST_ITEMS + s x TONE_NT + lane: a wave's lanes own
// consecutive runs of a row.  Only the run's own bytes are loaded and counted: no padding, no byte of the next row.
template <int C, bool CHW, bool MERGE = HIST_MERGE>
ZJ_HD void hist_count_phase(const HistParams& p, const int img, const uint32_t wg, const int tid, uint32_t* lds)
{
    const int w = (int)(p.wh[img] & 0xffffu), h = (int)(p.wh[img] >> 16);
    const uint32_t runs = (uint32_t)cmyk_runs(w), total = runs * (uint32_t)h;
    const uint64_t plane = (uint64_t)p.pitch[img] * (uint64_t)h;
    for (int s = 0; s < HIST_RUNS; s++) {
        const uint32_t id = wg * (uint32_t)HIST_ITEMS + (uint32_t)(s * TONE_NT + tid);
        if (id >= total) break;
        const uint32_t row = id / runs, x0 = (id - row * runs) * TONE_RUN;
        const int n = w - (int)x0 < TONE_RUN ? w - (int)x0 : TONE_RUN;
        if (C == 3 && !CHW) {
            uint32_t a[12];
            cmyk_get<12>(p.in[img] + (uint64_t)row * p.pitch[img] + (uint64_t)x0 * 3, a, 3 * n);
#pragma unroll
            for (int c = 0; c < 3; c++) hist_add<12, 3, MERGE>(lds + c * 256, a, c, n);
        } else {
#pragma unroll
            for (int c = 0; c < C; c++) {
                uint32_t a[4];
                cmyk_get<4>(p.in[img] + (uint64_t)c * plane + (uint64_t)row * p.pitch[img] + x0, a, n);
                hist_add<4, 1, MERGE>(lds + c * 256, a, 0, n);
            }
        }
    }
}

// the workgroup's non-empty counters added to the image's table: integer sums, the same whatever the order of arrival
template <int C>
ZJ_HD void hist_flush_phase(const HistParams& p, const int img, const int tid, const uint32_t* lds)
{
    for (int i = tid; i < C * 256; i += TONE_NT)
        if (lds[i]) ZJ_TONE_GLOBAL_ADD(p.hist[img] + (uint64_t)(4 * i), lds[i]);
}

/* ---- the table build ----------------------------------------------------------------------------------------------- */
constexpr int TONE_LUT_BATCH = 256; // images per launch: 8 bytes of kernel arguments each

struct ToneLutParams {
    uint64_t hist;                   // uint32 [nimg][channels][256] (0: no op of the launch needs it)
    uint64_t luts;                   // uint8 [nimg][channels][256]
    int32_t op[TONE_LUT_BATCH], param[TONE_LUT_BATCH];
    int nimg, channels;
};
static_assert(sizeof(ToneLutParams) <= 4096, "kernel arguments: 4 KB");

// one workgroup's LDS: the bins, the two buffers of the 64-bit scan, what the reductions leave
struct ToneLutLds {
    uint64_t scan[2][256];
    uint64_t total;      // the sum of the bins
    uint32_t h[256];
    uint32_t lo, hi;     // the first and the last non-empty bin (none: 255, 0)
    uint32_t count;      // non-empty bins
    uint32_t pad;
};

// the product and the sum of autocontrast's t = (int)(i * scale + offset) are two roundings, as Pillow's Python doubles are:
// never one fused multiply-add.  hipcc contracts a * b + c by default, through __dmul_rn and __dadd_rn as well (they are a
// plain product and sum in HIP's headers), so contraction is switched off for these two functions: their instructions carry
// no `contract` flag and stay v_mul_f64 and v_add_f64 wherever they are inlined.  The emulation is built with
// -ffp-contract=off.
ZJ_HD double tone_mul(const double a, const double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a * b;
}
ZJ_HD double tone_add(const double a, const double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return a + b;
}

// channel c of image img: lane `tid`'s bin into LDS, the reductions' start values
ZJ_HD uint32_t tone_lut_load_phase(const ToneLutParams& p, const int img, const int c, const int tid, ToneLutLds& l)
{
    uint32_t hv = 0;
    if (tone_needs_hist(p.op[img]))
        hv = ZJ_TONE_TABLE(uint32_t, p.hist + 4 * ((uint64_t)(img * p.channels + c) * 256 + (uint64_t)tid));
    l.h[tid] = hv;
    l.scan[0][tid] = hv;
    if (tid == 0) { l.lo = 255; l.hi = 0; l.count = 0; l.total = 0; }
    return hv;
}

// lo, hi, the count of non-empty bins and the total: LDS atomics
ZJ_HD void tone_lut_reduce_phase(const int tid, const uint32_t hv, ToneLutLds& l)
{
    if (hv == 0) return;
    ZJ_TONE_LDS_MIN(&l.lo, (uint32_t)tid);
    ZJ_TONE_LDS_MAX(&l.hi, (uint32_t)tid);
    ZJ_TONE_LDS_ADD(&l.count, 1u);
    ZJ_TONE_LDS_ADD(&l.total, (uint64_t)hv);
}

// one step of the inclusive scan over the 256 bins in 64 bits: distance d = 1 << step, from buffer step & 1 into the other
// (after the 8 steps the sums are in buffer 0)
ZJ_HD void tone_lut_scan_phase(const int tid, const int step, ToneLutLds& l)
{
    const int d = 1 << step, from = step & 1;
    l.scan[from ^ 1][tid] = l.scan[from][tid] + (tid >= d ? l.scan[from][tid - d] : 0);
}

// entry i of the table of (op, param) over the bins of l: Pillow's ImageOps
ZJ_HD uint32_t tone_lut_entry(const int32_t op, const int32_t param, const int i, const ToneLutLds& l)
{
    const uint32_t u = (uint32_t)i;
    if (op == TONE_INVERT) return 255u - u;
    if (op == TONE_POSTERIZE) return u & ~((1u << (8 - param)) - 1u) & 255u;
    if (op == TONE_SOLARIZE) return i < param ? u : 255u - u;
    if (op == TONE_AUTOCONTRAST) {
        if (l.hi <= l.lo) return u;
        const double scale = 255.0 / (double)(int)(l.hi - l.lo), offset = tone_mul(-(double)(int)l.lo, scale);
        const int t = (int)tone_add(tone_mul((double)i, scale), offset); // (toward zero; |.| <= 255 x 255)
        return (uint32_t)(t < 0 ? 0 : t > 255 ? 255 : t);
    }
    if (op == TONE_EQUALIZE) {
        if (l.count <= 1) return u;
        const uint64_t step = (l.total - (uint64_t)l.h[l.hi]) / 255u;
        if (step == 0) return u;
        const uint64_t n = step / 2 + (l.scan[0][i] - (uint64_t)l.h[i]); // (the bins in front of i: the exclusive sum)
        const uint64_t q = n / step;
        return (uint32_t)(q > 255 ? 255 : q);
    }
    return u;
}

ZJ_HD void tone_lut_entry_phase(const ToneLutParams& p, const int img, const int c, const int tid, const ToneLutLds& l)
{
    const uint32_t t = tone_lut_entry(p.op[img], p.param[img], tid, l);
    ZJ_TONE_TABLE_PUT(p.luts + (uint64_t)(img * p.channels + c) * 256 + (uint64_t)tid, (uint8_t)t);
}

/* ---- the lookup ---------------------------------------------------------------------------------------------------- */
constexpr int LUT_BATCH = 128; // images per launch: 28 bytes of kernel arguments each

struct LutParams {
    uint64_t in[LUT_BATCH], out[LUT_BATCH];
    uint32_t wh[LUT_BATCH];                             // w | h << 16
    uint32_t in_pitch[LUT_BATCH], out_pitch[LUT_BATCH]; // bytes between rows (CHW: of a plane's rows)
    uint64_t luts;                                      // uint8 [nimg][channels][256]
    int nimg;
};
static_assert(sizeof(LutParams) <= 4096, "kernel arguments: 4 KB");

ZJ_HD int lut_grid(const LutParams& p)
{
    uint32_t most = 1;
    for (int i = 0; i < p.nimg; i++)
        if (tone_items(p.wh[i]) > most) most = tone_items(p.wh[i]);
    return (int)((most + TONE_NT - 1) / TONE_NT);
}
ZJ_HD bool lut_block_active(const LutParams& p, const int img, const uint32_t wg)
{
    return (uint64_t)wg * TONE_NT < (uint64_t)tone_items(p.wh[img]);
}

// the image's C x 256 table bytes into LDS, once per workgroup: dwords where the table's address allows, else bytes
template <int C>
ZJ_HD void lut_table_phase(const LutParams& p, const int img, const int tid, uint32_t* lds)
{
    const uint64_t t = p.luts + (uint64_t)img * (C * 256);
    for (int i = tid; i < C * 64; i += TONE_NT) {
        const uint64_t a = t + (uint64_t)(4 * i);
        if ((t & 3u) == 0) lds[i] = ZJ_TONE_TABLE(uint32_t, a);
        else
            lds[i] = (uint32_t)ZJ_TONE_TABLE(uint8_t, a) | ((uint32_t)ZJ_TONE_TABLE(uint8_t, a + 1) << 8) |
                     ((uint32_t)ZJ_TONE_TABLE(uint8_t, a + 2) << 16) | ((uint32_t)ZJ_TONE_TABLE(uint8_t, a + 3) << 24);
    }
}

// One lane's work: item `id` (workgroup x TONE_NT + lane) of image img, run id % runs of row id / runs, loaded whole, every
// byte looked up in the LDS table of its channel, and stored.  A lane reads all of its run before it stores any of it and
// no other lane touches those bytes: the output may be the input itself (same address, same pitch).
template <int C, bool CHW>
ZJ_HD void lut_map_phase(const LutParams& p, const int img, const uint32_t id, const uint8_t* lds)
{
    const int w = (int)(p.wh[img] & 0xffffu), h = (int)(p.wh[img] >> 16);
    const uint32_t runs = (uint32_t)cmyk_runs(w);
    const uint32_t row = id / runs, x0 = (id - row * runs) * TONE_RUN;
    if (row >= (uint32_t)h) return;
    const int n = w - (int)x0 < TONE_RUN ? w - (int)x0 : TONE_RUN;
    if (C == 3 && !CHW) {
        uint32_t a[12], o[12];
        cmyk_get<12>(p.in[img] + (uint64_t)row * p.in_pitch[img] + (uint64_t)x0 * 3, a, 3 * n);
#pragma unroll
        for (int i = 0; i < 12; i++) o[i] = 0;
#pragma unroll
        for (int k = 0; k < 3 * TONE_RUN; k++) o[k >> 2] |= (uint32_t)lds[(k % 3) * 256 + tone_byte<12>(a, k)] << (8 * (k & 3));
        expand_put<12>(p.out[img] + (uint64_t)row * p.out_pitch[img] + (uint64_t)x0 * 3, o, 3 * n);
    } else {
        const uint64_t in_plane = (uint64_t)p.in_pitch[img] * (uint64_t)h, out_plane = (uint64_t)p.out_pitch[img] * (uint64_t)h;
        uint32_t a[C][4], o[C][4];
#pragma unroll
        for (int c = 0; c < C; c++) // (all read before any is stored)
            cmyk_get<4>(p.in[img] + (uint64_t)c * in_plane + (uint64_t)row * p.in_pitch[img] + x0, a[c], n);
#pragma unroll
        for (int c = 0; c < C; c++) {
#pragma unroll
            for (int i = 0; i < 4; i++) o[c][i] = 0;
#pragma unroll
            for (int k = 0; k < TONE_RUN; k++) o[c][k >> 2] |= (uint32_t)lds[c * 256 + tone_byte<4>(a[c], k)] << (8 * (k & 3));
        }
#pragma unroll
        for (int c = 0; c < C; c++) expand_put<4>(p.out[img] + (uint64_t)c * out_plane + (uint64_t)row * p.out_pitch[img] + x0, o[c], n);
    }
}

} // namespace zj
