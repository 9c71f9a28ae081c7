// zj_crop_tensor.h -- crop windows decoded straight into a normalised tensor, no resize (zj_decode_crops_tensor_device,
// DESIGN.md 3.14).
//
// The crop kernel's tile decode (zj_device.h: crop_locate, CropStage) with another copy-out: every staged byte a workgroup
// owns becomes ONE tensor element, converted on the way out with zj_resize.h's conversions (resize_f32, resize_pack2) and
// placed by resize_elem.  The ZJ_DEV / ZJ_HD functions here are shared by the kernels (zj_crop_tensor.hip) and their CPU
// emulation (tests/emu_crop_tensor, a g++ ZJ_EMU build).
#pragma once

#include "zj_device.h"
#include "zj_plan.h"   // the host side below: Plan, CropPlan, fill_crop_params_win
#include "zj_resize.h"

namespace zj {

constexpr int CROP_TENSOR_MAX_Z = 65535;   // a grid's z extent: frames of one launch
constexpr int CROP_TENSOR_SHIFT = 5;       // log2 of the frames a record of the one-geometry call holds
static_assert((1 << CROP_TENSOR_SHIFT) == SCATTER_MAX, "a record holds SCATTER_MAX frames");
constexpr int CROP_TENSOR_RUN = 8; // elements of one lane's store: 16 bytes of a 16-bit type, 32 of float32, 8 of u8

// One record of a launch's table (zj_crop_tensor.hip): the crop launch's arguments for up to SCATTER_MAX frames of ONE
// geometry (cp.p.fptr[f][3]: frame f's IMAGE of the tensor; cp.out_pitch 0), plus the output side.  dtype, layout and flip are workgroup-uniform run-time switches of the copy-out.
struct CropTensorParams {
    CropParams cp;
    float scale[3], bias[3];      // per channel: s_c = scale_c * 2^-16, bias_c (zj_resize.h: ResizeParams)
    int dtype;                    // ZJ_DTYPE_*
    int nhwc;                     // 1: [h, w, C], 0: [C, h, w]
    uint32_t flip;                // bit f: frame f of the launch is mirrored
};
static_assert(SCATTER_MAX <= 32, "one flip bit per frame of a launch");

// The converted zero for the window rows at or below rows_covered (Q6): blockIdx.y = frame, blockIdx.x = window row - rmin
struct CropTensorZero {
    uint64_t fptr[SCATTER_MAX];   // per frame: its image of the tensor
    uint32_t y0[SCATTER_MAX];     // per frame: the window's first frame row
    int rows_covered, w, h, ch, dtype, nhwc, nframes;
    int rmin;                     // the first window row that is such a row in any frame: the grid is the h - rmin rows from it
    float scale[3], bias[3];
};

// bytes of one image: C * w * h elements (0: no such dtype or channel count).  No 8192 limit: nothing is resized.
inline size_t crop_tensor_len(int channels, unsigned w, unsigned h, int dtype)
{
    if (channels <= 0 || w == 0 || h == 0 || w > 65535 || h > 65535) return 0;
    return (size_t)channels * w * h * (size_t)resize_elem_bytes(dtype);
}

// The output side of one workgroup, read from the launch's arguments once (all of it uniform)
struct CropTensorOut {
    float scale[3], bias[3];
    int w, h;                     // the window: the image is [C, h, w] or [h, w, C]
    int dtype;
    bool nhwc, flip;
};

// (fz: the frame's index in the launch, uniform)
ZJ_DEV CropTensorOut crop_tensor_out(const CropTensorParams& tp, const int fz)
{
    CropTensorOut o;
    for (int k = 0; k < 3; k++) { o.scale[k] = tp.scale[k]; o.bias[k] = tp.bias[k]; }
    const uint32_t wh = tp.cp.size[fz];
    o.w = (int)(wh & 0xffffu); o.h = (int)(wh >> 16);
    o.dtype = tp.dtype;
    o.nhwc = tp.nhwc != 0;
    o.flip = ((tp.flip >> fz) & 1u) != 0;
    return o;
}

// channel c's factor of three, c a per-lane value: a select between VALUES (an indexed read of a record by a vector index
// would go through scratch, and a select between references to it becomes control flow).  Once per run, never per element.
ZJ_HD float crop_tensor_pick(const float v0, const float v1, const float v2, const int c) { return c == 0 ? v0 : (c == 1 ? v1 : v2); }

// (the compiler is told what the copy-out's arithmetic guarantees, so that resize_store keeps its one matching path)
#if defined(ZJ_EMU)
#define ZJ_CT_ASSUME(x) ((void)0)
#else
#define ZJ_CT_ASSUME(x) __builtin_assume(x)
#endif

// One lane's run: cnt (1..8) consecutive DESTINATION elements of one tensor row, the first at dst.  pos: the first element's
// place in its row -- NHWC: element index (column * C + channel), NCHW: column of channel plane cf.  srow: index in `stage`
// of the window row's byte 0.  Element k of the run is the conversion of the staged byte of source pixel
// (flip ? w - 1 - column : column), channel c.
// What depends on the lane -- the first element's channel -- is settled once per run, as the three factors and address
// terms of the channels in the run's own order; element k then takes entry k % C, a compile-time index, at the address
// first + k * step (+ its term).  NCHW: every entry is channel cf's.  The staged byte of element E = column * C + c of a
// mirrored NHWC row is C (w - 1) - E + 2c.
// A full run starts on a boundary of its own size in the destination (the caller's blocks) and goes out with the widest
// stores; a shorter one element by element.  The dtype is a uniform switch around the packing and the store alone: one copy
// of the addressing per kernel, not four.
template <int C>
ZJ_DEV void crop_tensor_run(const CropTensorOut& tp, const uint8_t* stage, const int srow, uint8_t* dst, const int cnt,
                            const int pos, const int cf)
{
    constexpr int G = CROP_TENSOR_RUN;
    const float s0 = tp.scale[0], s1 = tp.scale[1], s2 = tp.scale[2], b0 = tp.bias[0], b1 = tp.bias[1], b2 = tp.bias[2];
    const bool nhwc = tp.nhwc, flip = tp.flip;
    const int c0 = nhwc ? pos % C : cf;
    float sr[C], br[C];
    int adj[C];
#pragma unroll
    for (int j = 0; j < C; j++) {
        int c = nhwc ? c0 + j : cf;
        c -= c >= C ? C : 0;
        sr[j] = crop_tensor_pick(s0, s1, s2, c);
        br[j] = crop_tensor_pick(b0, b1, b2, c);
        adj[j] = nhwc && flip ? 2 * c : 0;
    }
    const int step = nhwc ? (flip ? -1 : 1) : (flip ? -C : C);
    const int first = srow + (nhwc ? (flip ? C * (tp.w - 1) - pos : pos) : (flip ? tp.w - 1 - pos : pos) * C + cf);
    uint32_t px[G];
    float f[G];
#pragma unroll
    for (int k = 0; k < G; k++) {
        const int at = first + k * step + adj[k % C];
        px[k] = stage[k < cnt ? at : first + adj[0]]; // (past the run: its first byte again, never outside the staging)
        f[k] = resize_f32(px[k] << 16, sr[k % C], br[k % C]);
    }
    if (tp.dtype == RZ_F32) {
        uint32_t wd[G];
#pragma unroll
        for (int k = 0; k < G; k++) wd[k] = f32_bits(f[k]);
        if (cnt == G) { ZJ_CT_ASSUME((reinterpret_cast<uintptr_t>(dst) & 15u) == 0); resize_store<4, 4 * G>(dst, wd, 4 * G); }
        else { ZJ_CT_ASSUME(cnt < G); resize_store<4, 4 * G>(dst, wd, cnt * 4); }
    } else if (tp.dtype == RZ_U8) {
        uint32_t wd[G / 4];
#pragma unroll
        for (int k = 0; k < G / 4; k++) wd[k] = px[4 * k] | px[4 * k + 1] << 8 | px[4 * k + 2] << 16 | px[4 * k + 3] << 24;
        if (cnt == G) { ZJ_CT_ASSUME((reinterpret_cast<uintptr_t>(dst) & 7u) == 0); resize_store<1, G>(dst, wd, G); }
        else { ZJ_CT_ASSUME(cnt < G); resize_store<1, G>(dst, wd, cnt); }
    } else {
        uint32_t wd[G / 2];
#pragma unroll
        for (int k = 0; k < G / 2; k++)
            wd[k] = tp.dtype == RZ_BF16 ? resize_pack2<RZ_BF16>(f[2 * k], f[2 * k + 1]) : resize_pack2<RZ_F16>(f[2 * k], f[2 * k + 1]);
        if (cnt == G) { ZJ_CT_ASSUME((reinterpret_cast<uintptr_t>(dst) & 15u) == 0); resize_store<2, 2 * G>(dst, wd, 2 * G); }
        else { ZJ_CT_ASSUME(cnt < G); resize_store<2, 2 * G>(dst, wd, cnt * 2); }
    }
}

// Copy-out of the window bytes [s.b0, s.b1) of the frame rows [s.r0, s.r1) (b0 < b1) into frame s.frame's image `img`.
// The span's WHOLE pixels go out as runs of CROP_TENSOR_RUN elements aligned in the DESTINATION (one run per row for NHWC,
// one per row and channel for NCHW; a tensor row starts at element r * w, so the alignment differs from row to row); the
// elements in front of a run's first aligned block and behind its last, and the bytes of a pixel the span holds only a
// part of, go out one element at a time.  The span's ends may therefore fall anywhere: every owned byte is written as
// exactly one element by exactly this workgroup.
// An item is (row, run, aligned block) or (row, partial-pixel byte); a lane takes items tid, tid + nthreads, ..., counted
// on as (row, item of the row) without a division per item.
template <int HS, int VS, int OUT>
ZJ_DEV void crop_copyout_tensor(const CropTensorOut& tp, const CropSpan& s, const int tid, const int nthreads,
                                const uint8_t* stage, uint8_t* img)
{
    using S = CropStage<HS, VS, OUT>;
    using Cf = Cfg<HS, VS, OUT>;
    constexpr int C = S::BPP, G = CROP_TENSOR_RUN;
    static_assert(S::NPL == 1, "HWC staging only");
    const int E = resize_elem_bytes(tp.dtype), A = G * E; // bytes of an element, of an aligned block
    const int w = tp.w, h = tp.h;
    const bool nhwc = tp.nhwc, flip = tp.flip;
    // the owned bytes of a WINDOW row, their whole pixels [pa, pb), the bytes in front [j0, hend) and behind [tbeg, j1)
    const int j0 = s.b0 - s.x * C, j1 = s.b1 - s.x * C;
    const int pa = (j0 + C - 1) / C, pb = j1 / C;
    const int hend = pa * C < j1 ? pa * C : j1;
    const int tbeg = pb * C > hend ? pb * C : hend;
    const int npx = pb > pa ? pb - pa : 0;
    const int runs = nhwc ? 1 : C;
    const int n = nhwc ? npx * C : npx;                                                    // elements of a run
    const int pos0 = nhwc ? (flip ? (w - pb) * C : pa * C) : (flip ? w - pb : pa);        // its first, in the row
    const int nblk = (n + G - 1) / G + 1;                                                  // aligned blocks it touches, at most
    const int nsingle = 2 * (C - 1);                                                       // partial-pixel bytes, at most
    const int per = runs * nblk + nsingle;                                                 // items of a row
    const int nr = s.r1 - s.r0;
    // stage index of (row r0, window byte 0)
    const int sbase = (s.r0 - s.strip * Cf::SH) * S::PITCH + (s.x * C - (s.tile * Cf::TWY * S::BPP - S::MARGIN));
    const int dr = nthreads / per, dq = nthreads - dr * per; // (uniform)
    int ri = tid / per, q = tid - ri * per;
    for (; ri < nr; ri += dr, q += dq) {
        if (q >= per) { q -= per; ri++; if (ri >= nr) break; }
        const int r = s.r0 - s.y + ri;
        int run = 0, bq = q;
#pragma unroll
        for (int k = 0; k < C; k++)
            if (run < runs && bq >= nblk) { bq -= nblk; run++; } // (run == runs: the partial-pixel items behind the runs)
        long long el;       // the first element this lane writes, counted from the image's first
        int cnt, pos, cf;   // crop_tensor_run's
        if (run >= runs) {  // one byte of a pixel the span holds a part of
            const int t = q - runs * nblk;
            const int j = t < hend - j0 ? j0 + t : tbeg + (t - (hend - j0));
            if (j >= j1) continue;
            const int px = j / C, c = j - px * C;
            const int col = flip ? w - 1 - px : px;
            el = nhwc ? resize_elem<C, true>(c, r, col, w, h) : resize_elem<C, false>(c, r, col, w, h);
            cnt = 1; pos = nhwc ? col * C + c : col; cf = c;
        } else {
            if (n == 0) continue;
            const long long e0 = nhwc ? resize_elem<C, true>(0, r, 0, w, h) + pos0 : resize_elem<C, false>(run, r, pos0, w, h);
            // elements of the run's first aligned block that lie in front of the run
            const int lead = (int)(reinterpret_cast<uintptr_t>(img + e0 * E) & (uintptr_t)(A - 1)) / E;
            int k0 = G * bq - lead, k1 = k0 + G;
            if (k0 < 0) k0 = 0;
            if (k1 > n) k1 = n;
            if (k0 >= k1) continue;
            el = e0 + k0; cnt = k1 - k0; pos = pos0 + k0; cf = run;
        }
        crop_tensor_run<C>(tp, stage, sbase + ri * S::PITCH, img + el * E, cnt, pos, cf);
    }
}

// One thread's share of a zero row: window row r of frame fr, elements tid, tid + nthreads, ... of its C * w, each the
// conversion of a zero byte (bias[c], through the same two operations)
template <int DT>
ZJ_DEV void crop_tensor_zero_row(const CropTensorZero& z, const int fr, const int r, const int tid, const int nthreads)
{
    constexpr int E = resize_elem_bytes(DT);
    uint8_t* const img = ZJ_GLOBAL_PTR(uint8_t, z.fptr[fr]);
    const int n = z.ch * z.w;
    for (int i = tid; i < n; i += nthreads) {
        const int c = z.nhwc ? i % z.ch : i / z.w;
        const int col = z.nhwc ? i / z.ch : i - c * z.w;
        long long el;
        if (z.ch == 3) el = z.nhwc ? resize_elem<3, true>(c, r, col, z.w, z.h) : resize_elem<3, false>(c, r, col, z.w, z.h);
        else el = resize_elem<1, false>(0, r, col, z.w, z.h);
        const float f = DT == RZ_U8 ? 0.f : resize_f32(0u, crop_tensor_pick(z.scale[0], z.scale[1], z.scale[2], c), crop_tensor_pick(z.bias[0], z.bias[1], z.bias[2], c));
        uint32_t wd[1];
        if (DT == RZ_F32) wd[0] = f32_bits(f);
        else if (DT == RZ_U8) wd[0] = 0;
        else wd[0] = resize_pack2<DT>(f, f);
        uint8_t* const d = img + el * E;
        if (E == 4) *reinterpret_cast<uint32_t*>(d) = wd[0];
        else if (E == 2) *reinterpret_cast<uint16_t*>(d) = (uint16_t)wd[0];
        else *d = (uint8_t)wd[0];
    }
}

ZJ_DEV void crop_tensor_zero(const CropTensorZero& z, const int fr, const int r, const int tid, const int nthreads)
{
    if (r >= z.h || (int)z.y0[fr] + r < z.rows_covered) return;
    switch (z.dtype) {
    case RZ_F32: crop_tensor_zero_row<RZ_F32>(z, fr, r, tid, nthreads); break;
    case RZ_F16: crop_tensor_zero_row<RZ_F16>(z, fr, r, tid, nthreads); break;
    case RZ_BF16: crop_tensor_zero_row<RZ_BF16>(z, fr, r, tid, nthreads); break;
    default: crop_tensor_zero_row<RZ_U8>(z, fr, r, tid, nthreads); break;
    }
}

// ---- host side, shared by zj_api.cpp and the emulation -------------------------------------------------------------
// the descriptors that have a tensor: 3 or 1 channels, decoded as HWC rows at no pitch of the frame's own (the tensor's
// layout is the call's)
inline bool crop_tensor_desc_ok(const zj_frame_desc* d)
{
    return resize_channels(d) != 0 && d->out_layout == ZJ_LAYOUT_HWC && d->out_pitch == 0;
}

// The launch's arguments for frames [f0, f0 + n) of a call: every window cp.w x cp.h at origins[2f], origins[2f + 1], frame
// f's image at out + f * img_bytes.  s, b: the kernel's factors (3 each).  Returns whether any window reaches a row at or
// below rows_covered (the zero launch is needed).
inline bool crop_tensor_fill(const zj_frame_desc* d, const Plan& pl, const CropPlan& cp, const int16_t* const* y,
                             const int16_t* const* cb, const int16_t* const* cr, uint8_t* out, size_t img_bytes,
                             const unsigned* origins, int dtype, int nhwc, const float* s, const float* b, const uint8_t* flip,
                             size_t f0, int n, CropTensorParams& tp, CropTensorZero& z)
{
    const bool chroma = pl.out != OUT_GRAY;
    uint8_t* img[SCATTER_MAX];
    for (int f = 0; f < n; f++) img[f] = out + (f0 + f) * img_bytes;
    const int16_t* const* const py = y + f0;
    int nstrips = 0, ncols = 0;
    fill_crop_params_win(d, pl, cp, py, chroma ? cb + f0 : nullptr, chroma ? cr + f0 : nullptr, img, origins + 2 * f0, 2, 0, n, tp.cp,
                         nstrips, ncols);
    tp.cp.out_pitch = 0;
    tp.dtype = dtype; tp.nhwc = nhwc ? 1 : 0; tp.flip = 0;
    z = CropTensorZero{};
    z.rows_covered = pl.rows_covered; z.w = cp.w; z.h = cp.h; z.ch = cp.bpp; z.dtype = dtype; z.nhwc = tp.nhwc; z.nframes = n;
    for (int k = 0; k < 3; k++) { tp.scale[k] = z.scale[k] = s[k]; tp.bias[k] = z.bias[k] = b[k]; }
    z.rmin = cp.h;
    for (int f = 0; f < n; f++) {
        if (flip && flip[f0 + f]) tp.flip |= 1u << f;
        z.fptr[f] = (uint64_t)(uintptr_t)img[f];
        z.y0[f] = origins[2 * (f0 + f) + 1];
        const long long first = (long long)pl.rows_covered - z.y0[f]; // frame f's first such row (< 0: all of them)
        if (first < z.rmin) z.rmin = first < 0 ? 0 : (int)first;
    }
    return z.rmin < cp.h;
}

} // namespace zj
