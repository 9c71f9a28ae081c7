// zj_resize_aa.h -- the antialiased (triangle-filter) resize of zj_resize_filtered_device (ZJ_RESIZE_BILINEAR_AA).
//
// The definition's arithmetic as ZJ_HD functions, and the phases of one workgroup, shared by the kernel (zj_resize_aa.hip)
// and its CPU emulation (tests/emu_resize_aa, a g++ ZJ_EMU build).  The output conversions and stores are zj_resize.h's.
//   AaAxis / aa_axis   one axis, one destination index: its tap range [lo, hi] and the sum S of its unnormalised weights
//   aa_prefix          C_j, the prefix sum of the unnormalised weights, in closed form (two arithmetic progressions)
//   aa_weight          w_j = R_j - R_{j-1}, R_j = floor((C_j 2^14 + S / 2) / S): non-negative, summing to exactly 2^14
//   aa_*_phase         the workgroup's phases, each run by every lane between two barriers
#pragma once
#include "zj_resize.h"

namespace zj {

constexpr int AA_NT = 256;                    // threads per workgroup
constexpr int AA_ROWS = 4;                    // output rows per workgroup
constexpr int AA_COLS = 64;                   // output columns per workgroup
constexpr int AA_GROUP = 2;                   // output pixels of one row per lane (every channel) in the horizontal pass
constexpr int AA_TROW = 2048;                 // u16 vertical sums per output row in LDS: one source-column piece
constexpr int AA_WORD = 8;                    // source bytes per lane per row in the vertical pass
constexpr int AA_PLANE_WORDS = 85;            // CHW input: lanes per plane (3 x 85 of the 256)
constexpr int AA_PLANE_T = AA_PLANE_WORDS * AA_WORD; // ... and the plane's stride in a row of t (680)
constexpr int AA_WCAP = 2 * (AA_TROW + AA_COLS);     // column weights of one piece (see aa_col_count_phase)

// source pixels per piece: HWC C x PW bytes <= 2048; CHW 680 per plane
template <bool IN_CHW, int C>
ZJ_HD constexpr int aa_piece_w() { return IN_CHW ? AA_PLANE_T : AA_TROW / C; }

// One axis (source length n 1..65535, destination length m 1..8192), destination index i.  Positions in units of 1/(2m)
// source pixels: centre c = (2i + 1) n, source pixel j at (2j + 1) m, D = 2 max(n, m); W_j = max(0, D - |(2j + 1) m - c|).
// Every quantity but S fits in int32: c, (2j + 1) m < 2^30 + 2^20 and D <= 131070.
struct AaAxis {
    int lo, hi;  // the taps with W_j > 0, within [0, n)
    int c, D, m;
    int jc;      // the last j with (2j + 1) m <= c (-1: none): W rises up to it, falls after it
    uint64_t S;  // sum of W_j, < 2^35
};

ZJ_HD int aa_W(const AaAxis& a, const int j)
{
    const int p = (2 * j + 1) * a.m;
    return p <= a.c ? a.D - a.c + p : a.D + a.c - p;
}

// sum of W_k over k in [a, b] on one side of the centre: an arithmetic progression of step 2m, so W_a + W_b is even
ZJ_HD uint64_t aa_run(const AaAxis& x, const int a, const int b)
{
    if (a > b) return 0;
    return (uint64_t)(b - a + 1) * (uint64_t)((aa_W(x, a) + aa_W(x, b)) / 2);
}

// C_j = sum of W_k, k in [lo, min(j, hi)]; 0 below lo
ZJ_HD uint64_t aa_prefix(const AaAxis& x, int j)
{
    if (j < x.lo) return 0;
    if (j > x.hi) j = x.hi;
    const int l1 = j < x.jc ? j : x.jc;
    const int r0 = x.lo > x.jc + 1 ? x.lo : x.jc + 1;
    return aa_run(x, x.lo, l1) + aa_run(x, r0, j);
}

ZJ_HD AaAxis aa_axis(const uint32_t i, const uint32_t n, const uint32_t m)
{
    AaAxis a;
    a.m = (int)m;
    a.c = (int)((2u * i + 1u) * n);
    a.D = 2 * (int)(n > m ? n : m);
    const int m2 = 2 * a.m;
    const int t = a.c - a.D - a.m;                 // (2j + 1) m > c - D  <=>  2jm > t
    a.lo = t < 0 ? 0 : t / m2 + 1;
    a.hi = (a.c + a.D - a.m - 1) / m2;             // (2j + 1) m < c + D
    if (a.hi > (int)n - 1) a.hi = (int)n - 1;
    a.jc = a.c >= a.m ? (a.c - a.m) / m2 : -1;
    a.S = 0;
    a.S = aa_prefix(a, a.hi);
    return a;
}

// R_j = floor((C_j 2^14 + S / 2) / S), 0 .. 2^14.  The numerator is below 2^50 and S below 2^35, both exact in a double: the
// correctly rounded quotient is within one of the floor, which one exact integer step settles.
ZJ_HD uint32_t aa_R(const AaAxis& x, const int j)
{
    const uint64_t num = (aa_prefix(x, j) << 14) + (x.S >> 1);
    uint64_t q = (uint64_t)((double)num / (double)x.S);
    const long long r = (long long)(num - q * x.S);
    if (r < 0) q--;
    else if (r >= (long long)x.S) q++;
    return (uint32_t)q;
}

ZJ_HD uint32_t aa_weight(const AaAxis& x, const int j) { return aa_R(x, j) - aa_R(x, j - 1); }

// ---- the workgroup ---------------------------------------------------------------------------------------------------------
// (image, AA_ROWS output rows from r0, AA_COLS output columns from x0).  The block's source columns [sx0, sx1] are walked
// in pieces of aa_piece_w() pixels; per piece:
//   col_*       the block's column taps that fall in the piece: first tap, count, offset in the weight table, the weights
//               (every lane, a binary search for its entry's column)
//   vertical    per output row: the row's weights into LDS AA_NT at a time; each lane sums 8 source bytes of the piece
//               over the row's taps (dword loads, coalesced across the wave), then t = (sum + 32) >> 6 into LDS as u16
//   horizontal  each lane adds w x t over the piece's taps of its AA_GROUP pixels x C channels to its running sums
// and after the last piece, v = (sum + 32) >> 6 goes through zj_resize.h's conversion and store.
struct AaShared {
    uint16_t t[AA_ROWS][AA_TROW];
    uint16_t cw[AA_WCAP];
    uint16_t rw[AA_NT];
    AaAxis col[AA_COLS];
    int ca[AA_COLS], ccnt[AA_COLS], coff[AA_COLS + 1];
};

struct AaLane {
    uint32_t v[AA_WORD];            // vertical sums of the lane's 8 bytes (one output row at a time)
    uint32_t h[AA_GROUP * 3];       // horizontal sums: pixel g, channel c at g * C + c
};

struct AaBlock {
    const uint8_t* src;
    long long plane;                // CHW: bytes between planes
    int pitch, n_w, n_h, ow, oh, r0, x0, ncols, nrows;
    bool flip;
};

ZJ_HD AaBlock aa_block(const ResizeParams& p, const int img, const int bx, const int by, const bool in_chw)
{
    AaBlock b;
    const uint32_t wh = p.wh[img];
    b.n_w = (int)(wh & 0xffffu); b.n_h = (int)(wh >> 16);
    b.pitch = (int)p.pitch[img];
    b.plane = in_chw ? (long long)b.pitch * b.n_h : 0;
    b.src = (const uint8_t*)p.in[img];
    b.ow = p.out_w; b.oh = p.out_h;
    b.x0 = bx * AA_COLS; b.r0 = by * AA_ROWS;
    b.ncols = b.ow - b.x0 < AA_COLS ? b.ow - b.x0 : AA_COLS;
    b.nrows = b.oh - b.r0 < AA_ROWS ? b.oh - b.r0 : AA_ROWS;
    b.flip = (p.flip[img >> 5] >> (img & 31)) & 1u;
    return b;
}

// output column x0 + k of the block -> its destination index (flip mirrors the output columns)
ZJ_HD uint32_t aa_dest_col(const AaBlock& b, const int k) { return (uint32_t)(b.flip ? b.ow - 1 - (b.x0 + k) : b.x0 + k); }

ZJ_HD void aa_col_axes_phase(const AaBlock& b, AaShared& s, const int tid)
{
    if (tid < b.ncols) s.col[tid] = aa_axis(aa_dest_col(b, tid), (uint32_t)b.n_w, (uint32_t)b.ow);
}

// the block's source columns: from the first tap of its lowest destination index to the last of its highest
ZJ_HD void aa_span(const AaBlock& b, const AaShared& s, int& sx0, int& sx1)
{
    sx0 = s.col[b.flip ? b.ncols - 1 : 0].lo;
    sx1 = s.col[b.flip ? 0 : b.ncols - 1].hi;
}

// The columns' taps within the piece [px0, px1).  A downscale puts every source pixel under at most two output columns
// (2i + 1 lies in an open interval of length 4), an upscale gives every output column at most two taps: at most
// 2 (piece + AA_COLS) entries, AA_WCAP.
ZJ_HD void aa_col_count_phase(const AaBlock& b, AaShared& s, const int px0, const int px1, const int tid)
{
    if (tid < b.ncols) {
        const AaAxis& a = s.col[tid];
        const int lo = a.lo > px0 ? a.lo : px0, hi = a.hi < px1 - 1 ? a.hi : px1 - 1;
        s.ca[tid] = lo;
        s.ccnt[tid] = hi >= lo ? hi - lo + 1 : 0;
    }
}

ZJ_HD void aa_col_offset_phase(const AaBlock& b, AaShared& s, const int tid)
{
    if (tid <= b.ncols) {
        int o = 0;
        for (int k = 0; k < tid; k++) o += s.ccnt[k];
        s.coff[tid] = o;
    }
}

ZJ_HD void aa_col_weights_phase(const AaBlock& b, AaShared& s, const int tid)
{
    const int total = s.coff[b.ncols];
    for (int e = tid; e < total; e += AA_NT) {
        int lo = 0, hi = b.ncols - 1; // the column k with coff[k] <= e < coff[k + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s.coff[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        s.cw[e] = (uint16_t)aa_weight(s.col[lo], s.ca[lo] + (e - s.coff[lo]));
    }
}

// the weights of taps [lo + j0, lo + j0 + AA_NT) of one output row
ZJ_HD void aa_row_weights_phase(const AaAxis& ra, AaShared& s, const int j0, const int tid)
{
    const int j = ra.lo + j0 + tid;
    s.rw[tid] = j <= ra.hi ? (uint16_t)aa_weight(ra, j) : 0;
}

// The lane's 8 bytes of the piece: HWC one segment of C (px1 - px0) bytes, lanes 0..255; CHW one segment per plane of
// px1 - px0 bytes, 85 lanes per plane.  seg < 0: the lane has none.
template <bool IN_CHW, int C>
ZJ_HD void aa_lane_seg(const int tid, const int px0, const int px1, int& seg, long long& off, int& len, int& q0)
{
    const int w = IN_CHW ? tid % AA_PLANE_WORDS : tid;
    seg = IN_CHW ? tid / AA_PLANE_WORDS : 0;
    len = IN_CHW ? px1 - px0 : (px1 - px0) * C;
    q0 = AA_WORD * w;
    if (seg >= (IN_CHW ? 3 : 1) || q0 >= len) seg = -1;
    off = IN_CHW ? px0 : (long long)px0 * C;
}

// 8 bytes at a (any alignment) of a segment whose last byte is at `last`: three dword loads, the 2nd and 3rd only where
// they start at or before that byte (a dword that holds a byte of the segment never crosses the end of the allocation)
ZJ_HD void aa_load8(const uint8_t* a, const uint8_t* last, uint32_t& lo, uint32_t& hi)
{
    const uintptr_t ua = (uintptr_t)a;
    const uint8_t* ab = (const uint8_t*)(ua & ~(uintptr_t)3);
    const uint32_t sh = 8u * (uint32_t)(ua & 3u);
#if defined(ZJ_EMU)
    uint32_t d0, d1 = 0, d2 = 0;
    memcpy(&d0, ab, 4);
    if (ab + 4 <= last) memcpy(&d1, ab + 4, 4);
    if (ab + 8 <= last) memcpy(&d2, ab + 8, 4);
#else
    const uint32_t* const g = ZJ_RZ_GLOBAL(const uint32_t, ab);
    const uint32_t d0 = g[0];
    const uint32_t d1 = ab + 4 <= last ? g[1] : 0u;
    const uint32_t d2 = ab + 8 <= last ? g[2] : 0u;
#endif
    lo = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
    hi = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
}

// taps [lo + j0, lo + j0 + nt) of one output row: the lane's 8 bytes of each source row times the row's weight
template <bool IN_CHW, int C>
ZJ_HD void aa_vertical_phase(const AaBlock& b, const AaShared& s, AaLane& l, const int lo, const int j0, const int nt,
                             const int px0, const int px1, const int tid)
{
    int seg, len, q0;
    long long off;
    aa_lane_seg<IN_CHW, C>(tid, px0, px1, seg, off, len, q0);
    if (seg < 0) return;
    const uint8_t* const base = b.src + (long long)seg * b.plane + off;
#pragma unroll 4
    for (int k = 0; k < nt; k++) {
        const uint32_t w = s.rw[k];
        const uint8_t* const row = base + (long long)(lo + j0 + k) * b.pitch;
        uint32_t x0, x1;
        aa_load8(row + q0, row + len - 1, x0, x1);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            l.v[q] += w * ((x0 >> (8 * q)) & 255u);
            l.v[4 + q] += w * ((x1 >> (8 * q)) & 255u);
        }
    }
}

// the row's vertical sums rounded, t = (sum + 32) >> 6 (<= 255 x 2^8), for the lane's bytes of its segment; sums cleared
template <bool IN_CHW, int C>
ZJ_HD void aa_vertical_store(AaShared& s, AaLane& l, const int rr, const int px0, const int px1, const int tid)
{
    int seg, len, q0;
    long long off;
    aa_lane_seg<IN_CHW, C>(tid, px0, px1, seg, off, len, q0);
    if (seg >= 0) {
        uint16_t* const t = s.t[rr] + (IN_CHW ? seg * AA_PLANE_T : 0);
#pragma unroll
        for (int q = 0; q < AA_WORD; q++)
            if (q0 + q < len) t[q0 + q] = (uint16_t)((l.v[q] + 32u) >> 6);
    }
#pragma unroll
    for (int q = 0; q < AA_WORD; q++) l.v[q] = 0;
}

// the lane's item in the horizontal pass: output row rr, pixels [k0, k0 + count) of the block (count < 0: none)
ZJ_HD int aa_item(const AaBlock& b, const int tid, int& rr, int& k0)
{
    constexpr int GPR = AA_COLS / AA_GROUP;
    rr = tid / GPR;
    k0 = (tid % GPR) * AA_GROUP;
    if (rr >= b.nrows || k0 >= b.ncols) return -1;
    return b.ncols - k0 < AA_GROUP ? b.ncols - k0 : AA_GROUP;
}

template <bool IN_CHW, int C>
ZJ_HD void aa_horizontal_phase(const AaBlock& b, const AaShared& s, AaLane& l, const int px0, const int tid)
{
    int rr, k0;
    const int cnt = aa_item(b, tid, rr, k0);
    if (cnt < 0) return;
    const uint16_t* const t = s.t[rr];
#pragma unroll
    for (int g = 0; g < AA_GROUP; g++) {
        if (g >= cnt) continue;
        const int k = k0 + g, n = s.ccnt[k], o = s.coff[k], a = s.ca[k] - px0;
        for (int q = 0; q < n; q++) {
            const uint32_t w = s.cw[o + q];
#pragma unroll
            for (int c = 0; c < C; c++) l.h[g * C + c] += w * t[IN_CHW ? c * AA_PLANE_T + a + q : (a + q) * C + c];
        }
    }
}

// v = (sum + 32) >> 6 (<= 255 x 2^16, the meaning of zj_resize.h's v), converted and stored as resize_group does
template <int C, int DT, bool NHWC>
ZJ_HD void aa_store_phase(const ResizeParams& p, const AaBlock& b, const AaLane& l, uint8_t* img_out, const int tid)
{
    constexpr int G = AA_GROUP, E = resize_elem_bytes(DT);
    int rr, k0;
    const int cnt = aa_item(b, tid, rr, k0);
    if (cnt < 0) return;
    const int r = b.r0 + rr, x0 = b.x0 + k0;
    constexpr int RUNS = NHWC ? 1 : C, RUN = NHWC ? G * C : G, NB = RUN * E;
#pragma unroll
    for (int q = 0; q < RUNS; q++) {
        uint32_t v[RUN];
#pragma unroll
        for (int j = 0; j < RUN; j++) v[j] = (l.h[NHWC ? j : j * C + q] + 32u) >> 6;
        uint32_t w[(NB + 3) / 4];
#pragma unroll
        for (int wi = 0; wi < (NB + 3) / 4; wi++) {
            if (DT == RZ_F32) {
                const int c = NHWC ? wi % C : q;
                w[wi] = f32_bits(resize_f32(v[wi], p.scale[c], p.bias[c]));
            } else if (DT == RZ_U8) {
                uint32_t d = 0;
#pragma unroll
                for (int bb = 0; bb < 4; bb++)
                    if (4 * wi + bb < RUN) d |= resize_u8(v[4 * wi + bb]) << (8 * bb);
                w[wi] = d;
            } else {
                const int j0 = 2 * wi, j1 = 2 * wi + 1;
                const int c0 = NHWC ? j0 % C : q, c1 = NHWC ? j1 % C : q;
                const float a = resize_f32(v[j0], p.scale[c0], p.bias[c0]);
                const float bv = j1 < RUN ? resize_f32(v[j1], p.scale[c1], p.bias[c1]) : 0.f;
                w[wi] = resize_pack2<DT>(a, bv);
            }
        }
        uint8_t* const dst = img_out + resize_elem<C, NHWC>(NHWC ? 0 : q, r, x0, b.ow, b.oh) * E;
        resize_store<E, NB>(dst, w, (NHWC ? cnt * C : cnt) * E);
    }
}

} // namespace zj
