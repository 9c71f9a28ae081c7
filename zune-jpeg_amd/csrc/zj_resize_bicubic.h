// zj_resize_bicubic.h -- the bicubic antialiased resize of zj_resize_filtered_device (ZJ_RESIZE_BICUBIC_AA).
//
// The definition's arithmetic as ZJ_HD functions, and the phases of one workgroup, shared by the kernel
// (zj_resize_bicubic.hip) and its CPU emulation (tests/emu_resize_bicubic, a g++ ZJ_EMU build).  The workgroup's shape
// (AA_COLS x AA_ROWS outputs, AA_NT lanes), its block and item rules and the output conversion and store are
// zj_resize_aa.h's.
//   BcAxis / bc_axis   one axis, one destination index: its tap range [lo, hi]
//   bc_K               K'_j, Keys' cubic (a = -1/2) at the quantised position of tap j: signed, |K'| <= 2^30
//   bc_R               R = floor((C 2^14 + S / 2) / S) of a signed prefix sum C; w_j = R_j - R_{j-1}, summing to exactly 2^14
//   BcSet              up to K outputs of one axis (the block's columns, or its rows) and a window of taps of each: their
//                      S, the prefix carried into the window, and where the window's weights lie in a table
//   bc_*_phase         the workgroup's phases, each run by every lane between two barriers
#pragma once
#include "zj_resize_aa.h"

namespace zj {

constexpr int BC_TROW = 1024;                  // int32 vertical sums per output row in LDS: one source-column piece
constexpr int BC_WORD = 4;                     // source bytes per lane per row in the vertical pass
constexpr int BC_PLANE_WORDS = 85;             // CHW input: lanes per plane (3 x 85 of the 256)
constexpr int BC_PLANE_T = BC_PLANE_WORDS * BC_WORD; // ... and the plane's stride in a row of t (340)
constexpr int BC_WCAP = 4 * (BC_TROW + AA_COLS);     // column weights of one piece (see bc_window_phase)
constexpr int BC_RCH = 256;                    // taps of one output row per pass over the source rows
constexpr int BC_T = 1 << 15;                  // the filter unit: positions are quantised to 1 / BC_T of it

// source pixels per piece: HWC C x PW bytes <= 1024; CHW 340 per plane
template <bool IN_CHW, int C>
ZJ_HD constexpr int bc_piece_w() { return IN_CHW ? BC_PLANE_T : BC_TROW / C; }

// One axis (source length n 1..65535, destination length m 1..8192), destination index i: centre c = (2i + 1) n, source
// pixel j at (2j + 1) m, D = 2 max(n, m); the taps are the j in [0, n) with |(2j + 1) m - c| < 2D.  c + 2D < 2^31.
struct BcAxis {
    int lo, hi;  // the taps, hi - lo + 1 <= 4 x 65535 + 1 ... cut at [0, n)
    int c, D, m;
};

ZJ_HD BcAxis bc_axis(const uint32_t i, const uint32_t n, const uint32_t m)
{
    BcAxis a;
    a.m = (int)m;
    a.c = (int)((2u * i + 1u) * n);
    a.D = 2 * (int)(n > m ? n : m);
    const int m2 = 2 * a.m;
    const int t = a.c - 2 * a.D - a.m;             // (2j + 1) m > c - 2D  <=>  2jm > t
    a.lo = t < 0 ? 0 : t / m2 + 1;
    a.hi = (a.c + 2 * a.D - a.m - 1) / m2;         // (2j + 1) m < c + 2D
    if (a.hi > (int)n - 1) a.hi = (int)n - 1;
    return a;
}

// K'_j of a tap j in [lo, hi].  d < 2D = qd D + rd with rd < D < 2^17, so q = floor(d 2^15 / D) = qd 2^15 +
// floor(rd 2^15 / D) in 32 bits.  K in its factored forms (the same integers as the polynomials of the definition):
//   q < T:  (T - q) (2 T^2 + 2 q T - 3 q^2) >= 0;   T <= q < 2T:  -(q - T) (2T - q)^2 <= 0
ZJ_HD int bc_K(const BcAxis& a, const int j)
{
    const int p = (2 * j + 1) * a.m;
    uint32_t d = (uint32_t)(p < a.c ? a.c - p : p - a.c);
    uint32_t q = 0;
    if (d >= (uint32_t)a.D) { d -= (uint32_t)a.D; q = BC_T; }
    q += (d << 15) / (uint32_t)a.D;
    long long K;
    if (q < (uint32_t)BC_T) {
        const long long ql = (long long)q, T = BC_T;
        K = (T - ql) * (2 * T * T + 2 * ql * T - 3 * ql * ql);
    } else {
        const long long u = (long long)q - BC_T, v = 2ll * BC_T - (long long)q;
        K = -u * (v * v);
    }
    return (int)((K + 32768) >> 16);
}

// R = floor((C 2^14 + floor(S / 2)) / S), S > 0, |C| 2^14 < 2^62: an exact 64-bit division, rounded down below zero too
ZJ_HD int bc_R(const long long Cp, const long long S)
{
    const long long num = Cp * 16384 + (S >> 1);
    long long q = num / S;
    if (num - q * S < 0) q--;
    return (int)q;
}

// ---- the workgroup ---------------------------------------------------------------------------------------------------------
// (image, AA_ROWS output rows from r0, AA_COLS output columns from x0), as zj_resize_aa.h's.  A cubic's prefix sums C_j
// have no closed form and S is needed before the first weight, so the lanes share both: the AA_NT lanes are dealt out
// evenly over the set's outputs (`lpc` lanes each), each lane takes a contiguous share of its output's window of taps.
//   sum      every lane: the sum of K' over its share, into part[]
//   S        (once, the window being all taps) one lane per output: S = the sum of its lanes' parts
//   weights  every lane: its prefix = the output's carry + the parts of the lanes before it; then tap by tap
//            C += K', R, w = R - R_before into the table
//   carry    one lane per output: carry += the parts (the prefix at the end of the window, for the next window)
// Integer sums throughout: how the taps are dealt out changes no bit.
// The block's source columns are walked in pieces of bc_piece_w() pixels (the columns' windows); per piece the source rows
// are walked BC_RCH taps of every output row at a time (the rows' windows), the lanes summing w x byte over them; then
// t = (sum + 32) >> 6 into LDS as int32 and the horizontal pass adds w x t to 64-bit sums that live across the pieces.
template <int K>
struct BcSet {
    long long S[K], carry[K];
    BcAxis ax[K];
    int a[K], cnt[K], off[K + 1]; // the window [a, a + cnt) of each output and its weights' offset in the table
};

struct BcShared {
    int t[AA_ROWS][BC_TROW];
    long long cpart[AA_NT], rpart[AA_NT];
    BcSet<AA_COLS> col;
    BcSet<AA_ROWS> row;
    int16_t cw[BC_WCAP];
    int16_t rw[AA_ROWS * BC_RCH];
};

struct BcLane {
    int v[AA_ROWS][BC_WORD];        // vertical sums of the lane's 4 bytes, per output row: |sum| <= 255 x sum |w| < 2^23
    long long h[AA_GROUP * 3];      // horizontal sums: pixel g, channel c at g * C + c
};

// the lane's output k of nk and its share [j0, j1) of that output's window; false: the lane has none
template <int K>
ZJ_HD bool bc_share(const BcSet<K>& s, const int nk, const int tid, int& k, int& sub, int& lpc, int& j0, int& j1)
{
    lpc = AA_NT / nk;
    k = tid / lpc;
    sub = tid - k * lpc;
    if (k >= nk) return false;
    const int cnt = s.cnt[k], chunk = (cnt + lpc - 1) / lpc;
    j0 = sub * chunk < cnt ? sub * chunk : cnt;
    j1 = j0 + chunk < cnt ? j0 + chunk : cnt;
    j0 += s.a[k]; j1 += s.a[k];
    return true;
}

template <int K>
ZJ_HD void bc_sum_phase(const BcSet<K>& s, long long* part, const int nk, const int tid)
{
    int k, sub, lpc, j0, j1;
    long long sum = 0;
    if (bc_share(s, nk, tid, k, sub, lpc, j0, j1))
        for (int j = j0; j < j1; j++) sum += bc_K(s.ax[k], j);
    part[tid] = sum;
}

ZJ_HD long long bc_parts(const long long* part, const int first, const int n)
{
    long long sum = 0;
    for (int q = 0; q < n; q++) sum += part[first + q];
    return sum;
}

template <int K>
ZJ_HD void bc_S_phase(BcSet<K>& s, const long long* part, const int nk, const int tid)
{
    if (tid < nk) {
        const int lpc = AA_NT / nk;
        s.S[tid] = bc_parts(part, tid * lpc, lpc);
        s.carry[tid] = 0;
    }
}

template <int K>
ZJ_HD void bc_carry_phase(BcSet<K>& s, const long long* part, const int nk, const int tid)
{
    if (tid < nk) {
        const int lpc = AA_NT / nk;
        s.carry[tid] += bc_parts(part, tid * lpc, lpc);
    }
}

template <int K>
ZJ_HD void bc_weights_phase(const BcSet<K>& s, const long long* part, int16_t* w, const int nk, const int tid)
{
    int k, sub, lpc, j0, j1;
    if (!bc_share(s, nk, tid, k, sub, lpc, j0, j1) || j0 >= j1) return;
    const long long S = s.S[k];
    long long Cp = s.carry[k] + bc_parts(part, k * lpc, sub);
    int R0 = bc_R(Cp, S);
    int16_t* const wk = w + s.off[k] - s.a[k];
    for (int j = j0; j < j1; j++) {
        Cp += bc_K(s.ax[k], j);
        const int R1 = bc_R(Cp, S);
        wk[j] = (int16_t)(R1 - R0); // |w| < 2^15
        R0 = R1;
    }
}

// the whole tap range of every output as its window: what S is summed over
template <int K>
ZJ_HD void bc_all_taps_phase(BcSet<K>& s, const int nk, const int tid)
{
    if (tid < nk) {
        s.a[tid] = s.ax[tid].lo;
        s.cnt[tid] = s.ax[tid].hi - s.ax[tid].lo + 1;
    }
}

ZJ_HD void bc_axes_phase(const AaBlock& b, BcShared& s, const int tid)
{
    if (tid < b.ncols) s.col.ax[tid] = bc_axis(aa_dest_col(b, tid), (uint32_t)b.n_w, (uint32_t)b.ow);
    if (tid < b.nrows) s.row.ax[tid] = bc_axis((uint32_t)(b.r0 + tid), (uint32_t)b.n_h, (uint32_t)b.oh);
    bc_all_taps_phase(s.col, b.ncols, tid);
    bc_all_taps_phase(s.row, b.nrows, tid);
}

// the block's source columns: from the first tap of its lowest destination index to the last of its highest
ZJ_HD void bc_span(const AaBlock& b, const BcShared& s, int& sx0, int& sx1)
{
    sx0 = s.col.ax[b.flip ? b.ncols - 1 : 0].lo;
    sx1 = s.col.ax[b.flip ? 0 : b.ncols - 1].hi;
}

// the most taps of any of the block's rows
ZJ_HD int bc_row_taps(const AaBlock& b, const BcShared& s)
{
    int n = 0;
    for (int k = 0; k < b.nrows; k++) {
        const int c = s.row.ax[k].hi - s.row.ax[k].lo + 1;
        n = c > n ? c : n;
    }
    return n;
}

// The columns' windows: their taps within the piece [px0, px1).  A downscale puts every source pixel under at most four
// output columns (2i + 1 lies in an open interval of length 8), an upscale gives every output column at most four taps: at
// most 4 (piece + AA_COLS) entries, BC_WCAP.  The rows' carries start over with every piece.
ZJ_HD void bc_col_window_phase(const AaBlock& b, BcShared& s, const int px0, const int px1, const int tid)
{
    if (tid < b.ncols) {
        const BcAxis& a = s.col.ax[tid];
        const int lo = a.lo > px0 ? a.lo : px0, hi = a.hi < px1 - 1 ? a.hi : px1 - 1;
        s.col.a[tid] = lo;
        s.col.cnt[tid] = hi >= lo ? hi - lo + 1 : 0;
    }
    if (tid < b.nrows) s.row.carry[tid] = 0;
}

ZJ_HD void bc_col_offset_phase(const AaBlock& b, BcShared& s, const int tid)
{
    if (tid <= b.ncols) {
        int o = 0;
        for (int k = 0; k < tid; k++) o += s.col.cnt[k];
        s.col.off[tid] = o;
    }
}

// The rows' windows: taps [lo + j0, lo + j0 + BC_RCH) of every row; the window before it (j0 > 0) goes into the carry first
ZJ_HD void bc_row_window_phase(const AaBlock& b, BcShared& s, const int j0, const int tid)
{
    if (j0 > 0) bc_carry_phase(s.row, s.rpart, b.nrows, tid);
    if (tid < b.nrows) {
        const BcAxis& a = s.row.ax[tid];
        const int left = a.hi - a.lo + 1 - j0;
        s.row.a[tid] = a.lo + j0;
        s.row.cnt[tid] = left < 0 ? 0 : (left < BC_RCH ? left : BC_RCH);
        s.row.off[tid] = tid * BC_RCH;
    }
}

// The lane's 4 bytes of the piece: HWC one segment of C (px1 - px0) bytes, lanes 0..255; CHW one segment per plane of
// px1 - px0 bytes, 85 lanes per plane.  seg < 0: the lane has none.
template <bool IN_CHW, int C>
ZJ_HD void bc_lane_seg(const int tid, const int px0, const int px1, int& seg, long long& off, int& len, int& q0)
{
    const int w = IN_CHW ? tid % BC_PLANE_WORDS : tid;
    seg = IN_CHW ? tid / BC_PLANE_WORDS : 0;
    len = IN_CHW ? px1 - px0 : (px1 - px0) * C;
    q0 = BC_WORD * w;
    if (seg >= (IN_CHW ? 3 : 1) || q0 >= len) seg = -1;
    off = IN_CHW ? px0 : (long long)px0 * C;
}

// 4 bytes at a (any alignment) of a segment whose last byte is at `last`: two dword loads, the 2nd only where it starts at
// or before that byte (a dword that holds a byte of the segment never crosses the end of the allocation)
ZJ_HD uint32_t bc_load4(const uint8_t* a, const uint8_t* last)
{
    const uintptr_t ua = (uintptr_t)a;
    const uint8_t* ab = (const uint8_t*)(ua & ~(uintptr_t)3);
    const uint32_t sh = 8u * (uint32_t)(ua & 3u);
#if defined(ZJ_EMU)
    uint32_t d0, d1 = 0;
    memcpy(&d0, ab, 4);
    if (ab + 4 <= last) memcpy(&d1, ab + 4, 4);
#else
    const uint32_t* const g = ZJ_RZ_GLOBAL(const uint32_t, ab);
    const uint32_t d0 = g[0];
    const uint32_t d1 = ab + 4 <= last ? g[1] : 0u;
#endif
    return (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
}

// the window's taps of output row rr: the lane's 4 bytes of each source row times the row's signed weight, added to v
// (the lane's sums of that row: the caller's loop over the rows is unrolled, so they stay in registers)
template <bool IN_CHW, int C>
ZJ_HD void bc_vertical_phase(const AaBlock& b, const BcShared& s, int (&v)[BC_WORD], const int rr, const int px0,
                             const int px1, const int tid)
{
    int seg, len, q0;
    long long off;
    bc_lane_seg<IN_CHW, C>(tid, px0, px1, seg, off, len, q0);
    if (seg < 0) return;
    const uint8_t* const base = b.src + (long long)seg * b.plane + off;
    const int16_t* const rw = s.rw + s.row.off[rr];
    const int a = s.row.a[rr], nt = s.row.cnt[rr];
#pragma unroll 4
    for (int k = 0; k < nt; k++) {
        const int w = rw[k];
        const uint8_t* const row = base + (long long)(a + k) * b.pitch;
        const uint32_t x = bc_load4(row + q0, row + len - 1);
#pragma unroll
        for (int q = 0; q < BC_WORD; q++) v[q] += w * (int)((x >> (8 * q)) & 255u);
    }
}

// the rows' vertical sums rounded, t = (sum + 32) >> 6 (signed, not clamped), for the lane's bytes of its segment; sums
// cleared
template <bool IN_CHW, int C>
ZJ_HD void bc_vertical_store(const AaBlock& b, BcShared& s, BcLane& l, const int px0, const int px1, const int tid)
{
    int seg, len, q0;
    long long off;
    bc_lane_seg<IN_CHW, C>(tid, px0, px1, seg, off, len, q0);
#pragma unroll
    for (int rr = 0; rr < AA_ROWS; rr++) {
        if (seg >= 0 && rr < b.nrows) {
            int* const t = s.t[rr] + (IN_CHW ? seg * BC_PLANE_T : 0);
#pragma unroll
            for (int q = 0; q < BC_WORD; q++)
                if (q0 + q < len) t[q0 + q] = (l.v[rr][q] + 32) >> 6;
        }
#pragma unroll
        for (int q = 0; q < BC_WORD; q++) l.v[rr][q] = 0;
    }
}

// |sum| <= sum |w| x max |t| < 2^15 x 2^17: 64-bit sums (one v_mad_i64_i32 per product)
template <bool IN_CHW, int C>
ZJ_HD void bc_horizontal_phase(const AaBlock& b, const BcShared& s, BcLane& l, const int px0, const int tid)
{
    int rr, k0;
    const int cnt = aa_item(b, tid, rr, k0);
    if (cnt < 0) return;
    const int* const t = s.t[rr];
#pragma unroll
    for (int g = 0; g < AA_GROUP; g++) {
        if (g >= cnt) continue;
        const int k = k0 + g, n = s.col.cnt[k], o = s.col.off[k], a = s.col.a[k] - px0;
        for (int q = 0; q < n; q++) {
            const int w = s.cw[o + q];
#pragma unroll
            for (int c = 0; c < C; c++)
                l.h[g * C + c] += (long long)w * (long long)t[IN_CHW ? c * BC_PLANE_T + a + q : (a + q) * C + c];
        }
    }
}

// v = (sum + 32) >> 6 clamped to [0, 255 x 2^16], then aa_store_phase's conversion and store: that takes a sum whose
// (sum + 32) >> 6 is v, and v << 6 is one (below 2^30)
template <int C, int DT, bool NHWC>
ZJ_HD void bc_store_phase(const ResizeParams& p, const AaBlock& b, const BcLane& l, uint8_t* img_out, const int tid)
{
    AaLane a;
#pragma unroll
    for (int q = 0; q < AA_GROUP * 3; q++) {
        long long v = (l.h[q] + 32) >> 6;
        v = v < 0 ? 0 : (v > (255ll << 16) ? (255ll << 16) : v);
        a.h[q] = (uint32_t)v << 6;
    }
    aa_store_phase<C, DT, NHWC>(p, b, a, img_out, tid);
}

} // namespace zj
