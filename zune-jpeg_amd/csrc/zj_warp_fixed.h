// zj_warp_fixed.h -- the host-side rules of the affine warp: a matrix of doubles as the six integers the
// kernel takes, and the window of the source a warped output can see.  Nothing of HIP here, and no kernel file includes
// it: zj_api.cpp's entry points (zj_warp_fixed, zj_warp_source_window) and tests/emu_warp call the same functions.
#pragma once

#include <math.h>
#include <stdint.h>

namespace zj {

constexpr int WARP_FIXED_Q = 24;

// floor(x * 2^24 + 1/2) as an integer; x finite and |x| < 2^38 (the scaling is exact, the sum and the floor are double's)
inline int64_t warp_round_q(const double x) { return (int64_t)floor(ldexp(x, WARP_FIXED_Q) + 0.5); }

// m = (a, b, c, d, e, f), output pixel CENTRE -> source coordinates: sx = a (X + 1/2) + b (Y + 1/2) + c.  The integers take
// the pixel INDEX to the first tap's position: Ux = A X + B Y + C0 with C0 = round((a / 2 + b / 2 + c - 1/2) 2^24), the sum
// formed in doubles from left to right.  false: a non-finite entry, |a|, |b|, |d|, |e| >= 128 or |c|, |f| >= 2^31.
inline bool warp_fixed(const double m[6], int64_t q[6])
{
    for (int k = 0; k < 6; k++) {
        if (!(m[k] - m[k] == 0.0)) return false;
        if (!(fabs(m[k]) < (k % 3 == 2 ? 2147483648.0 : 128.0))) return false;
    }
    q[0] = warp_round_q(m[0]); q[1] = warp_round_q(m[1]);
    q[2] = warp_round_q(((m[0] * 0.5 + m[1] * 0.5) + m[2]) - 0.5);
    q[3] = warp_round_q(m[3]); q[4] = warp_round_q(m[4]);
    q[5] = warp_round_q(((m[3] * 0.5 + m[4] * 0.5) + m[5]) - 0.5);
    return true;
}

// are these the integers of some matrix warp_fixed accepts (what the window and the kernel's 64-bit sums rely on)
inline bool warp_ints_valid(const int64_t q[6])
{
    const int64_t lin = (int64_t)1 << 31, off = ((int64_t)1 << 55) + ((int64_t)1 << 32);
    for (int k = 0; k < 6; k++) {
        const int64_t lim = k % 3 == 2 ? off : lin;
        if (q[k] > lim || q[k] < -lim) return false;
    }
    return true;
}

// the first tap's index of one axis at output pixel (X, Y): (A X + B Y + C0) >> 24, a floor
inline int64_t warp_tap0(const int64_t A, const int64_t B, const int64_t C0, const int64_t X, const int64_t Y)
{
    return (A * X + B * Y + C0) >> WARP_FIXED_Q;
}

// The window x, y, w, h of a frame of fw x fh that an out_w x out_h output under the integers q can read, and the integers
// relative to it.  U is affine, so the extremes of the first tap lie at the output's four corner pixels; the tap box is
// [min, max + 1] on each axis.  fill (edge 0): the box cut to the frame, an empty cut gives w = h = 0 (the output is all
// fill).  replicate (edge 1): both ends of the box clamped into the frame.  shifted = q with C0 - x 2^24, F0 - y 2^24.
inline void warp_source_window(const int64_t q[6], unsigned fw, unsigned fh, unsigned out_w, unsigned out_h, bool replicate,
                               unsigned win[4], int64_t shifted[6])
{
    const int64_t X1 = (int64_t)out_w - 1, Y1 = (int64_t)out_h - 1;
    int64_t lo[2], hi[2];
    for (int ax = 0; ax < 2; ax++) {
        const int64_t A = q[3 * ax], B = q[3 * ax + 1], C = q[3 * ax + 2];
        const int64_t t[4] = {warp_tap0(A, B, C, 0, 0), warp_tap0(A, B, C, X1, 0), warp_tap0(A, B, C, 0, Y1), warp_tap0(A, B, C, X1, Y1)};
        lo[ax] = hi[ax] = t[0];
        for (int k = 1; k < 4; k++) { if (t[k] < lo[ax]) lo[ax] = t[k]; if (t[k] > hi[ax]) hi[ax] = t[k]; }
        hi[ax] += 1;
        const int64_t n = ax == 0 ? (int64_t)fw : (int64_t)fh;
        if (replicate) {
            lo[ax] = lo[ax] < 0 ? 0 : (lo[ax] > n - 1 ? n - 1 : lo[ax]);
            hi[ax] = hi[ax] < 0 ? 0 : (hi[ax] > n - 1 ? n - 1 : hi[ax]);
        } else {
            if (lo[ax] < 0) lo[ax] = 0;
            if (hi[ax] > n - 1) hi[ax] = n - 1;
        }
    }
    for (int k = 0; k < 6; k++) shifted[k] = q[k];
    if (lo[0] > hi[0] || lo[1] > hi[1]) { // (fill alone: the box misses the frame)
        win[0] = win[1] = win[2] = win[3] = 0;
        return;
    }
    win[0] = (unsigned)lo[0]; win[1] = (unsigned)lo[1];
    win[2] = (unsigned)(hi[0] - lo[0] + 1); win[3] = (unsigned)(hi[1] - lo[1] + 1);
    shifted[2] = q[2] - lo[0] * ((int64_t)1 << WARP_FIXED_Q);
    shifted[5] = q[5] - lo[1] * ((int64_t)1 << WARP_FIXED_Q);
}

} // namespace zj
