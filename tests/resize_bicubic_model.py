"""numpy model of the bicubic antialiased resized output (ZJ_RESIZE_BICUBIC_AA), written from the definition
alone.  TEST ONLY.

One axis, source length n <= 65535, destination length m <= 8192 (64-bit integers): output i has its centre at
c = (2i + 1) n and source pixel j at (2j + 1) m, both in units of 1/(2m) source pixels; D = 2 max(n, m); d_j = |(2j + 1) m - c|.
    taps: the j in [0, n) with d_j < 2D
    q = floor(d_j 2^15 / D), T = 2^15 (0 <= q < 2T)
    K(q) = 3 q^3 - 5 q^2 T + 2 T^3 (q < T),  -q^3 + 5 q^2 T - 8 q T^2 + 4 T^3 (T <= q < 2T): Keys' cubic, a = -1/2, times 2 T^3
    K'_j = (K(q) + 2^15) >> 16;  S = sum of K'_j > 0;  C_j = K'_lo + ... + K'_j
    R_j = floor((C_j 2^14 + floor(S / 2)) / S) (floor division, also below zero);  w_j = R_j - R_{j-1} (R before the first tap: 0)
The weights sum to 2^14 and may be negative.  Vertical pass first: t = (sum_j w_j p[j][x] + 32) >> 6, signed, not clamped;
then horizontal: v = (sum_k w_k t[k] + 32) >> 6, clamped to [0, 255 x 2^16].
Output: as tests/resize_model.py from v: float32 fl32(fl32(v * s) + b), f16 / bf16 its nearest-even rounding, u8
(v + 32768) >> 16; flip mirrors the output columns.
"""
import numpy as np

from resize_model import BF16, F16, F32, U8, bf16_bits, factors  # noqa: F401

P = 14
T = 1 << 15
MAX_TAPS = 4 * 65535 + 1
ABS_W_MAX = 2 << P     # the stated bound on sum |w_j|; the ranges below follow from it
T_MAX = (255 * ABS_W_MAX + 32) >> 6            # |t| <= this
H_MAX = ABS_W_MAX * T_MAX                      # |sum_k w_k t[k]| <= this
V_MAX = 255 << 16


def kernel(q):
    """K(q) of an int64 array, 0 <= q < 2T"""
    q = q.astype(np.int64)
    near = 3 * q ** 3 - 5 * q ** 2 * T + 2 * T ** 3
    far = -q ** 3 + 5 * q ** 2 * T - 8 * q * T ** 2 + 4 * T ** 3
    return np.where(q < T, near, far)


def taps(n, m):
    """one axis -> (j, w, S), [m, N] int64 twice and [m] int64: output i reads source j[i, k] with weight w[i, k].  The
    candidates are a window of every j within 2D / (2m) + 2 pixels of the centre (a superset of d_j < 2D); entries outside
    the taps weigh 0."""
    assert 1 <= n <= 65535 and 1 <= m <= 8192
    i = np.arange(m, dtype=np.int64)
    c = (2 * i + 1) * n
    D = 2 * max(n, m)
    Kw = (2 * D) // (2 * m) + 2
    j = (c // (2 * m))[:, None] + np.arange(-Kw, Kw + 1, dtype=np.int64)[None, :]
    d = np.abs((2 * j + 1) * m - c[:, None])
    tap = (d < 2 * D) & (j >= 0) & (j < n)
    assert tap.sum(axis=1).max() <= MAX_TAPS
    q = np.where(tap, (d << 15) // D, 0)
    assert (q >= 0).all() and (q < 2 * T).all()
    Kp = np.where(tap, (kernel(q) + (1 << 15)) >> 16, 0)
    assert (np.abs(Kp) <= 1 << 30).all()
    Cs = np.cumsum(Kp, axis=1)
    S = Cs[:, -1:]
    assert (S > 0).all(), "S must be positive"
    assert np.abs(Cs).max() < 1 << (63 - P) and np.abs(Kp).sum(axis=1).max() < 1 << (63 - P)
    R = (Cs * (1 << P) + S // 2) // S
    w = np.diff(R, axis=1, prepend=0)
    assert np.abs(w).sum(axis=1).max() <= ABS_W_MAX and np.abs(w).max() < 1 << 15
    return np.clip(j, 0, n - 1), w, S[:, 0]


def _apply(src, j, w, axis):
    """sum_k w[i, k] src[..., j[i, k], ...] along `axis` (1: rows, 2: columns) of a [C, H, W] int64 array"""
    shape = list(src.shape)
    shape[axis] = j.shape[0]
    acc = np.zeros(shape, np.int64)
    for k in range(j.shape[1]):
        wk = w[:, k]
        if not wk.any():
            continue
        sel = np.take(src, j[:, k], axis=axis)
        acc += sel * (wk[None, :, None] if axis == 1 else wk[None, None, :])
    return acc


def passes(img_chw, out_w, out_h):
    """img_chw: [C, h, w] uint8 -> (t [C, out_h, w], the horizontal sums [C, out_h, out_w], v before the clamp), int64"""
    _, h, w = img_chw.shape
    jy, wy, _ = taps(h, out_h)
    t = (_apply(img_chw.astype(np.int64), jy, wy, 1) + 32) >> 6
    assert np.abs(t).max() <= T_MAX
    jx, wx, _ = taps(w, out_w)
    hs = _apply(t, jx, wx, 2)
    assert np.abs(hs).max() <= H_MAX
    return t, hs, (hs + 32) >> 6


def values(img_chw, out_w, out_h, flip=False):
    """img_chw: [C, h, w] uint8 -> v [C, out_h, out_w] int64 (the value in 1/65536 units, clamped to [0, 255 x 2^16])"""
    v = np.clip(passes(img_chw, out_w, out_h)[2], 0, V_MAX)
    return v[:, :, ::-1] if flip else v


def resize(img_chw, out_w, out_h, dtype, scale=None, bias=None, flip=False, layout="NCHW"):
    """one image [C, h, w] uint8 -> its output [C, out_h, out_w] (or [out_h, out_w, C] for NHWC): float32 values for F32,
    uint16 raw bits for F16 / BF16, uint8 for U8"""
    c = img_chw.shape[0]
    v = values(img_chw, out_w, out_h, flip)
    if dtype == U8:
        out = ((v + 32768) >> 16).astype(np.uint8)
    else:
        s, b = factors(c, scale, bias)
        y = (v.astype(np.float32) * s[:, None, None]).astype(np.float32)
        y = (y + b[:, None, None]).astype(np.float32)
        if dtype == F32:
            out = y
        elif dtype == F16:
            with np.errstate(over="ignore"):
                out = y.astype(np.float16).view(np.uint16)
        else:
            out = bf16_bits(y)
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if layout == "NHWC" else np.ascontiguousarray(out)
