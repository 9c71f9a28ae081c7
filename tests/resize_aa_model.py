"""numpy model of the antialiased resized output (ZJ_RESIZE_BILINEAR_AA), written from the definition alone.
TEST ONLY.

One axis, source length n, destination length m (64-bit integers): output i has its centre at c = (2i + 1) n and source
pixel j at (2j + 1) m, both in units of 1/(2m) source pixels; D = 2 max(n, m).
    W_j = max(0, D - |(2j + 1) m - c|) for j in [0, n);  S = sum of W_j;  C_j = W_0 + ... + W_j
    R_j = floor((C_j 2^14 + floor(S / 2)) / S);  w_j = R_j - R_{j-1} (R_{-1} = 0): non-negative, summing to 2^14
Vertical pass first: t = (sum_j w_j p[j][x] + 32) >> 6; then horizontal: v = (sum_k w_k t[k] + 32) >> 6 (0 .. 255 x 2^16).
Output: as tests/resize_model.py from v: float32 fl32(fl32(v * s) + b), f16 / bf16 its nearest-even rounding, u8
(v + 32768) >> 16; flip mirrors the output columns.
"""
import numpy as np

from resize_model import BF16, F16, F32, U8, bf16_bits, factors  # noqa: F401

P = 14


def taps(n, m):
    """one axis -> (j, w), both [m, T] int64: output i reads source j[i, k] with weight w[i, k].  The candidates are a
    window of every j within D / (2m) + 2 pixels of the centre (a superset of W_j > 0); entries outside [0, n) weigh 0."""
    i = np.arange(m, dtype=np.int64)
    c = (2 * i + 1) * n
    D = 2 * max(n, m)
    K = D // (2 * m) + 2
    j = (c // (2 * m))[:, None] + np.arange(-K, K + 1, dtype=np.int64)[None, :]
    W = np.maximum(D - np.abs((2 * j + 1) * m - c[:, None]), 0)
    W[(j < 0) | (j >= n)] = 0
    Cs = np.cumsum(W, axis=1)
    S = Cs[:, -1:]
    R = (Cs * (1 << P) + S // 2) // S
    w = np.diff(R, axis=1, prepend=0)
    return np.clip(j, 0, n - 1), w


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


def values(img_chw, out_w, out_h, flip=False):
    """img_chw: [C, h, w] uint8 -> v [C, out_h, out_w] int64 (the value in 1/65536 units)"""
    _, h, w = img_chw.shape
    jy, wy = taps(h, out_h)
    t = (_apply(img_chw.astype(np.int64), jy, wy, 1) + 32) >> 6
    jx, wx = taps(w, out_w)
    v = (_apply(t, jx, wx, 2) + 32) >> 6
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
