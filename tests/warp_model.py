"""numpy model of the affine warp, written from the definition alone.  TEST ONLY.

Matrix m = (a, b, c, d, e, f) of doubles: output pixel centre -> source coordinates, sx = a (X + 1/2) + b (Y + 1/2) + c.
Fixed point, Q = 24: A = floor(a 2^24 + 1/2) (B, D, E likewise), C0 = floor((a / 2 + b / 2 + c - 1/2) 2^24 + 1/2) (F0
likewise), the sums formed in doubles from left to right.  Position, 64-bit integers: Ux = A X + B Y + C0, ux = Ux >> 16,
x0 = ux >> 8, fx = ux & 255.  Taps (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1): FILL reads fill[c] outside the
image, REPLICATE clamps the indices.  Value: resize_model's top / bot / v; output: resize_model's conversions.
"""
import math

import numpy as np

import resize_model as rm

Q = 24
FILL, REPLICATE = 0, 1


def round_q(x):
    return int(math.floor(x * 2.0 ** Q + 0.5))


def fixed(m):
    """the six integers (python ints), None: refused"""
    m = [float(v) for v in m]
    for k, v in enumerate(m):
        if not math.isfinite(v) or not abs(v) < (2.0 ** 31 if k % 3 == 2 else 128.0):
            return None
    a, b, c, d, e, f = m
    return [round_q(a), round_q(b), round_q(((a * 0.5 + b * 0.5) + c) - 0.5),
            round_q(d), round_q(e), round_q(((d * 0.5 + e * 0.5) + f) - 0.5)]


def positions(q, out_w, out_h):
    """x0, fx, y0, fy: [out_h, out_w] int64 each"""
    Y, X = np.meshgrid(np.arange(out_h, dtype=np.int64), np.arange(out_w, dtype=np.int64), indexing="ij")
    res = []
    for A, B, C0 in (q[:3], q[3:]):
        u = (A * X + B * Y + C0) >> 16
        res += [u >> 8, u & 255]
    return res


def values(img, q, out_w, out_h, edge=FILL, fill=None):
    """img: [h, w, C] uint8 -> v [C, out_h, out_w] int64 (the value in 1/65536 units)"""
    h, w, ch = img.shape
    fill = np.zeros(ch, np.int64) if fill is None else np.asarray(fill, np.int64)[:ch]
    x0, fx, y0, fy = positions(q, out_w, out_h)

    def tap(y, x):
        if edge == REPLICATE:
            return img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        px = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        return np.where(inside[..., None], px, fill[None, None, :])

    fx, fy = fx[..., None], fy[..., None]
    top = tap(y0, x0) * (256 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (256 - fx) + tap(y0 + 1, x0 + 1) * fx
    return (top * (256 - fy) + bot * fy).transpose(2, 0, 1)


def convert(v, dtype, scale=None, bias=None, layout="NCHW"):
    """v [C, oh, ow] -> the output as resize_model.resize gives it"""
    c = v.shape[0]
    if dtype == rm.U8:
        out = ((v + 32768) >> 16).astype(np.uint8)
    else:
        s, b = rm.factors(c, scale, bias)
        y = (v.astype(np.float32) * s[:, None, None]).astype(np.float32)
        y = (y + b[:, None, None]).astype(np.float32)
        if dtype == rm.F32:
            out = y
        elif dtype == rm.F16:
            with np.errstate(over="ignore"):
                out = y.astype(np.float16).view(np.uint16)
        else:
            out = rm.bf16_bits(y)
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if layout == "NHWC" else out


def warp(img, q, out_w, out_h, dtype, scale=None, bias=None, edge=FILL, fill=None, layout="NCHW"):
    return convert(values(img, q, out_w, out_h, edge, fill), dtype, scale, bias, layout)


def source_window(q, fw, fh, out_w, out_h, edge):
    """((x, y, w, h), shifted integers): the tap box over the output's four corner pixels, cut to (FILL) or clamped into
    (REPLICATE) the frame; FILL and no overlap: (0, 0, 0, 0)"""
    lo, hi = [], []
    for (A, B, C0), n in ((q[:3], fw), (q[3:], fh)):
        t = [(A * X + B * Y + C0) >> Q for X in (0, out_w - 1) for Y in (0, out_h - 1)]
        a, b = min(t), max(t) + 1
        if edge == REPLICATE:
            a, b = min(max(a, 0), n - 1), min(max(b, 0), n - 1)
        else:
            a, b = max(a, 0), min(b, n - 1)
        lo.append(a); hi.append(b)
    if lo[0] > hi[0] or lo[1] > hi[1]:
        return (0, 0, 0, 0), list(q)
    sh = list(q)
    sh[2] -= lo[0] << Q
    sh[5] -= lo[1] << Q
    return (lo[0], lo[1], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1), sh


def orientation_matrix(o, W, H):
    """the integer matrix of EXIF orientation o for a stored W x H image (displayed pixel centre -> stored coordinates)"""
    return {1: (1, 0, 0, 0, 1, 0), 2: (-1, 0, W, 0, 1, 0), 3: (-1, 0, W, 0, -1, H), 4: (1, 0, 0, 0, -1, H),
            5: (0, 1, 0, 1, 0, 0), 6: (0, 1, 0, -1, 0, H), 7: (0, -1, W, -1, 0, H), 8: (0, -1, W, 1, 0, 0)}[o]
