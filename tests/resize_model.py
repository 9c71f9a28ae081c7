"""numpy model of the resized crop output, written from the definition alone.  TEST ONLY.

Taps, one axis (source length n, destination length m, 64-bit integers):
    u = floor((2i + 1) n 256 / (2m)) - 128, clamped to [0, (n - 1) 256];  i0 = u >> 8, f = u & 255, i1 = min(i0 + 1, n - 1)
Value: top = p[y0][x0] (256 - fx) + p[y0][x1] fx, bot likewise on y1, v = top (256 - fy) + bot fy.
Output: float32 fl32(fl32(v * s) + b) with s = scale * 2^-16; f16 / bf16 its nearest-even rounding; u8 (v + 32768) >> 16.
"""
import numpy as np

F32, F16, BF16, U8 = 0, 1, 2, 3


def taps(n, m):
    i = np.arange(m, dtype=np.int64)
    u = ((2 * i + 1) * n * 256) // (2 * m) - 128
    u = np.clip(u, 0, (n - 1) * 256)
    i0 = u >> 8
    return i0, u & 255, np.minimum(i0 + 1, n - 1)


def factors(channels, scale=None, bias=None):
    s = np.float32(np.ones(channels) if scale is None else np.asarray(scale, np.float32)) * np.float32(1.0 / 65536)
    b = np.float32(np.zeros(channels) if bias is None else np.asarray(bias, np.float32))
    return np.asarray(s, np.float32).reshape(channels), np.asarray(b, np.float32).reshape(channels)


def bf16_bits(y):
    u = np.asarray(y, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def values(img_chw, out_w, out_h, flip=False):
    """img_chw: [C, h, w] uint8 -> v [C, out_h, out_w] int64 (the value in 1/65536 units)"""
    c, h, w = img_chw.shape
    x0, fx, x1 = taps(w, out_w)
    y0, fy, y1 = taps(h, out_h)
    if flip:
        x0, fx, x1 = x0[::-1], fx[::-1], x1[::-1]
    r0, r1 = img_chw[:, y0, :], img_chw[:, y1, :]  # (the rows and columns the taps read, before widening)
    q = lambda r, x: r[:, :, x].astype(np.int64)
    top = q(r0, x0) * (256 - fx) + q(r0, x1) * fx
    bot = q(r1, x0) * (256 - fx) + q(r1, x1) * fx
    return top * (256 - fy)[None, :, None] + bot * fy[None, :, None]


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
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if layout == "NHWC" else out


def raw_view(buf, dtype):
    """the bytes of an output as the model's arrays"""
    return buf.view({F32: np.float32, F16: np.uint16, BF16: np.uint16, U8: np.uint8}[dtype])


def chw_of(crop, channels, chw):
    """a u8 crop in its own layout (HWC rows of w * C bytes, or 3 planes) -> [C, h, w]"""
    if channels == 1:
        return crop.reshape(1, *crop.shape[-2:]) if crop.ndim >= 2 else crop
    return crop if chw else crop.transpose(2, 0, 1)
