"""The definition of the reduced-size decode in numpy: scale s = 2, 4, 8 (scale_log2 = 1, 2, 3).

Per component and axis a block yields N = min(8, (8 / s) * (f_max / f_c)) samples; with r = 8 / N a sample is the mean
of r consecutive outputs of the exact 8-point IDCT of the dequantised block (+ 128), in two dimensions the mean of an
r_x x r_y rectangle, taken BEFORE rounding and clamping.  Per axis that mean is a linear map of the 8 coefficients,

    A_N[m][k] = C_k / 2 * mean_{j < r} cos((2 (r m + j) + 1) k pi / 16),      C_0 = 1 / sqrt 2, C_k = 1

(`float_matrix`).  Averaging pairs is the "fold": out[n] = (x[2n] + x[2n+1]) / 2 = sum_k C_k/2 cos(k pi/16) X_k
cos((2n+1) k pi/8), a 4-point transform in which k = 4 drops out (cos((2n+1) pi/2) = 0) and k = 5, 6, 7 land on the
basis functions of 3, 2, 1 with a sign (cos((2n+1)(8-k) pi/8) = -cos((2n+1) k pi/8)): in A_4 the columns 5, 6, 7 are
multiples of the columns 3, 2, 1, column 4 is zero; folding again, A_2 keeps column 0 and the odd ones, A_1 column 0.
The integer form keeps the map as the matrix it is, with the even/odd symmetry A_N[N-1-m][k] = (-1)^k A_N[m][k]:

    K_N[m][k] = round(2^13 A_N[m][k])                                              (`int_matrix`)
    pass 1 (columns, N_y outputs each):  t = (sum_k s[k][col] K_Ny[m][k] + 512) >> 10        s = coefficient x q
    pass 2 (rows, N_x outputs each):     v = (sum_k t[m][k] K_Nx[n][k] + 32768 + (128 << 16)) >> 16, clamped to 0..255
    N_x = N_y = 1:                        v = ((s[0][0] + 4) >> 3) + 128, clamped            (exactly DC q / 8 + 128, rounded)

in int32 with two's-complement wrap-around (every operand of a product fits 24 bits: |s| < 2^23, |t| < 2^21, so the
kernel's 24-bit multiplies give the same low 32 bits).  A component with N = 8 on both axes (chroma of 4:2:0 at 1/2) is
NOT reduced: its samples are the full path's (oracle_np.idct_blocks: the reference's butterfly, its DC-only shortcut Q1,
ZJ_FLAG_CLAMP_DC).  Colour is the full path's per-pixel arithmetic, placement is plain.
"""
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(_ROOT, "oracle"))
import oracle_np as onp  # noqa: E402

RGB, GRAYSCALE, YCBCR = 0, 1, 2  # ZJ_CS_*


def float_matrix(n):
    """A_N as float64 [N][8]"""
    r = 8 // n
    a = np.zeros((n, 8))
    for m in range(n):
        for k in range(8):
            ck = 1 / math.sqrt(2) if k == 0 else 1.0
            a[m, k] = ck / 2 * np.mean([math.cos((2 * (r * m + j) + 1) * k * math.pi / 16) for j in range(r)])
    return a


def int_matrix(n):
    """K_N as int32 [N][8]; rows m >= N/2 by the symmetry, as the kernel forms them"""
    a = float_matrix(n)
    k = np.zeros((n, 8), np.int64)
    half = max(n // 2, 1)
    for m in range(half):
        k[m] = np.round(a[m] * 8192).astype(np.int64)
        k[m][np.abs(a[m]) < 1e-12] = 0
    for m in range(half, n):
        k[m] = k[n - 1 - m] * np.array([1, -1] * 4)
    return k.astype(np.int32)


def samples_per_block(scale_log2, f_max, f_c):
    return min(8, (8 >> scale_log2) * (f_max // f_c))


def float_samples(deq, nx, ny):
    """the definition in float64: deq (n, 8, 8) dequantised coefficients [vertical k][horizontal k] -> (n, ny, nx),
    before rounding and clamping"""
    ay, ax = float_matrix(ny), float_matrix(nx)
    return np.einsum("mk,nkl,pl->nmp", ay, np.asarray(deq, np.float64), ax) + 128.0


def float_rounded(deq, nx, ny):
    return np.clip(np.floor(float_samples(deq, nx, ny) + 0.5), 0, 255).astype(np.int32)


def _w32(v):
    """int64 -> the int32 it wraps to, kept as int64"""
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _mat32(x, k, axis_bias):
    """sum_k x[..., k] * K[m][k] + bias, every product and sum wrapped to int32; x int64 (..., 8) -> (..., N)"""
    acc = np.full(x.shape[:-1] + (k.shape[0],), axis_bias, np.int64)
    for kk in range(8):
        acc = _w32(acc + _w32(x[..., kk, None] * k[None, :, kk].astype(np.int64)))
    return acc


def int_samples(blocks, qt, nx, ny):
    """the integer definition: blocks (n, 64) int16 natural order, qt (64,) 0..255 -> (n, ny, nx) int16 in 0..255"""
    blocks = np.ascontiguousarray(blocks, np.int16).reshape(-1, 64)
    qt = np.asarray(qt, np.int64).reshape(64)
    s = (blocks.astype(np.int64) * qt[None, :]).reshape(-1, 8, 8)  # [k vertical][column], |s| < 2^23
    if nx == 1 and ny == 1:
        return np.clip(((s[:, 0, 0] + 4) >> 3) + 128, 0, 255).astype(np.int16).reshape(-1, 1, 1)
    ky, kx = int_matrix(ny), int_matrix(nx)
    t = _mat32(np.swapaxes(s, 1, 2), ky, 512) >> 10              # (n, column, m)
    t = np.swapaxes(t, 1, 2)                                      # (n, m, column = horizontal k)
    v = _mat32(t, kx, 32768 + (128 << 16)) >> 16                  # (n, m, x)
    return np.clip(v, 0, 255).astype(np.int16)


def component_samples(blocks, qt, nx, ny, clamp_dc=False):
    """a component's blocks -> (n, ny, nx) int16: the reduced samples, or (8 x 8) the full path's"""
    if nx == 8 and ny == 8:
        blocks = np.ascontiguousarray(blocks, np.int16).reshape(-1, 64)
        px = onp.idct_blocks(blocks, qt)
        if clamp_dc:
            dc_only = ~np.any(blocks[:, 1:] != 0, axis=1)
            px[dc_only] = np.clip(px[dc_only], 0, 255)
        return px
    return int_samples(blocks, qt, nx, ny)


def scaled_size(width, height, scale_log2):
    s = 1 << scale_log2
    return (width + s - 1) // s, (height + s - 1) // s


def component_plane(plane, qt, bw, bh, nx, ny, clamp_dc=False):
    """a coefficient plane of bh x bw blocks (block raster) -> its (bh * ny, bw * nx) int16 sample plane"""
    px = component_samples(np.asarray(plane, np.int16)[: bw * bh * 64].reshape(-1, 64), qt, nx, ny, clamp_dc)
    return px.reshape(bh, bw, ny, nx).transpose(0, 2, 1, 3).reshape(bh * ny, bw * nx)


def decode_scaled_ycc(width, height, hs, vs, in_components, qts, planes, scale_log2, clamp_dc=False):
    """the reduced frame's sample planes [Y] or [Y, Cb, Cr], each (rh, rw) int16"""
    rw, rh = scaled_size(width, height, scale_log2)
    mcu_x, mcu_y = (width + 8 * hs - 1) // (8 * hs), (height + 8 * vs - 1) // (8 * vs)
    ln = 8 >> scale_log2
    out = [component_plane(planes[0], qts[0], mcu_x * hs, mcu_y * vs, ln, ln, clamp_dc)[:rh, :rw]]
    if in_components == 3:
        nx, ny = samples_per_block(scale_log2, hs, 1), samples_per_block(scale_log2, vs, 1)
        for c in (1, 2):
            out.append(component_plane(planes[c], qts[min(c, len(qts) - 1)], mcu_x, mcu_y, nx, ny, clamp_dc)[:rh, :rw])
    return out


def decode_scaled(width, height, hs, vs, in_components, out_cs, qts, planes, scale_log2, chw=False, clamp_dc=False):
    """the whole reduced frame: (rh, rw, C) uint8, C = 3 (RGB, YCbCr) or 1 (GRAYSCALE); chw: (C, rh, rw).  A
    single-component frame with a colour output is all zeros (zj_crop_out_len's rule)."""
    rw, rh = scaled_size(width, height, scale_log2)
    nc = 1 if out_cs == GRAYSCALE else 3
    if in_components == 1 and out_cs != GRAYSCALE:
        img = np.zeros((rh, rw, nc), np.uint8)
    else:
        ycc = decode_scaled_ycc(width, height, hs, vs, in_components, qts, planes, scale_log2, clamp_dc)
        low = lambda a: a.astype(np.uint16).astype(np.uint8)
        if out_cs == GRAYSCALE:
            img = low(ycc[0])[:, :, None]
        elif out_cs == YCBCR:
            img = np.stack([low(c) for c in ycc], axis=-1)
        else:
            img = onp.ycbcr_to_rgb_px(ycc[0], ycc[1], ycc[2])
    return np.ascontiguousarray(img.transpose(2, 0, 1)) if chw and nc == 3 else img


def crop(img, x, y, w, h, chw=False):
    return np.ascontiguousarray(img[:, y:y + h, x:x + w] if (chw and img.ndim == 3 and img.shape[0] == 3 and img.shape[2] != 3)
                                else img[y:y + h, x:x + w])


# ---- the prescaled resized crop's plan (include/zjhip.h: zj_decode_crops_resized_prescaled_device) ------
def prescale_log2(w, h, out_w, out_h, max_prescale_log2):
    """the largest k <= max_prescale_log2 with floor(w / 2^k) >= out_w and floor(h / 2^k) >= out_h (0 if none)"""
    k = 0
    for c in range(1, max_prescale_log2 + 1):
        if (w >> c) >= out_w and (h >> c) >= out_h:
            k = c
    return k


def reduced_window(x, y, w, h, k, width, height):
    """[floor(x / s), ceil((x + w) / s)) x [floor(y / s), ceil((y + h) / s)), clipped to the reduced frame: x, y, w, h"""
    s = 1 << k
    rw, rh = scaled_size(width, height, k)
    x0, y0 = x // s, y // s
    x1, y1 = min((x + w + s - 1) // s, rw), min((y + h + s - 1) // s, rh)
    return x0, y0, x1 - x0, y1 - y0
