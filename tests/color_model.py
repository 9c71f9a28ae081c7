"""The colour-matrix stage in numpy: the definition the kernel, its CPU emulation and the pipeline calls are
compared with, byte for byte.  TEST ONLY.

A matrix is 12 doubles, m[c][0..2] multiply R, G, B and m[c][3] is an offset in grey levels.
    q[c][k] = floor(m[c][k] * 65536 + 1/2)                         (in doubles)
    v       = q[c][0] R + q[c][1] G + q[c][2] B + q[c][3]          (|v| < 2^31)
    out[c]  = clamp((v + 32768) >> 16, 0, 255)                     (arithmetic shift)
"""
import numpy as np

LIN_MAX, OFF_MAX = 16.0, 4096.0
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64)
BGR = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0]], np.float64)
LUMA = (0.299, 0.587, 0.114)
GRAY = np.array([[*LUMA, 0]] * 3, np.float64)
NEGATIVE = np.array([[-1, 0, 0, 255], [0, -1, 0, 255], [0, 0, -1, 255]], np.float64)


def fixed(m):
    """the 12 integers of a matrix ([3, 4] or 12 numbers), or None: a matrix the stage refuses"""
    m = np.asarray(m, np.float64).reshape(12)
    lim = np.array([LIN_MAX, LIN_MAX, LIN_MAX, OFF_MAX] * 3)
    if not np.all(np.isfinite(m)) or np.any(np.abs(m) > lim):
        return None
    return [int(v) for v in np.floor(m * 65536.0 + 0.5)]


def apply_fixed(q, img, chw=False):
    """the stage on a u8 image, [H, W, 3] (chw: [3, H, W]), under the 12 integers q"""
    q = np.asarray(q, np.int64).reshape(3, 4)
    x = np.asarray(img).astype(np.int64)
    r, g, b = (x[0], x[1], x[2]) if chw else (x[..., 0], x[..., 1], x[..., 2])
    out = []
    for c in range(3):
        v = q[c, 0] * r + q[c, 1] * g + q[c, 2] * b + q[c, 3]
        assert np.abs(v).max(initial=0) < 2 ** 31 - 32768
        out.append(np.clip((v + 32768) >> 16, 0, 255).astype(np.uint8))
    return np.stack(out, axis=0 if chw else -1)


def apply(m, img, chw=False):
    q = fixed(m)
    assert q is not None, "a matrix the stage refuses"
    return apply_fixed(q, img, chw)


def affine_f64(m, img):
    """clip(floor(m . (R, G, B, 1) + 1/2)) in float64: what the integers approximate, [H, W, 3] only"""
    m = np.asarray(m, np.float64).reshape(3, 4)
    x = np.asarray(img).astype(np.float64)
    return np.clip(np.floor(x @ m[:, :3].T + m[:, 3] + 0.5), 0, 255).astype(np.uint8)


def noise_image(seed=5):
    """the 64 x 96 image of the Pillow comparisons: noise with an 8-row gray ramp at the bottom"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    ramp = np.linspace(0, 255, 96).astype(np.uint8)
    img[56:] = ramp[None, :, None]
    return img
