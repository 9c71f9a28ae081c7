"""The tone stage's definition in numpy and Python integers / doubles: the six tables, the histogram, the
whole op on an image.  tests/test_tone_model.py pins every table to Pillow's ImageOps; the emulation and the GPU tests compare
against this model, so they need no Pillow.  TEST ONLY."""
import numpy as np

IDENTITY, INVERT, POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE = range(6)
NEEDS_HIST = (AUTOCONTRAST, EQUALIZE)


def valid(op, param):
    if op == POSTERIZE:
        return 1 <= param <= 8
    if op == SOLARIZE:
        return 0 <= param <= 256
    return IDENTITY <= op <= EQUALIZE and param == 0


def histogram(img, chw=False):
    """img: [H, W] / [H, W, C] (chw: [C, H, W]) uint8 -> int64 [C, 256]"""
    a = np.asarray(img)
    if a.ndim == 2:
        planes = [a]
    elif chw:
        planes = list(a)
    else:
        planes = [a[..., c] for c in range(a.shape[-1])]
    return np.stack([np.bincount(p.reshape(-1), minlength=256).astype(np.int64) for p in planes])


def autocontrast_table(h):
    """one channel's bins (256 Python ints) -> its table: ImageOps.autocontrast with cutoff 0"""
    h = [int(v) for v in h]
    lo = next((i for i in range(256) if h[i]), 255)
    hi = next((i for i in range(255, -1, -1) if h[i]), 0)
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(255, max(0, int(i * scale + offset))) for i in range(256)]


def equalize_table(h):
    """one channel's bins -> its table: ImageOps.equalize without a mask, through point()'s clipping"""
    h = [int(v) for v in h]
    histo = [v for v in h if v]
    if len(histo) <= 1:
        return list(range(256))
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return list(range(256))
    n = step // 2
    t = []
    for i in range(256):
        t.append(min(n // step, 255))
        n += h[i]
    return t


def table(op, param, h=None):
    """the table of (op, param) for one channel with bins h (needed for AUTOCONTRAST and EQUALIZE) as uint8 [256]"""
    assert valid(op, param), (op, param)
    i = np.arange(256)
    if op == IDENTITY:
        t = i
    elif op == INVERT:
        t = 255 - i
    elif op == POSTERIZE:
        t = i & ~((1 << (8 - param)) - 1) & 255
    elif op == SOLARIZE:
        t = np.where(i < param, i, 255 - i)
    elif op == AUTOCONTRAST:
        t = autocontrast_table(h)
    else:
        t = equalize_table(h)
    return np.asarray(t, np.uint8)


def tables(op, param, hist, channels):
    """uint8 [channels, 256]; hist: [channels, 256] or None"""
    return np.stack([table(op, param, None if hist is None else hist[c]) for c in range(channels)])


def apply_luts(img, luts, chw=False):
    """out[c] = luts[c][in[c]]"""
    a = np.asarray(img)
    if a.ndim == 2:
        return luts[0][a]
    if chw:
        return np.stack([luts[c][a[c]] for c in range(a.shape[0])])
    return np.stack([luts[c][a[..., c]] for c in range(a.shape[-1])], -1)


def apply(op, param, img, chw=False):
    a = np.asarray(img)
    channels = 1 if a.ndim == 2 else (a.shape[0] if chw else a.shape[-1])
    hist = histogram(a, chw) if op in NEEDS_HIST else None
    return apply_luts(a, tables(op, param, hist, channels), chw)


# ---- the histograms no image of testable size produces: synthetic bins for the table builder ----
def equalize_cases():
    """named one-channel bin lists (Python ints, each < 2^32) that take every branch of equalize"""
    rng = np.random.default_rng(5)
    out = {}
    out["empty"] = [0] * 256
    flat = [0] * 256
    flat[77] = 1 << 20
    out["one_bin"] = flat
    two = [0] * 256
    two[3], two[200] = 1000, 5
    out["two_bins"] = two
    small = [0] * 256                       # fewer than 255 pixels outside the last bin: step 0
    small[10], small[20], small[250] = 100, 154, 70000
    out["step_zero"] = small
    edge = [0] * 256                        # exactly 255 outside the last bin: step 1
    edge[0], edge[255] = 255, 9
    out["step_one"] = edge
    # a bin in use with n // step > 255, which point() clips: total - last = 255 step + r gives the last bin the quotient
    # 255 + (step // 2 + r) // step, so a small step does it -- step 1, r 254: 509; step 2, r 254: 382
    big = [0] * 256
    big[5], big[6], big[200] = 300, 209, 100000
    out["quotient_509"] = big
    big2 = [0] * 256
    big2[0], big2[128], big2[129], big2[255] = 400, 300, 64, 7
    out["quotient_382"] = big2
    out["random"] = [int(v) for v in rng.integers(0, 5000, 256)]
    sparse = [0] * 256
    for i in rng.choice(256, 9, replace=False):
        sparse[int(i)] = int(rng.integers(1, 1 << 16))
    out["sparse"] = sparse
    total = [0] * 256                       # the bins of a 65535 x 65535 image: the running n passes 2^32
    total[0], total[100], total[255] = 65535 * 65535 - 2 * 65535, 65535, 65535
    out["sum_65535_squared"] = total
    spread = [(65535 * 65535 - 65535) // 255] * 255 + [65535]
    spread[0] += 65535 * 65535 - sum(spread)
    out["sum_65535_squared_spread"] = spread
    return out


def autocontrast_pairs():
    """all 32 640 (lo, hi) with lo < hi"""
    return [(lo, hi) for lo in range(256) for hi in range(lo + 1, 256)]


def two_bin_hist(lo, hi):
    h = np.zeros(256, np.uint32)
    h[lo], h[hi] = 3, 5
    return h
