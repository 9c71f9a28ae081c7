"""The inputs that take the tensor stages' output conversions (zune-jpeg_amd/csrc/zj_resize.h: resize_f32, resize_pack2,
resize_u8) to the edges of each number format, and the classifier that says which edge an element sits on.  TEST ONLY; numpy
only (no GPU, no torch), shared by test_convert_cases.py, test_convert_edges_emu.py and test_gpu_convert_edges.py.

The definition (include/zjhip.h): y = fl32(fl32(fl32(v) * s) + b) with s = scale * 2^-16 formed in float32, v the stage's
value in 1/65536 grey levels; F16 / BF16 are y rounded to nearest-even with gradual underflow; U8 is (v + 32768) >> 16.

Images: u8 sources of SRC (24 x 6) for the resampling stages and of the output sizes for the stages that do not resample.
Every colour image holds a 0..255 ramp, noise and a 0/255 checkerboard, one per channel, and the three rotations of that
assignment make three images, so that every channel's factors meet every kind of content; the fourth image is the 0/255
step-and-checkerboard that drives the bicubic filter into both of its clamps.  Row 0 of every plane starts with runs of 0, 255,
1 and 254.  The outputs (67 x 13 and 7 x 5) have a lead, whole groups of eight and a tail, and odd widths, so the half-filled
last pair of resize_pack2 is emitted.

Factor sets: one (scale, bias) per channel, so a three-channel launch carries three; a one-channel launch takes them one
at a time (factor_cases).
"""
import math

import numpy as np

import resize_model as rm

F32, F16, BF16, U8 = rm.F32, rm.F16, rm.BF16, rm.U8
SRC = (24, 6)
OUTS = [(67, 13), (7, 5)]
KINDS = ["ramp", "noise", "checker"]


def plane(kind, w, h, seed=0):
    """one u8 plane [h, w]"""
    yy, xx = np.indices((h, w))
    if kind == "ramp":
        p = np.linspace(0, 255, w * h).astype(np.uint8).reshape(h, w)
    elif kind == "noise":
        p = np.random.default_rng(1000 + seed).integers(0, 256, (h, w)).astype(np.uint8)
    elif kind == "checker":
        p = (((xx + yy) & 1) * 255).astype(np.uint8)
    elif kind == "step":  # a 0 -> 255 step above, the checkerboard below; seed 1: 255 -> 0; seed 2: the step lies across
        edge = (yy * 2 >= h) if seed == 2 else (xx * 2 >= w)
        p = np.where(edge ^ (seed == 1), 255, 0).astype(np.uint8)
        low = yy * 3 >= 2 * h
        p[low] = (((xx + yy) & 1) * 255).astype(np.uint8)[low]
        return p
    else:
        raise ValueError(kind)
    runs = np.repeat(np.array([0, 255, 1, 254], np.uint8), 4)[:w]
    p[0, :runs.size] = runs
    return p


def images(w, h, channels):
    """the four images of a launch, [C, h, w] uint8 each"""
    if channels == 1:
        return [plane(k, w, h)[None] for k in KINDS] + [plane("step", w, h)[None]]
    out = [np.stack([plane(KINDS[(c + r) % 3], w, h, seed=r) for c in range(3)]) for r in range(3)]
    return out + [np.stack([plane("step", w, h, seed=c) for c in range(3)])]


FLIPS = [False, True, False, True]

_STD, _MEAN = np.array([0.229, 0.224, 0.225]), np.array([0.485, 0.456, 0.406])
# name -> (scale[3], bias[3]).  What each is aimed at:
#   half_subnormal  y below 2^-14: subnormal halves, inexact ones, ties between two of them, zero from a non-zero y, and the
#                   smallest normal reached from below
#   half_min_normal y in [2^-14 - 2^-26, 2^-14): the smallest normal half, reached by rounding a subnormal-range y up
#   half_overflow   y around 65504 .. 65520 and beyond: inf from a finite y, in both signs; 256.94118 x 255 = 65520, the tie
#   half_top        y in [65504, 65520): the largest finite half, by truncation and by rounding down from above 65504
#   half_ties       y a multiple of 2^-3 near 2048, of 2^5 near 2^16 / 8 ...: exact ties of normal halves
#   bf16_top        y near 2^127 .. FLT_MAX: bf16 inf from a finite float32
#   f32_overflow    the product or the sum overflows float32
#   f32_subnormal   the product, the sum, or both are float32 subnormals; bf16 subnormals and bf16 zero from a non-zero y
#   cancel          t + b = +0 exactly, and around it
#   negzero         v = 0 times a negative scale plus a bias of -0.0: y = -0.0, kept by every format
SETS = {
    "imagenet": (1 / (255 * _STD), -_MEAN / _STD),
    "half_subnormal": ([2.0 ** -21, 3.0 * 2 ** -23, 2.0 ** -25], [-2.0 ** -14, 0.0, 2.0 ** -24]),
    "half_min_normal": ([-2.0 ** -30, 2.0 ** -30, -2.0 ** -28], [2.0 ** -14, 2.0 ** -14 - 2.0 ** -22, 2.0 ** -14]),
    "half_overflow": ([514.0, -257.0, 256.94118], [-65535.0, 0.0, 0.0]),
    "half_top": ([65504.0 / 255, 256.9, -65519.0 / 255], [0.0, 0.0, 0.0]),
    "half_ties": ([2.0 ** -3, 2.0 ** 5, 2.0 ** -13], [2048.0, 0.0, -2.0 ** -6]),
    "bf16_top": ([2.0 ** 120, -2.0 ** 120, 2.0 ** 119], [0.0, 0.0, 3.0e38]),
    "f32_overflow": ([3.0e38, -3.0e38, 1.0e36], [0.0, 1.0, -3.4e38]),
    "f32_subnormal": ([2.0 ** -126, -2.0 ** -131, 2.0 ** -133], [0.0, 2.0 ** -149, -2.0 ** -127]),
    "cancel": ([1 / 255, 1 / 255, 1.0], [-0.5, -1.0, -255.0]),
    "negzero": ([-1.0, -2.0 ** -131, -3.0e38], [-0.0, -0.0, -0.0]),
}


def factor_cases(channels):
    """(name, scale, bias) of every launch's factors, float32 arrays of `channels`"""
    for name, (sc, bi) in SETS.items():
        sc, bi = np.asarray(sc, np.float32), np.asarray(bi, np.float32)
        if channels == 3:
            yield name, sc, bi
        else:
            for k in range(3):
                yield f"{name}[{k}]", sc[k:k + 1], bi[k:k + 1]


# ---- the classes ----------------------------------------------------------------------------------------------------
CLASSES = {
    F32: ["f32_product_subnormal", "f32_sum_subnormal", "f32_inf", "f32_zero_from_cancellation", "f32_negzero", "fma_differs"],
    F16: ["half_inf_from_finite", "half_largest_finite", "half_subnormal", "half_subnormal_inexact", "half_zero_from_nonzero",
          "half_smallest_normal_rounded_up", "half_tie", "half_subnormal_tie", "half_negzero"],
    BF16: ["bf16_inf_from_finite", "bf16_tie", "bf16_subnormal", "bf16_zero_from_nonzero", "bf16_negzero"],
    U8: ["u8_exact_half"],
}
BICUBIC_CLASSES = ["clamped_at_0", "clamped_at_255"]


def masks(v, scale, bias, axis=0):
    """v: integer array whose axis `axis` is the channel -> {class: boolean array of v's shape}.  Raises on a NaN."""
    v = np.asarray(v, np.int64)
    ch = v.shape[axis]
    s, b = rm.factors(ch, scale, bias)
    shape = [1] * v.ndim
    shape[axis] = ch
    s, b = s.reshape(shape), b.reshape(shape)
    with np.errstate(all="ignore"):
        vf = v.astype(np.float32)
        t = (vf * s).astype(np.float32)
        y = (t + b).astype(np.float32)
        fused = (vf.astype(np.float64) * s.astype(np.float64) + b.astype(np.float64)).astype(np.float32)  # (exact, rounded once)
        half = y.astype(np.float16)
        back = half.astype(np.float32)
        # the half on the other side of y, for the ties: y is as far from it as from `half`
        other = np.nextafter(half, np.where(y > back, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
        tie16 = (back != y) & np.isfinite(other) & (np.abs(y.astype(np.float64) - back) == np.abs(other.astype(np.float64) - y))
    if np.isnan(y).any() or np.isnan(t).any():
        raise AssertionError("a NaN: the factors are not usable")
    u, tu = y.view(np.uint32), t.view(np.uint32)
    a, ta = u & 0x7FFFFFFF, tu & 0x7FFFFFFF
    hb = half.view(np.uint16).astype(np.uint32)
    ha = hb & 0x7FFF
    bb = rm.bf16_bits(y).astype(np.uint32)
    ba = bb & 0x7FFF
    finite = a < 0x7F800000
    hsub = (ha > 0) & (ha < 0x400)
    return {
        "f32_product_subnormal": (ta > 0) & (ta < 0x00800000),
        "f32_sum_subnormal": (a > 0) & (a < 0x00800000),
        "f32_inf": ~finite,
        "f32_zero_from_cancellation": (u == 0) & (ta != 0),
        "f32_negzero": u == 0x80000000,
        "fma_differs": fused.view(np.uint32) != u,
        "half_inf_from_finite": finite & (ha == 0x7C00),
        "half_largest_finite": ha == 0x7BFF,
        "half_subnormal": hsub,
        "half_subnormal_inexact": hsub & (back != y),
        "half_zero_from_nonzero": (a > 0) & (ha == 0),
        "half_smallest_normal_rounded_up": (ha == 0x400) & (a < 0x38800000),
        "half_tie": tie16 & (a >= 0x38800000) & finite,
        "half_subnormal_tie": tie16 & (a < 0x38800000),
        "half_negzero": hb == 0x8000,
        "bf16_inf_from_finite": finite & (ba == 0x7F80),
        "bf16_tie": finite & ((u & 0xFFFF) == 0x8000),
        "bf16_subnormal": (ba > 0) & (ba < 0x80),
        "bf16_zero_from_nonzero": (a > 0) & (ba == 0),
        "bf16_negzero": bb == 0x8000,
        "u8_exact_half": (v & 0xFFFF) == 0x8000,
    }


def classify(v, scale, bias, axis=0):
    """counts per class"""
    return {k: int(m.sum()) for k, m in masks(v, scale, bias, axis).items()}


def classes_at(v, scale, bias, index, axis=0):
    """the classes of the element v.reshape(-1)[index], as text"""
    hit = [k for k, m in masks(v, scale, bias, axis).items() if m.reshape(-1)[index]]
    return ", ".join(hit) if hit else "no edge class"


def first_difference(got, exp, v, scale, bias, axis=0):
    """None if the two integer arrays are equal, else a sentence naming the first differing element and its classes"""
    got, exp = np.asarray(got).reshape(-1), np.asarray(exp).reshape(-1)
    bad = np.nonzero(got != exp)[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (f"{bad.size} of {exp.size} elements differ; the first, element {i}: got {int(got[i]):#x}, the model {int(exp[i]):#x}, "
            f"v = {int(np.asarray(v).reshape(-1)[i])}, classes: {classes_at(v, scale, bias, i, axis)}")


# ---- the warp stage's matrices: an enlargement that leaves the source on two sides, 17 degrees about the centre, a half-
# pixel shift, the identity scale (a, b, c, d, e, f; output pixel centre -> source coordinates) ----------------------------------
def warp_matrices(w, h, ow, oh):
    sx, sy = w / ow, h / oh
    co, si = math.cos(math.radians(17)), math.sin(math.radians(17))
    return [(sx * 1.25, 0.0, -1.5, 0.0, sy * 1.25, -0.75),
            (co * sx, -si * sy, w / 2 - co * sx * ow / 2 + si * sy * oh / 2, si * sx, co * sy, h / 2 - si * sx * ow / 2 - co * sy * oh / 2),
            (sx, 0.0, 0.5, 0.0, sy, -0.25),
            (sx, 0.0, 0.0, 0.0, sy, 0.0)]


WARP_FILL = (0, 255, 77)


# ---- coefficient planes for the two plane calls: DC-only blocks under all-ones tables, so that a block is flat at
# 128 + DC / 8 and a reduced-size decode keeps the level; a horizontal first harmonic in every other block ------------------
def frame(width, height, hs, vs, seed):
    """(planes, qts): luma blocks whose levels walk 0, 255, 1, 254 and a ramp; chroma near grey"""
    rng = np.random.default_rng(seed)
    mcu_x, mcu_y = (width + 8 * hs - 1) // (8 * hs), (height + 8 * vs - 1) // (8 * vs)
    planes = []
    for c in range(3):
        br, bc = (mcu_y * vs, mcu_x * hs) if c == 0 else (mcu_y, mcu_x)
        blk = np.zeros((br * bc, 64), np.int16)
        if c == 0:
            level = np.linspace(0, 255, br * bc).astype(np.int64)
            level[::5] = np.resize([0, 255, 1, 254], level[::5].size)
            blk[:, 0] = (level - 128) * 8
            blk[1::2, 1] = rng.integers(-160, 161, blk[1::2, 1].size)
        else:
            blk[:, 0] = rng.integers(-6, 7, br * bc) * 8
        planes.append(blk.reshape(-1))
    return planes, [np.ones(64, np.int32)] * 3


# crop-tensor: 4:2:0, 112 x 40 -- the reference drops the odd third MCU row, so rows 32 .. 39 are the stage's fill path (the
# conversion of a zero byte); the windows of each output size, one per frame of the launch
CROP_FRAME = (112, 40, 2, 2)
CROP_ORIGINS = {(67, 13): [(0, 27), (45, 27), (20, 0), (33, 19)], (7, 5): [(3, 30), (105, 35), (50, 10), (0, 0)]}
# resized crop over a 1/2 reduced decode (max_prescale 2): 4:4:4, 144 x 32; every window at least twice the larger output
SCALED_FRAME = (144, 32, 1, 1)
SCALED_WINDOWS = [(0, 0, 144, 32), (2, 1, 140, 30), (8, 4, 136, 27), (5, 0, 139, 32)]


# ---- every stage's value v over its images, from the stage's numpy model ---------------------------------------------------
STAGES = ["resize", "resize_aa", "resize_bicubic", "to_tensor", "crop_tensor", "warp_fill", "warp_replicate", "scaled"]


def crop_frame(channels):
    """(descriptor arguments, planes, qts) of the crop-tensor launch: out_colorspace 1 (grey) for one channel, 0 (RGB) for three"""
    w, h, hs, vs = CROP_FRAME
    planes, qts = frame(w, h, hs, vs, seed=7)
    return (w, h, hs, vs, 3, 1 if channels == 1 else 0, qts), planes, qts


def scaled_frame(channels):
    w, h, hs, vs = SCALED_FRAME
    planes, qts = frame(w, h, hs, vs, seed=11)
    return (w, h, hs, vs, 3, 1 if channels == 1 else 0, qts), planes, qts


def scaled_sources(channels):
    """the 1/2 reduced crops the resize of the prescaled call reads, [C, h, w] uint8 each (tests/scaled_model.py)"""
    import scaled_model as sm
    (w, h, hs, vs, ncomp, cs, qts), planes, _ = scaled_frame(channels)
    img = sm.decode_scaled(w, h, hs, vs, ncomp, cs, qts, planes, 1)
    out = []
    for (x, y, ww, hh) in SCALED_WINDOWS:
        rx, ry, rw, rh = sm.reduced_window(x, y, ww, hh, 1, w, h)
        out.append(np.ascontiguousarray(img[ry:ry + rh, rx:rx + rw].transpose(2, 0, 1)))
    return out


def crop_sources(channels, size):
    """the u8 crops of the crop-tensor launch as the emulated crop kernel decodes them (tests/emu_crop), [C, h, w] each"""
    import emu_crop_c as ec
    args, planes, _ = crop_frame(channels)
    d = ec.desc(*args)
    n = len(CROP_ORIGINS[size])
    rc, crops = ec.decode_crops(d, [planes] * n, CROP_ORIGINS[size], size[0], size[1])
    assert rc == 0
    return [c.reshape(size[1], size[0], channels).transpose(2, 0, 1) for c in crops]


def stage_values(stage, channels):
    """[(output size, image index, v [C, oh, ow] int64)] of one stage's launches; resize_bicubic: a fourth entry, the value
    before the clamp"""
    import resize_aa_model as am
    import resize_bicubic_model as bm
    import warp_model as wm
    out = []
    for size in OUTS:
        ow, oh = size
        if stage in ("resize", "resize_aa", "resize_bicubic"):
            for i, img in enumerate(images(*SRC, channels)):
                if stage == "resize_bicubic":
                    raw = bm.passes(img, ow, oh)[2]
                    out.append((size, i, np.clip(raw, 0, bm.V_MAX), raw))
                else:
                    out.append((size, i, (rm if stage == "resize" else am).values(img, ow, oh)))
        elif stage == "to_tensor":
            out += [(size, i, img.astype(np.int64) << 16) for i, img in enumerate(images(ow, oh, channels))]
        elif stage == "crop_tensor":
            out += [(size, i, c.astype(np.int64) << 16) for i, c in enumerate(crop_sources(channels, size))]
        elif stage in ("warp_fill", "warp_replicate"):
            edge = wm.FILL if stage == "warp_fill" else wm.REPLICATE
            for i, (img, m) in enumerate(zip(images(*SRC, channels), warp_matrices(*SRC, ow, oh))):
                out.append((size, i, wm.values(img.transpose(1, 2, 0), wm.fixed(m), ow, oh, edge, WARP_FILL)))
        elif stage == "scaled":
            out += [(size, i, rm.values(img, ow, oh)) for i, img in enumerate(scaled_sources(channels))]
        else:
            raise ValueError(stage)
    return out


def stage_counts(stage, channels=3):
    """class -> how many elements of the stage's launches (every factor set, every image, both output sizes) are in it"""
    total = {}
    vals = stage_values(stage, channels)
    for name, sc, bi in factor_cases(channels):
        for entry in vals:
            for k, n in classify(entry[2], sc, bi).items():
                total[k] = total.get(k, 0) + n
    u8 = sum(int(((e[2] & 0xFFFF) == 0x8000).sum()) for e in vals)
    total["u8_exact_half"] = u8
    if stage == "resize_bicubic":
        import resize_bicubic_model as bm
        total["clamped_at_0"] = sum(int((e[3] < 0).sum()) for e in vals)
        total["clamped_at_255"] = sum(int((e[3] > bm.V_MAX).sum()) for e in vals)
    return total


# ---- comparing an output with its model, as integers -------------------------------------------------------------------------
INT_OF = {F32: np.uint32, F16: np.uint16, BF16: np.uint16, U8: np.uint8}


def as_ints(a, dtype):
    """an output's bytes, or the model's array (float32 values, uint16 bits or uint8), as a flat array of integers"""
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), INT_OF[dtype])


def check(got, exp, dtype, v, scale, bias, flip, layout, what):
    """got: the image's bytes; exp: the model's output in `layout`; v [C, oh, ow]: the model's values, for the report"""
    vv = v[:, :, ::-1] if flip else v
    vv = vv.transpose(1, 2, 0) if layout == "NHWC" else vv
    msg = first_difference(as_ints(got, dtype), as_ints(exp, dtype), vv, scale, bias, 2 if layout == "NHWC" else 0)
    if msg:
        raise AssertionError(f"{what}: {msg}")


_VALUES = {}


def cached_values(stage, channels):
    """stage_values, computed once and read-only"""
    if (stage, channels) not in _VALUES:
        vals = stage_values(stage, channels)
        for e in vals:
            e[2].setflags(write=False)
        _VALUES[stage, channels] = {(e[0], e[1]): e[2] for e in vals}
    return _VALUES[stage, channels]
