"""Matrices for the warp-limit tests (test_warp_limits_emu.py, test_gpu_warp_limits.py): the affine warp's position arithmetic
(zj_warp.h) where its operands do not fit 32 bits -- A, B, D, E at +-2^31 and +-(2^31 - 1), C0 and F0 near
+-2^55, first-tap indices beyond int32 on both sides, the clamp of warp_pos approached from both sides, negative U at every
edge of the two shifts -- on sources from 1 x 1 up to the ends of the packed w | h << 16.  Every matrix is six doubles, the only
form the public calls take.  What the set reaches is stated by assert_cases() from numpy and Python integers alone, together
with seven wrong variants of warp_model.positions, each of which some named case must tell from the model: no kernel under test
has a say in it.  TEST ONLY."""
import contextlib
import functools
import math
import zlib
from fractions import Fraction

import numpy as np

import warp_model as wm

Q = 24
ONE = 1 << Q
FILL, REPLICATE = wm.FILL, wm.REPLICATE
BOTH = (FILL, REPLICATE)
LIN_MAX = math.nextafter(128.0, 0.0)            # A = 2^31: the largest entry the definition takes, rounded up
LIN_ODD = float((1 << 31) - 1) / ONE            # A = 2^31 - 1
LIN_F1 = float((1 << 31) - 65521) / ONE         # the fraction moves by about -1/256 pixel per output pixel ...
LIN_F2 = float((1 << 31) - 33001) / ONE         # ... and by about -1/512
OFF_MAX = math.nextafter(2.0 ** 31, 0.0)        # 2^31 - 2^-22: C0 = 2^55 - 4 + (a + b - 1) 2^23
OFF_INT = 2.0 ** 31 - 1
FILLS = ((0, 0, 0), (7, 130, 255))
FRAMES = ((96, 80), (1, 1), (65535, 65535))
# U at an output pixel -> the (i0, f) the definition's two floors give
FLOORS = ((-1, (-1, 255)), (-(1 << 16), (-1, 255)), (-(1 << 16) - 1, (-1, 254)), (-(1 << 24), (-1, 0)), (-(1 << 24) - 1, (-2, 255)),
          (-(1 << 24) + (1 << 16) - 1, (-1, 0)), (-(1 << 32), (-256, 0)), (-(1 << 32) - 1, (-257, 255)))
CLAMP_FRACTIONS = (0, 1, 255)


# ---- the definition on Python integers and rationals ----------------------------------------------------------------------
def fixed_ints(m):
    """warp_model.fixed restated on rationals: every double operation is the exact result rounded once (float(Fraction) rounds
    to nearest even, as the hardware does), the products by 1/2 and 2^24 are exact"""
    m = [float(v) for v in m]
    rq = lambda x: math.floor(Fraction(float(Fraction(x) * ONE + Fraction(1, 2))))
    add = lambda x, y: float(Fraction(x) + Fraction(y))
    a, b, c, d, e, f = m
    return [rq(a), rq(b), rq(add(add(add(a * 0.5, b * 0.5), c), -0.5)), rq(d), rq(e), rq(add(add(add(d * 0.5, e * 0.5), f), -0.5))]


def pos_int(A, B, C0, X, Y):
    """(i0, f) of one axis at one output pixel, Python integers (>> is a floor on them)"""
    u = (A * X + B * Y + C0) >> 16
    return u >> 8, u & 255


def window_ints(q, fw, fh, out_w, out_h, edge):
    """warp_model.source_window restated on Python integers: ((x, y, w, h), shifted integers)"""
    box = []
    for ax, n in ((0, fw), (1, fh)):
        A, B, C0 = (int(v) for v in q[3 * ax:3 * ax + 3])
        taps = [pos_int(A, B, C0, X, Y)[0] for X in (0, out_w - 1) for Y in (0, out_h - 1)]
        lo, hi = min(taps), max(taps) + 1
        if edge == REPLICATE:
            lo, hi = sorted((0, lo, n - 1))[1], sorted((0, hi, n - 1))[1]
        else:
            lo, hi = max(lo, 0), min(hi, n - 1)
        box.append((lo, hi))
    if any(lo > hi for lo, hi in box):
        return (0, 0, 0, 0), [int(v) for v in q]
    sh = [int(v) for v in q]
    sh[2] -= box[0][0] * ONE
    sh[5] -= box[1][0] * ONE
    return (box[0][0], box[1][0], box[0][1] - box[0][0] + 1, box[1][1] - box[1][0] + 1), sh


def ints_valid(q):
    """zj_warp_fixed.h's warp_ints_valid"""
    return all(abs(int(v)) <= ((1 << 55) + (1 << 32) if k % 3 == 2 else 1 << 31) for k, v in enumerate(q))


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _offset_for(lin, cross, target, at):
    """the double c under which U = target (an integer, units of 2^-24) at the output pixel `at` = (own index, other index) of
    an axis with entries lin (times its own index) and cross: C0 = target - A own - B other"""
    A, B = fixed_ints((lin, cross, 0, 0, 0, 0))[:2]
    c0 = target - A * at[0] - B * at[1]
    return float(Fraction(c0, ONE) + Fraction(1, 2) - Fraction(lin) / 2 - Fraction(cross) / 2)


def _matrix(ax, lin, off, olin, ooff, cross=0.0):
    """ax 0: x = lin (X + 1/2) + cross (Y + 1/2) + off, y = olin (Y + 1/2) + ooff; ax 1: the axes exchanged"""
    return (lin, cross, off, 0.0, olin, ooff) if ax == 0 else (olin, 0.0, ooff, cross, lin, off)


def _case(name, src, ch, out, m, edges=BOTH, **tags):
    m = tuple(float(v) for v in m)
    return dict(name=name, group=name.split("/")[0], src=src, ch=ch, out=out, m=m, ints=tuple(fixed_ints(m)), edges=tuple(edges), **tags)


def _linear():
    """an entry at the limit, the offset c = t - lin (X* + 1/2): the pixel X* lands at source coordinate t, its neighbours 128
    pixels to either side"""
    out = []
    rows = [  # ax, src, ch, out, lin, t, X*, the other axis: olin, ooff
        (0, (65535, 1), 3, (8192, 1), LIN_MAX, 32894.3, 4096, 0.0, 0.5 + 77 / 256),
        (0, (65535, 1), 3, (8185, 2), -LIN_ODD, 32894.7, 4000, 1.0, -0.25),
        (0, (65535, 1), 3, (8192, 1), LIN_F1, 32768.0, 4096, 0.0, 0.5),
        (0, (65535, 2), 1, (8185, 2), -LIN_MAX, 32894.3, 4100, 1.0, 0.0),
        (0, (65535, 2), 1, (8192, 1), LIN_ODD, 32000.2, 3000, 0.0, 1.0),
        (0, (65535, 2), 1, (8185, 2), -LIN_F2, 32768.5, 4096, 1.0, 0.3),
        (0, (5, 3), 3, (8192, 1), LIN_MAX, 2.3, 8190, 0.0, 1.7),
        (0, (7, 5), 1, (8185, 2), -LIN_MAX, 3.6, 8183, 1.0, 1.2),
        (0, (258, 3), 3, (8192, 1), LIN_ODD, 130.4, 4097, 0.0, 1.1),
        (0, (1, 1), 1, (8192, 1), -LIN_ODD, 0.7, 8190, 0.0, 0.5),
        (0, (2, 1), 3, (8185, 2), LIN_F1, 1.0, 5000, 0.5, 0.3),
        (1, (1, 65535), 3, (1, 8192), LIN_MAX, 32894.3, 4096, 0.0, 0.5 + 33 / 256),
        (1, (1, 65535), 3, (9, 8192), -LIN_F1, 32768.0, 4096, 0.25, -0.6),
        (1, (1, 65535), 3, (1, 8192), -LIN_ODD, 32001.9, 5000, 0.0, 0.5),
        (1, (3, 65535), 1, (9, 8192), -LIN_MAX, 32894.3, 4100, 0.5, -0.75),
        (1, (3, 65535), 1, (1, 8192), LIN_F2, 32768.5, 4000, 0.0, 1.5),
        (1, (3, 65535), 1, (9, 8192), LIN_ODD, 32894.6, 4200, 0.375, 0.0),
        (1, (5, 3), 1, (9, 8192), -LIN_MAX, 1.4, 8190, 0.5, 0.2),
        (1, (7, 5), 3, (1, 8192), LIN_MAX, 2.6, 8000, 0.0, 3.3),
        (1, (258, 3), 1, (9, 8192), LIN_ODD, 1.5, 4000, 28.0, 3.0),
    ]
    for k, (ax, src, ch, o, lin, t, xs, olin, ooff) in enumerate(rows):
        out.append(_case(f"linear/{'xy'[ax]}{k}-{src[0]}x{src[1]}", src, ch, o, _matrix(ax, lin, t - lin * (xs + 0.5), olin, ooff), axis=ax))
    # all four entries at the limit, mixed signs: pixel (32, 16) lands inside and with it its diagonal (a = -b, d = -e up to one
    # unit), every other pixel 128 source pixels or more away
    for k, (src, ch, (a, b, d, e), (tx, ty)) in enumerate([((7, 5), 3, (LIN_MAX, -LIN_MAX, -LIN_ODD, LIN_MAX), (3.4, 2.2)),
                                                           ((258, 3), 1, (-LIN_MAX, LIN_ODD, LIN_MAX, -LIN_MAX), (130.7, 1.5))]):
        m = (a, b, tx - a * 32.5 - b * 16.5, d, e, ty - d * 32.5 - e * 16.5)
        out.append(_case(f"linear/all4-{k}", src, ch, (65, 33), m, axis=2))
    return out


def _offsets():
    """c, f at the limit: the first tap's index leaves int32 on either side"""
    out = []
    offs = (OFF_MAX, -OFF_MAX, OFF_INT, -OFF_INT)
    lins = (0.0, 1.0, LIN_MAX, -LIN_MAX)
    k = 0
    for ax in (0, 1):
        for off in offs:
            for lin in lins:
                src, ch = [((5, 3), 3), ((7, 5), 1)][k % 2]
                o = [(16, 1), (65, 33)][(k // 2) % 2]
                out.append(_case(f"offset/{'xy'[ax]}{k}", src, ch, o, _matrix(ax, lin, off, src[1 - ax] / o[1 - ax], 0.0), axis=ax))
                k += 1
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):  # both at once: the four corners
        out.append(_case(f"offset/corner{k}", (5, 3), 3, (16, 1) if sx == sy else (65, 33),
                         (1.0, 0.0, sx * OFF_MAX, 0.0, LIN_MAX * sx, sy * OFF_INT), axis=2))
        k += 1
    return out


def _clamps():
    """first-tap indices -3 .. n + 1 at fractions 0, 1, 255: one index per output pixel with a unit entry; with an entry at the
    limit at pixel 5 of 9 alone (its neighbours 128 pixels off, deep in the clamp), the index moved by the other output axis"""
    out = []
    for src in ((1, 1), (2, 1), (7, 5)):
        for ax in (0, 1):
            n = src[ax]
            for fr in CLAMP_FRACTIONS:
                target = (-3 * 256 + fr) << 16
                ch = 3 if (ax + fr) % 2 else 1
                o = (n + 5, 2) if ax == 0 else (2, n + 5)
                m = _matrix(ax, 1.0, _offset_for(1.0, 0.0, target, (0, 0)), 0.5, 0.1)
                out.append(_case(f"clamp/unit-{'xy'[ax]}-{src[0]}x{src[1]}-f{fr}", src, ch, o, m, axis=ax, fraction=fr, kind="unit"))
                lin = LIN_MAX if ax == 0 else -LIN_MAX
                o = (9, n + 5) if ax == 0 else (n + 5, 9)
                m = _matrix(ax, lin, _offset_for(lin, 1.0, target, (5, 0)), 0.3, 0.1, cross=1.0)
                out.append(_case(f"clamp/limit-{'xy'[ax]}-{src[0]}x{src[1]}-f{fr}", src, ch, o, m, axis=ax, fraction=fr, kind="limit"))
    return out


def _floors():
    """negative U at every edge of the two shifts, on both axes at once: with a = e = 0 at every pixel, with a = e = 1 at
    pixel (3, 2)"""
    out = []
    for k, (u, _) in enumerate(FLOORS):
        src, ch = [((7, 5), 3), ((2, 1), 1)][k % 2]
        c = _offset_for(0.0, 0.0, u, (0, 0))
        out.append(_case(f"floor/zero-{k}", src, ch, (3, 2), (0.0, 0.0, c, 0.0, 0.0, c), u=u, at=(0, 0)))
        c, f = _offset_for(1.0, 0.0, u, (3, 0)), _offset_for(1.0, 0.0, u, (2, 0))
        out.append(_case(f"floor/unit-{k}", src, ch, (9, 5), (1.0, 0.0, c, 0.0, 1.0, f), u=u, at=(3, 2)))
    return out


def _degenerate():
    b = LIN_MAX
    return [_case("degenerate/zero", (5, 3), 3, (65, 33), (0.0,) * 6),
            _case("degenerate/a0-b-limit", (7, 5), 1, (65, 33), (0.0, b, 3.5 - b * 16.5, 0.0, 0.15, 0.0)),
            _case("degenerate/a-limit-e0", (258, 3), 3, (65, 33), (-b, 0.0, 129.2 + b * 32.5, 0.0, 0.0, 1.75))]


@functools.lru_cache(maxsize=None)
def _cases():
    cs = _linear() + _offsets() + _clamps() + _floors() + _degenerate()
    assert len({c["name"] for c in cs}) == len(cs)
    return tuple(cs)


def cases():
    return list(_cases())


def names():
    return [c["name"] for c in _cases()]


def by_name(name):
    return next(c for c in _cases() if c["name"] == name)


def rotation(k):
    """(dtypes and layouts, pitch pad, tensor base) of case k: F32 NHWC and U8 always, the third of the six others in turn"""
    import resize_model as rm
    rest = [(rm.F16, "NCHW"), (rm.BF16, "NHWC"), (rm.F32, "NCHW"), (rm.U8, "NHWC"), (rm.F16, "NHWC"), (rm.BF16, "NCHW")]
    return [(rm.F32, "NHWC"), (rm.U8, "NCHW"), rest[k % 6]], (0, 1, 13)[k % 3], k % 8


def cycle_matrices():
    """matrices that make sense on any small source and a 65 x 33 output, for a call of many images"""
    return [c["m"] for c in _cases() if c["out"] == (65, 33) and c["group"] in ("offset", "degenerate", "linear")]


@functools.lru_cache(maxsize=None)
def image(name):
    c = by_name(name)
    img = np.random.default_rng(zlib.crc32(name.encode())).integers(0, 256, (c["src"][1], c["src"][0], c["ch"]), dtype=np.uint8)
    img.setflags(write=False)
    return img


# ---- wrong variants of warp_model.positions ---------------------------------------------------------------------------------
def _grid(out_w, out_h):
    return np.meshgrid(np.arange(out_h, dtype=np.int64), np.arange(out_w, dtype=np.int64), indexing="ij")


def _i32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _variant(u_of=None, split=None, index=None):
    def positions(q, out_w, out_h, w, h):
        Y, X = _grid(out_w, out_h)
        res = []
        for (A, B, C0), n in ((q[:3], w), (q[3:], h)):
            U = u_of(A, B, C0, X, Y) if u_of else A * X + B * Y + C0
            i, f = split(U) if split else ((U >> 16) >> 8, (U >> 16) & 255)
            res += [index(i, n) if index else i, f]
        return res
    return positions


def _trunc(U):
    u = np.where(U < 0, -((-U) >> 16), U >> 16)
    return np.where(u < 0, -((-u) >> 8), u >> 8), u & 255


# name -> (the variant, the edge modes in which its error can show)
MUTANTS = {
    # an index in [2^31, 2^32) wraps to below -2^31 + 2^21 and one below -2^31 to above 2^31 - 2^21 (|i0| < 2^31 + 2^21 for every
    # matrix the definition takes): still outside every image, so FILL reads fill either way; REPLICATE reads the other edge
    "index narrowed to int32 before the clamp": (_variant(index=lambda i, n: _i32(i)), (REPLICATE,)),
    "A, B, D, E narrowed to int32": (_variant(u_of=lambda A, B, C0, X, Y: _i32(A) * X + _i32(B) * Y + C0), BOTH),
    "A X + B Y kept to its low 32 bits": (_variant(u_of=lambda A, B, C0, X, Y: _i32(A * X + B * Y) + C0), BOTH),
    "C0 narrowed to 32 bits": (_variant(u_of=lambda A, B, C0, X, Y: A * X + B * Y + _i32(C0)), BOTH),
    "both shifts truncate toward zero": (_variant(split=_trunc), BOTH),
    # at -2 both taps are outside, at -1 the second is tap 0: FILL differs.  REPLICATE clamps the taps of -2 and of -1 to
    # (0, 0) alike, those of n and of n - 1 to (n - 1, n - 1): no difference there
    "the clamp at [-1, n - 1]": (_variant(index=lambda i, n: np.clip(i, -1, n - 1)), (FILL,)),
    "the per-pixel step drops its carry": (_variant(u_of=lambda A, B, C0, X, Y: (((B * Y + C0) >> 32) << 32) + ((B * Y + C0 + A * X) & 0xFFFFFFFF)),
                                           BOTH),
}


@contextlib.contextmanager
def _positions_replaced(fn, w, h):
    keep = wm.positions
    wm.positions = lambda q, ow, oh: fn(q, ow, oh, w, h)
    try:
        yield
    finally:
        wm.positions = keep


def values(c, edge, variant=None):
    """the model's values [C, oh, ow] of a case over its image, or those of a wrong variant of its positions"""
    img, (ow, oh) = image(c["name"]), c["out"]
    fill = FILLS[1][:c["ch"]]
    if variant is None:
        return wm.values(img, list(c["ints"]), ow, oh, edge, fill)
    with _positions_replaced(variant, *c["src"]):
        return wm.values(img, list(c["ints"]), ow, oh, edge, fill)


@functools.lru_cache(maxsize=None)
def surviving_mutants():
    """({(mutant, edge): the first case whose values it changes}, [(mutant, edge) no case tells from the model])"""
    caught, alive = {}, []
    truth = {}
    for name, (variant, modes) in MUTANTS.items():
        for edge in modes:
            for c in _cases():
                if edge not in c["edges"]:
                    continue
                key = (c["name"], edge)
                if key not in truth:
                    truth[key] = values(c, edge)
                if not np.array_equal(values(c, edge, variant), truth[key]):
                    caught[(name, edge)] = c["name"]
                    break
            else:
                alive.append((name, edge))
    return caught, alive


# ---- what the set reaches ---------------------------------------------------------------------------------------------------
def _pixels(c, samples=1000):
    ow, oh = c["out"]
    if ow * oh <= 65 * 33:
        return [(X, Y) for Y in range(oh) for X in range(ow)]
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()) + 1)
    return [(X, Y) for X in (0, ow - 1) for Y in (0, oh - 1)] + [(int(rng.integers(ow)), int(rng.integers(oh))) for _ in range(samples)]


@functools.lru_cache(maxsize=None)
def assert_cases():
    """Asserts what the docstring of this module claims, and returns the counts the record quotes"""
    cs = _cases()
    rep = {"cases": len(cs), "calls": sum(len(c["edges"]) for c in cs)}
    seen_src, seen_out, seen_ch = {c["src"] for c in cs}, {c["out"] for c in cs}, {c["ch"] for c in cs}
    assert seen_src >= {(1, 1), (2, 1), (5, 3), (7, 5), (258, 3), (65535, 1), (65535, 2), (1, 65535), (3, 65535)}
    assert seen_out >= {(8192, 1), (8185, 2), (1, 8192), (9, 8192), (65, 33), (16, 1)} and seen_ch == {1, 3}
    umax = 0
    for c in cs:
        (ow, oh), (w, h), q = c["out"], c["src"], c["ints"]
        assert 1 <= ow <= 8192 and 1 <= oh <= 8192 and c["ch"] * ow * oh * 4 <= 1 << 20, c["name"]
        # the integers: the model's, the restatement's, and valid
        assert wm.fixed(c["m"]) == list(q), (c["name"], wm.fixed(c["m"]), q)
        assert ints_valid(q), c["name"]
        # the int64 model is exact: |U| is largest at a corner
        for ax in (0, 1):
            A, B, C0 = q[3 * ax:3 * ax + 3]
            m = max(abs(A * X + B * Y + C0) for X in (0, ow - 1) for Y in (0, oh - 1))
            assert m < 1 << 62, c["name"]
            umax = max(umax, m)
        x0, fx, y0, fy = wm.positions(list(q), ow, oh)
        for (X, Y) in _pixels(c):
            assert pos_int(*q[:3], X, Y) == (int(x0[Y, X]), int(fx[Y, X])) and pos_int(*q[3:], X, Y) == (int(y0[Y, X]), int(fy[Y, X])), \
                (c["name"], X, Y)
    rep["max |U|"] = umax
    assert umax < 1 << 56

    # ---- linear entries at the limit
    lin = [c for c in cs if c["group"] == "linear"]
    entries = {c["ints"][k] for c in lin for k in (0, 1, 3, 4)}
    assert {1 << 31, -(1 << 31), (1 << 31) - 1, 1 - (1 << 31)} <= entries
    assert {(1 << 31) - 65521, 65521 - (1 << 31), (1 << 31) - 33001, 33001 - (1 << 31)} & entries
    assert {c["ints"][0] for c in lin} >= {1 << 31, -(1 << 31)} and {c["ints"][4] for c in lin} >= {1 << 31, -(1 << 31)}
    assert any(all(abs(c["ints"][k]) >= (1 << 31) - 1 for k in (0, 1, 3, 4)) and len({c["ints"][k] > 0 for k in (0, 1, 3, 4)}) == 2 for c in lin)
    fxs, fys, last, inside, steps = set(), set(), set(), {}, 0
    for c in lin:
        (ow, oh), (w, h), q = c["out"], c["src"], c["ints"]
        x0, fx, y0, fy = wm.positions(list(q), ow, oh)
        both = (x0 >= 0) & (x0 < w) & (y0 >= 0) & (y0 < h)
        assert both.any(), c["name"]
        for ax, i0, n in ((0, x0, w), (1, y0, h)):
            A, B, C0 = q[3 * ax:3 * ax + 3]
            if abs(A) >= 1 << 30 or abs(B) >= 1 << 30:
                # the sum lands inside though its terms do not: A X and C0 (B Y and C0) pass 2^43 each where it does
                assert max(abs(A) * (ow - 1), abs(B) * (oh - 1)) >= 1 << 36 and abs(C0) >= 1 << 31, c["name"]
                assert (i0 < -2).any() and (i0 > n).any(), f"{c['name']}: the output does not leave the source on both sides"
            if abs(A) >= 1 << 30 and ow > 1:  # the lane's step: U += A.  It changes the high dword about every second time
                U = A * _grid(ow, oh)[1] + B * _grid(ow, oh)[0] + C0
                carried = int(((U[:, 1:] >> 32) != (U[:, :-1] >> 32)).sum())
                assert carried >= (ow - 1) * oh // 3, c["name"]
                steps += carried
        if c["axis"] == 0:
            fxs |= set(fx[both].tolist())
            cols = np.unique(x0[(x0 >= 0) & (x0 < w)])
            inside[c["name"]] = cols.size
            if w == 65535 and ((x0 == w - 1) | (x0 == w - 2)).any():
                last.add(("w", c["src"]))
        if c["axis"] == 1:
            fys |= set(fy[both].tolist())
            rows = np.unique(y0[(y0 >= 0) & (y0 < h)])
            inside[c["name"]] = rows.size
            if h == 65535 and ((y0 == h - 1) | (y0 == h - 2)).any():
                last.add(("h", c["src"]))
    assert fxs == set(range(256)) and fys == set(range(256)), (len(fxs), len(fys))
    assert last == {("w", (65535, 1)), ("w", (65535, 2)), ("h", (1, 65535)), ("h", (3, 65535))}, last
    for name, cnt in inside.items():
        big = 65535 in by_name(name)["src"]
        assert (500 <= cnt <= 514) if big else (1 <= cnt <= 3), (name, cnt)
    rep["carrying steps"] = steps
    rep["first taps inside, 65535 sources"] = sorted(v for k, v in inside.items() if 65535 in by_name(k)["src"])

    # ---- offsets at the limit
    offs = [c for c in cs if c["group"] == "offset"]
    assert {c["m"][2] for c in offs} >= {OFF_MAX, -OFF_MAX, OFF_INT, -OFF_INT} and {c["m"][5] for c in offs} >= {OFF_MAX, -OFF_MAX, OFF_INT, -OFF_INT}
    assert {c["m"][0] for c in offs} >= {0.0, 1.0, LIN_MAX, -LIN_MAX} and {c["out"] for c in offs} == {(16, 1), (65, 33)}
    ext = {0: [0, 0], 1: [0, 0]}
    sides = 0
    for c in offs:
        (ow, oh), (w, h), q = c["out"], c["src"], c["ints"]
        assert REPLICATE in c["edges"]
        pos = wm.positions(list(q), ow, oh)
        img = image(c["name"]).astype(np.int64)
        assert not np.array_equal(img[:, 0], img[:, -1]) and not np.array_equal(img[0], img[-1])
        v = values(c, REPLICATE)
        for ax in (0, 1):
            i0 = pos[2 * ax]
            ext[ax] = [min(ext[ax][0], int(i0.min())), max(ext[ax][1], int(i0.max()))]
        # where an index lies beyond int32: the value is the correct side's column / row / corner, from Python integers
        far = (np.abs(pos[0]) >= 1 << 31) | (np.abs(pos[2]) >= 1 << 31)
        ys, xs = np.nonzero(far)
        for Y, X in list(zip(ys.tolist(), xs.tolist()))[:: max(1, ys.size // 40)]:
            (ix, f_x), (iy, f_y) = pos_int(*q[:3], X, Y), pos_int(*q[3:], X, Y)
            cl = lambda i, n: min(max(i, 0), n - 1)
            xa, xb, ya, yb = cl(ix, w), cl(ix + 1, w), cl(iy, h), cl(iy + 1, h)
            if abs(ix) >= 1 << 31:
                assert xa == xb == (w - 1 if ix > 0 else 0)
            if abs(iy) >= 1 << 31:
                assert ya == yb == (h - 1 if iy > 0 else 0)
            for ch in range(c["ch"]):
                top = int(img[ya, xa, ch]) * (256 - f_x) + int(img[ya, xb, ch]) * f_x
                bot = int(img[yb, xa, ch]) * (256 - f_x) + int(img[yb, xb, ch]) * f_x
                assert int(v[ch, Y, X]) == top * (256 - f_y) + bot * f_y, (c["name"], X, Y)
            sides += 1
    for ax in (0, 1):
        assert ext[ax][0] < -(1 << 31) and ext[ax][1] >= 1 << 31, ext
    rep["first-tap index range"] = (ext[0], ext[1])
    rep["pixels beyond int32 checked"] = sides

    # ---- the clamp from both sides
    cl = [c for c in cs if c["group"] == "clamp"]
    for src in ((1, 1), (2, 1), (7, 5)):
        for ax in (0, 1):
            n = src[ax]
            for kind in ("unit", "limit"):
                got = set()
                for c in cl:
                    if (c["src"], c["axis"], c["kind"]) != (src, ax, kind):
                        continue
                    assert c["edges"] == BOTH and abs(c["ints"][4 * ax]) == (1 << 24 if kind == "unit" else 1 << 31)
                    pos = wm.positions(list(c["ints"]), *c["out"])
                    got |= set(zip(pos[2 * ax].reshape(-1).tolist(), pos[2 * ax + 1].reshape(-1).tolist()))
                    if kind == "limit":  # its other pixels are far beyond the clamp on both sides
                        assert pos[2 * ax].min() < -300 and pos[2 * ax].max() > 300
                want = {(i, f) for i in (-3, -2, -1, 0, n - 2, n - 1, n, n + 1) for f in CLAMP_FRACTIONS}
                assert want <= got, (src, ax, kind, sorted(want - got))

    # ---- floors of negatives
    fl = [c for c in cs if c["group"] == "floor"]
    for u, want in FLOORS:
        hit = [c for c in fl if c["u"] == u]
        assert {c["ints"][0] for c in hit} == {0, ONE}
        for c in hit:
            X, Y = c["at"]
            q = c["ints"]
            assert q[0] * X + q[1] * Y + q[2] == u and q[3] * X + q[4] * Y + q[5] == u
            assert pos_int(*q[:3], X, Y) == want and pos_int(*q[3:], X, Y) == want, (c["name"], pos_int(*q[:3], X, Y), want)
            pos = wm.positions(list(q), *c["out"])
            assert (int(pos[0][Y, X]), int(pos[1][Y, X]), int(pos[2][Y, X]), int(pos[3][Y, X])) == want + want

    # ---- degenerate matrices
    dg = {c["name"]: c["ints"] for c in cs if c["group"] == "degenerate"}
    assert dg["degenerate/zero"] == (0, 0, -(1 << 23), 0, 0, -(1 << 23))
    assert dg["degenerate/a0-b-limit"][:2] == (0, 1 << 31) and dg["degenerate/a-limit-e0"][0] == -(1 << 31) and dg["degenerate/a-limit-e0"][4] == 0

    # ---- the windows: valid shifted integers, every tap inside
    for c in cs:
        windows(c)

    # ---- the wrong variants
    caught, alive = surviving_mutants()
    assert not alive, f"no case tells these from the model: {alive}"
    assert set(caught) == {(name, edge) for name, (_, modes) in MUTANTS.items() for edge in modes}
    rep["mutants"] = caught
    rep["surviving mutants"] = len(alive)
    return rep


def windows(c):
    """[(frame, edge, window, shifted)] of a case, with the window's promises checked by brute force over the case's output
    pixels: every tap inside the frame lies in the window, under REPLICATE every clamped tap does"""
    res = []
    (ow, oh), q = c["out"], c["ints"]
    x0, _, y0, _ = wm.positions(list(q), ow, oh)
    for (fw, fh) in FRAMES:
        for edge in BOTH:
            win, sh = window_ints(q, fw, fh, ow, oh, edge)
            assert ints_valid(sh), (c["name"], fw, fh, edge, sh)
            for i0, lo, ln, n in ((x0, win[0], win[2], fw), (y0, win[1], win[3], fh)):
                for t in (i0, i0 + 1):
                    if edge == REPLICATE:
                        t = np.clip(t, 0, n - 1)
                        assert ln >= 1 and bool(((t >= lo) & (t < lo + ln)).all()), (c["name"], fw, fh, "replicate")
                    elif win[2] and win[3]:
                        t = t[(t >= 0) & (t < n)]
                        assert bool(((t >= lo) & (t < lo + ln)).all()), (c["name"], fw, fh, "fill")
            if edge == FILL and not (win[2] and win[3]):  # an empty window: no pixel has a tap inside on both axes
                both = ((x0 >= -1) & (x0 < fw) & (y0 >= -1) & (y0 < fh))
                assert not both.any(), (c["name"], fw, fh, "an empty window, but a tap inside")
            res.append(((fw, fh), edge, win, sh))
    return res


# ---- limit matrices against a decoded frame -----------------------------------------------------------------------------------
def frame_cases(W, H):
    """[(name, (out_w, out_h), matrix, kind)] for the plane and file calls on a W x H frame (both at least 16).  kind "few": an
    entry at the limit, one output pixel lands in a corner region of the frame and its neighbour 128 pixels outside, so the
    window is a few pixels in both edge modes.  kind "whole": all four entries at the limit, one diagonal of pixels inside, the window the whole frame.  The others lie
    beyond int32: FILL sees nothing (an empty window, the output all fill), REPLICATE collapses to one "corner", one edge
    "column" or one edge "row"."""
    L = LIN_MAX
    return [("few-left", (2, 3), (L, 0.0, 2.7 - L * 1.5, 0.0, 1.0, 10.25), "few"),
            ("few-top", (3, 2), (1.0, 0.0, 20.5, 0.0, -L, 3.6 + L * 0.5), "few"),
            ("few-bottom-right", (2, 2), (L, 0.0, W - 2.6 - L * 0.5, 0.0, L, H - 2.3 - L * 0.5), "few"),
            ("whole", (9, 5), (L, -L, W / 2 + 0.3 - L * 4.5 + L * 2.5, -LIN_ODD, L, H / 2 - 0.4 + LIN_ODD * 4.5 - L * 2.5), "whole"),
            ("far-bottom-right", (9, 5), (1.0, 0.0, OFF_MAX, 0.0, L, OFF_MAX), "corner"),
            ("far-top-left", (9, 5), (-L, 0.0, -OFF_MAX, 0.0, 1.0, -OFF_INT), "corner"),
            ("far-top-right", (9, 5), (L, L, OFF_INT, -L, -L, -OFF_MAX), "corner"),
            ("far-left", (9, 5), (0.0, 0.0, -OFF_MAX, 0.0, 2.0, 30.0), "column"),
            ("far-right", (9, 5), (L, 0.0, OFF_MAX, 0.0, 0.5, 7.25), "column"),
            ("far-below", (9, 5), (1.5, 0.0, 10.0, 0.0, L, OFF_MAX), "row"),
            ("far-above", (9, 5), (-1.0, 0.25, W - 8.0, 0.0, 0.0, -OFF_INT), "row")]


def assert_frame_cases(W, H):
    """the windows of frame_cases are what its docstring says, from Python integers"""
    seen = set()
    for name, (ow, oh), m, kind in frame_cases(W, H):
        q = fixed_ints(m)
        assert wm.fixed(m) == q, name
        fill, rep = window_ints(q, W, H, ow, oh, FILL)[0], window_ints(q, W, H, ow, oh, REPLICATE)[0]
        x0, _, y0, _ = wm.positions(q, ow, oh)
        if kind == "few":
            assert fill == rep and 2 <= fill[2] <= 5 and 2 <= fill[3] <= 5, (name, fill, rep)
            assert max(abs(v) for v in (q[0], q[4])) == 1 << 31
        elif kind == "whole":
            assert fill == rep == (0, 0, W, H) and min(abs(q[k]) for k in (0, 1, 3, 4)) >= (1 << 31) - 1, (name, fill, rep)
            assert 1 <= ((x0 >= 0) & (x0 < W - 1) & (y0 >= 0) & (y0 < H - 1)).sum() <= min(ow, oh)
        else:
            assert fill == (0, 0, 0, 0), (name, fill)
            assert max(int(np.abs(x0).max()), int(np.abs(y0).max())) >= 1 << 31, name
            want = {"corner": rep[2] == 1 and rep[3] == 1 and rep[0] in (0, W - 1) and rep[1] in (0, H - 1),
                    "column": rep[2] == 1 and rep[3] > 1 and rep[0] in (0, W - 1), "row": rep[3] == 1 and rep[2] > 1 and rep[1] in (0, H - 1)}
            assert want[kind], (name, rep)
            seen.add((kind, rep[0] if kind != "row" else None, rep[1] if kind != "column" else None))
    assert len(seen) == 7, seen
