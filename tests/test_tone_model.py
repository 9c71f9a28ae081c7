"""CPU: the numpy model of the tone stage (tests/tone_model.py) pinned to Pillow's ImageOps with exact
equality -- equalize, autocontrast, posterize, solarize, invert on RGB and L images: random, flat, two-valued, fewer than 255
pixels outside the last bin (equalize's step 0), a bin in use whose quotient passes 255 (point()'s clipping), every posterize
bits value, the solarize thresholds at both ends."""
import numpy as np
import pytest
from PIL import Image, ImageOps

import tone_model as tm


def images():
    rng = np.random.default_rng(11)
    out = {}
    out["random_rgb"] = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    out["random_l"] = rng.integers(0, 256, (41, 29), dtype=np.uint8)
    out["narrow_rgb"] = rng.integers(60, 190, (30, 31, 3), dtype=np.uint8)
    out["flat_rgb"] = np.full((16, 17, 3), (9, 200, 255), np.uint8)
    out["flat_l"] = np.full((5, 9), 128, np.uint8)
    two = np.where(rng.random((24, 25, 1)) < 0.3, np.array([10, 0, 254], np.uint8), np.array([240, 255, 255], np.uint8)).astype(np.uint8)
    out["two_values_rgb"] = two
    out["two_values_l"] = np.where(rng.random((19, 23)) < 0.5, 3, 250).astype(np.uint8)
    # fewer than 255 pixels outside the last non-empty bin: step 0, the identity
    few = np.full((40, 40), 222, np.uint8)
    few.reshape(-1)[:254] = rng.integers(0, 222, 254)
    out["step_zero_l"] = few
    few3 = np.full((40, 40, 3), 250, np.uint8)
    few3.reshape(-1, 3)[:100] = rng.integers(0, 250, (100, 3))
    out["step_zero_rgb"] = few3
    # 509 pixels outside the last bin: step 1, the last bin's quotient 509; 764: step 2, quotient 382
    for name, outside in (("quotient_509_l", 509), ("quotient_382_l", 764)):
        a = np.full((64, 64), 251, np.uint8)
        a.reshape(-1)[:outside] = rng.integers(0, 200, outside)
        out[name] = a
    a = np.full((64, 64, 3), 251, np.uint8)
    a.reshape(-1, 3)[:509] = rng.integers(0, 200, (509, 3))
    out["quotient_509_rgb"] = a
    ramp = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    out["ramp_l"] = ramp
    out["dark_rgb"] = (rng.integers(0, 256, (33, 35, 3)) ** 2 // 700).astype(np.uint8)
    return out


IMAGES = images()


def pil(a):
    return Image.fromarray(a, "L" if a.ndim == 2 else "RGB")


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_equalize_is_pillows(name):
    a = IMAGES[name]
    assert np.array_equal(tm.apply(tm.EQUALIZE, 0, a), np.asarray(ImageOps.equalize(pil(a))))


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_autocontrast_is_pillows(name):
    a = IMAGES[name]
    assert np.array_equal(tm.apply(tm.AUTOCONTRAST, 0, a), np.asarray(ImageOps.autocontrast(pil(a))))


@pytest.mark.parametrize("bits", range(1, 9))
def test_posterize_is_pillows(bits):
    for name in ("random_rgb", "random_l", "ramp_l"):
        a = IMAGES[name]
        assert np.array_equal(tm.apply(tm.POSTERIZE, bits, a), np.asarray(ImageOps.posterize(pil(a), bits)))


@pytest.mark.parametrize("threshold", [0, 1, 128, 255, 256])
def test_solarize_is_pillows(threshold):
    for name in ("random_rgb", "random_l", "ramp_l"):
        a = IMAGES[name]
        assert np.array_equal(tm.apply(tm.SOLARIZE, threshold, a), np.asarray(ImageOps.solarize(pil(a), threshold)))


def test_invert_and_identity():
    for name in ("random_rgb", "random_l", "ramp_l"):
        a = IMAGES[name]
        assert np.array_equal(tm.apply(tm.INVERT, 0, a), np.asarray(ImageOps.invert(pil(a))))
        assert np.array_equal(tm.apply(tm.IDENTITY, 0, a), a)


def test_the_histogram_is_pillows_in_both_layouts():
    for name, a in IMAGES.items():
        want = np.asarray(pil(a).histogram(), np.int64).reshape(-1, 256)
        assert np.array_equal(tm.histogram(a), want), name
        if a.ndim == 3:
            chw = np.ascontiguousarray(a.transpose(2, 0, 1))
            assert np.array_equal(tm.histogram(chw, chw=True), want)
            assert np.array_equal(tm.apply(tm.EQUALIZE, 0, chw, chw=True), tm.apply(tm.EQUALIZE, 0, a).transpose(2, 0, 1))


def test_the_cases_take_the_branches_they_are_named_for():
    """the step-0 images have a step of 0, the quotient images a bin in use whose unclipped quotient is the one named"""
    def quotients(h):
        histo = [int(v) for v in h if v]
        step = (sum(histo) - histo[-1]) // 255
        n, q = step // 2, []
        for v in h:
            q.append(n // step if step else None)
            n += int(v)
        return step, [q[i] for i in range(256) if h[i]]
    assert quotients(tm.histogram(IMAGES["step_zero_l"])[0])[0] == 0
    assert all(quotients(h)[0] == 0 for h in tm.histogram(IMAGES["step_zero_rgb"]))
    assert quotients(tm.histogram(IMAGES["quotient_509_l"])[0]) [1][-1] == 509
    assert quotients(tm.histogram(IMAGES["quotient_382_l"])[0])[1][-1] == 382
    cases = tm.equalize_cases()
    assert quotients(cases["quotient_509"])[1][-1] == 509 and quotients(cases["quotient_382"])[1][-1] == 382
    assert quotients(cases["step_zero"])[0] == 0 and quotients(cases["step_one"])[0] == 1
    for name in ("sum_65535_squared", "sum_65535_squared_spread"):
        h = cases[name]
        assert sum(h) == 65535 ** 2 and max(h) < 2 ** 32
        step = (sum(h) - h[255]) // 255
        assert step // 2 + sum(h) - h[255] >= 2 ** 32, "the running n must pass 32 bits"


def test_the_synthetic_equalize_cases_equal_pillows_rule_on_an_image_where_one_exists():
    """the cases small enough to be an image: built as one, equalized by Pillow, equal to the table from the bins"""
    for name, h in tm.equalize_cases().items():
        if sum(h) == 0 or sum(h) > 1 << 21:
            continue
        a = np.repeat(np.arange(256, dtype=np.uint8), h)
        a = np.concatenate([a, np.full((-a.size) % 64, a[-1], np.uint8)]) if a.size % 64 else a
        hh = tm.histogram(a.reshape(-1, 64))[0]
        got = tm.table(tm.EQUALIZE, 0, hh)[a]
        assert np.array_equal(got.reshape(-1, 64), np.asarray(ImageOps.equalize(pil(a.reshape(-1, 64))))), name


def test_every_lo_hi_pair_of_autocontrast_equals_pillow_on_a_two_pixel_image():
    """all 32 640 pairs: Pillow's own doubles on the image (lo, hi)"""
    for lo, hi in tm.autocontrast_pairs()[::37]:
        a = np.array([[lo, hi]], np.uint8)
        t = tm.table(tm.AUTOCONTRAST, 0, tm.two_bin_hist(lo, hi))
        assert np.array_equal(t[a], np.asarray(ImageOps.autocontrast(pil(a))))
        assert t[lo] == 0 and t[hi] in (254, 255)


def test_the_argument_rule():
    ok = [(0, 0), (1, 0), (2, 1), (2, 8), (3, 0), (3, 256), (4, 0), (5, 0)]
    bad = [(-1, 0), (6, 0), (0, 1), (1, 5), (2, 0), (2, 9), (3, -1), (3, 257), (4, 1), (5, -1)]
    assert all(tm.valid(*c) for c in ok) and not any(tm.valid(*c) for c in bad)
