"""CPU: the colour-matrix stage's definition (tests/color_model.py) -- zj_color_fixed, which runs without a
device, against the model's integers and its refusals at and just past each limit; the identity, the six channel orders and
Pillow's convert("L") exactly; tensors.color_matrix against Pillow's ImageEnhance and against the float64 affine map."""
import ctypes as C
import importlib
import itertools
import math
import os

import numpy as np
import pytest

import color_model as cm

ARG = -1
FACTORS = (0.0, 0.3, 0.6, 0.75, 1.0, 1.25, 1.4, 2.0)


@pytest.fixture(scope="module")
def zj():
    m = importlib.import_module("zune-jpeg_amd")
    if not os.path.exists(m.lib_path()):
        import __graft_entry__ as g
        g.build()
    return m


@pytest.fixture(scope="module")
def tensors():
    return importlib.import_module("zune-jpeg_amd.tensors")


def all_bytes():
    """every byte value in every channel, the channels out of step: [256, 3, 3]"""
    v = np.arange(256, dtype=np.uint8)
    return np.stack([np.stack([v, np.roll(v, 85), np.roll(v, 170)], -1), np.stack([v[::-1], v, np.roll(v, 7)], -1),
                     np.stack([np.roll(v, 128), v[::-1], v], -1)], 1)


def test_fixed_equals_the_models_integers(zj):
    rng = np.random.default_rng(17)
    for _ in range(300):
        m = rng.uniform(-1, 1, (3, 4)) * rng.choice([0.01, 1.0, 16.0]) * np.array([1, 1, 1, 256.0])
        assert zj.color_fixed(m) == cm.fixed(m)
    assert zj.color_fixed(cm.IDENTITY) == [65536, 0, 0, 0, 0, 65536, 0, 0, 0, 0, 65536, 0]
    assert zj.color_fixed(cm.GRAY) == [19595, 38470, 7471, 0] * 3
    # the rounding: floor(x + 1/2), halves up, negative values included
    for v, want in ((0.5 / 65536, 1), (-0.5 / 65536, 0), (-1.5 / 65536, -1), (1.49 / 65536, 1), (-0.51 / 65536, -1)):
        m = cm.IDENTITY.copy()
        m[1, 2] = v
        assert zj.color_fixed(m)[6] == want == cm.fixed(m)[6]


def test_fixed_refuses_at_its_limits(zj):
    L = zj.lib()
    q = (C.c_int32 * 12)()
    ident = (C.c_double * 12)(*cm.IDENTITY.reshape(-1))
    assert L.zj_color_fixed(None, q) == ARG and L.zj_color_fixed(ident, None) == ARG and L.zj_color_fixed(ident, q) == 0
    for k in range(12):
        lim = cm.OFF_MAX if k % 4 == 3 else cm.LIN_MAX
        for sign in (1.0, -1.0):
            m = cm.IDENTITY.reshape(-1).copy()
            m[k] = sign * lim
            got = zj.color_fixed(m)                       # at the limit: taken
            assert got == cm.fixed(m) and abs(got[k]) == int(lim) << 16
            m[k] = sign * math.nextafter(lim, math.inf)   # just past it
            assert cm.fixed(m) is None
            with pytest.raises(zj.ZjError) as e:
                zj.color_fixed(m)
            assert e.value.status == ARG
        for bad in (float("nan"), float("inf"), -float("inf")):
            m = cm.IDENTITY.reshape(-1).copy()
            m[k] = bad
            assert cm.fixed(m) is None
            with pytest.raises(zj.ZjError):
                zj.color_fixed(m)


def test_the_identity_and_the_six_channel_orders_are_exact(zj):
    img = all_bytes()
    for perm in itertools.permutations(range(3)):
        m = np.zeros((3, 4))
        for c, src in enumerate(perm):
            m[c, src] = 1.0
        assert np.array_equal(cm.apply_fixed(zj.color_fixed(m), img), img[..., list(perm)])
    assert np.array_equal(cm.apply(cm.BGR, img), img[..., ::-1])


def test_saturation_0_is_pillows_convert_l(zj, tensors):
    from PIL import Image
    img = cm.noise_image()
    m = tensors.color_matrix(grayscale=True)
    assert zj.color_fixed(m) == [19595, 38470, 7471, 0] * 3 == zj.color_fixed(tensors.color_matrix(saturation=0.0))
    got = cm.apply_fixed(zj.color_fixed(m), img)
    want = np.asarray(Image.fromarray(img).convert("L"))
    for c in range(3):
        assert np.array_equal(got[..., c], want)


@pytest.mark.parametrize("f", FACTORS)
def test_color_matrix_against_pillows_image_enhance(zj, tensors, f):
    from PIL import Image, ImageEnhance
    img = cm.noise_image()
    pil = Image.fromarray(img)
    diff = lambda m, enh: int(np.abs(cm.apply_fixed(zj.color_fixed(m), img).astype(int)
                                     - np.asarray(enh.enhance(f)).astype(int)).max())
    centre = int(np.asarray(pil.convert("L")).mean() + 0.5)   # Pillow's own
    assert diff(tensors.color_matrix(brightness=f), ImageEnhance.Brightness(pil)) <= 1
    assert diff(tensors.color_matrix(contrast=f, contrast_center=centre), ImageEnhance.Contrast(pil)) <= 1
    assert diff(tensors.color_matrix(saturation=f), ImageEnhance.Color(pil)) <= 2


def test_hue_0_and_1_are_the_identity(zj, tensors):
    ident = zj.color_fixed(cm.IDENTITY)
    assert zj.color_fixed(tensors.color_matrix()) == ident
    assert zj.color_fixed(tensors.color_matrix(hue=0.0)) == ident
    assert zj.color_fixed(tensors.color_matrix(hue=1.0)) == ident
    assert zj.color_fixed(tensors.color_matrix(hue=-1.0)) == ident


def test_gray_pixels_keep_their_value_under_saturation_and_hue(zj, tensors):
    g = np.arange(256, dtype=np.uint8)
    img = np.stack([g, g, g], -1)[None]
    for s in (0.0, 0.4, 1.0, 1.7, 3.0):
        for h in (0.0, 0.1, 0.25, 0.5, -0.3, 0.77):
            assert np.array_equal(cm.apply_fixed(zj.color_fixed(tensors.color_matrix(saturation=s, hue=h)), img), img), (s, h)


@pytest.mark.parametrize("hue", [0.1, 0.25, 0.5, -0.3])
def test_hue_is_within_1_of_the_float64_affine_map(zj, tensors, hue):
    img = cm.noise_image()
    m = tensors.color_matrix(hue=hue)
    got = cm.apply_fixed(zj.color_fixed(m), img)
    assert np.abs(got.astype(int) - cm.affine_f64(m, img).astype(int)).max() <= 1
    assert not np.array_equal(got, img)
    # a rotation of the I, Q plane: the luma of the unclamped map is the input's
    lin = m[:, :3]
    assert np.allclose(np.asarray(cm.LUMA) @ lin, cm.LUMA, atol=1e-6) and np.allclose(m[:, 3], 0, atol=1e-9)


def test_the_composition_order_and_bgr(tensors):
    """brightness, then contrast about the centre, then saturation, then hue, no clamp between; bgr swaps rows 0 and 2 last"""
    b, c, s, h, centre = 1.3, 0.7, 1.5, 0.15, 100.0
    x = np.array([200.0, 30.0, 90.0])
    step = lambda **kw: tensors.color_matrix(**kw)
    ap = lambda m, v: m[:, :3] @ v + m[:, 3]
    want = ap(step(hue=h), ap(step(saturation=s), ap(step(contrast=c, contrast_center=centre), ap(step(brightness=b), x))))
    m = step(brightness=b, contrast=c, saturation=s, hue=h, contrast_center=centre)
    assert m.shape == (3, 4) and m.dtype == np.float64
    assert np.allclose(ap(m, x), want, atol=1e-9)
    assert np.array_equal(step(brightness=b, contrast=c, saturation=s, hue=h, contrast_center=centre, bgr=True), m[::-1])
    assert np.array_equal(step(grayscale=True, saturation=5.0), step(saturation=0.0))
