"""CPU: the numpy definition of EXIF orientation (tests/orient_model.py) against Pillow's transpose operations, the window
rule against the pixel rule, and the library's zj_oriented_size / zj_orient_window against the model."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import orient_model as om

PIL_OPS = {2: "FLIP_LEFT_RIGHT", 3: "ROTATE_180", 4: "FLIP_TOP_BOTTOM", 5: "TRANSPOSE", 6: "ROTATE_270", 7: "TRANSVERSE",
           8: "ROTATE_90"}


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.mark.parametrize("shape", [(7, 5, 3), (5, 7, 3), (6, 11), (11, 6)])
def test_model_is_pillows_transpose(shape):
    from PIL import Image
    S = np.random.default_rng(3).integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(om.orient(S, 1), S)
    for o, name in PIL_OPS.items():
        exp = np.asarray(Image.fromarray(S).transpose(getattr(Image.Transpose, name)))
        got = om.orient(S, o)
        assert got.shape == exp.shape and np.array_equal(got, exp), (o, name)
        assert got.shape[:2][::-1] == om.oriented_size(o, shape[1], shape[0])


def test_orienting_the_stored_window_is_the_displayed_window():
    W, H = 7, 5
    S = np.arange(H * W * 3, dtype=np.uint8).reshape(H, W, 3)
    for o in range(1, 9):
        D = om.orient(S, o)
        dw, dh = om.oriented_size(o, W, H)
        n = 0
        for x, y in itertools.product(range(dw), range(dh)):
            for w, h in itertools.product(range(1, dw - x + 1), range(1, dh - y + 1)):
                sx, sy, sw, sh = om.stored_window(o, W, H, (x, y, w, h))
                assert 0 <= sx and sx + sw <= W and 0 <= sy and sy + sh <= H
                assert np.array_equal(om.orient(S[sy:sy + sh, sx:sx + sw], o), D[y:y + h, x:x + w]), (o, x, y, w, h)
                n += 1
        assert n == (dw * (dw + 1) // 2) * (dh * (dh + 1) // 2)


def test_library_geometry_is_the_model(zj):
    L = zj.lib()
    for o in range(1, 9):
        for w, h in ((1, 1), (7, 5), (5, 7), (65535, 3), (96, 80)):
            assert zj.oriented_size(o, w, h) == om.oriented_size(o, w, h)
    W, H = 7, 5
    for o in range(1, 9):
        dw, dh = om.oriented_size(o, W, H)
        for x, y, w, h in itertools.product(range(dw + 1), range(dh + 1), range(0, dw + 2), range(0, dh + 2)):
            exp = om.stored_window(o, W, H, (x, y, w, h))
            win, st = (C.c_uint * 4)(x, y, w, h), (C.c_uint * 4)()
            rc = L.zj_orient_window(o, W, H, win, st)
            assert (rc == 0 and tuple(st) == exp) if exp is not None else rc == -1, (o, x, y, w, h)
    a, b = C.c_uint(9), C.c_uint(9)
    for o in (0, 9, -1, 256 + 6):
        assert L.zj_oriented_size(o, 4, 3, C.byref(a), C.byref(b)) == -1
        assert L.zj_orient_window(o, 4, 3, (C.c_uint * 4)(0, 0, 1, 1), (C.c_uint * 4)()) == -1
    # the issue's own case: 96 x 80 stored, o = 6 (displayed 80 x 96), x + w = 90 is inside the stored width only
    assert L.zj_orient_window(6, 96, 80, (C.c_uint * 4)(60, 0, 30, 10), (C.c_uint * 4)()) == -1
    assert L.zj_orient_window(6, 96, 80, (C.c_uint * 4)(2**32 - 5, 0, 10, 10), (C.c_uint * 4)()) == -1  # (no wrap-around)
    assert L.zj_orient_window(1, 4, 3, None, (C.c_uint * 4)()) == -1
