"""CPU: the bicubic antialiased resize (ZJ_RESIZE_BICUBIC_AA) -- the kernel's arithmetic and phases
(zune-jpeg_amd/csrc/zj_resize_bicubic.h, built by g++ as tests/emu_resize_bicubic) against the numpy model of the definition
(tests/resize_bicubic_model.py) bit for bit, and the argument checks of the filtered entry points and of the Python
keywords (no GPU needed)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import emu_resize_bicubic_c as eb
import resize_bicubic_model as bm
import resize_model as rm
from test_resize_aa_emu import CASES, _check, _images

AXES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 5), (8, 4), (9, 4), (64, 224), (224, 64), (500, 224), (4096, 224),
        (65535, 1), (65535, 8192), (1, 8192)]
_EXPECTED = {}


def expected(img, ow, oh):
    """the model's v of one image and size, computed once and shared (read-only) by the dtype / layout cases"""
    key = (img.tobytes(), img.shape, ow, oh)
    if key not in _EXPECTED:
        v = bm.values(img, ow, oh)
        v.setflags(write=False)
        _EXPECTED[key] = v
    return _EXPECTED[key]


def model_output(img, ow, oh, dtype, scale, bias, flip, layout):
    """bm.resize from the shared v"""
    v = expected(img, ow, oh)
    v = v[:, :, ::-1] if flip else v
    c = img.shape[0]
    if dtype == rm.U8:
        out = ((v + 32768) >> 16).astype(np.uint8)
    else:
        s, b = rm.factors(c, scale, bias)
        y = ((v.astype(np.float32) * s[:, None, None]).astype(np.float32) + b[:, None, None]).astype(np.float32)
        if dtype == rm.F32:
            out = y
        elif dtype == rm.F16:
            with np.errstate(over="ignore"):
                out = y.astype(np.float16).view(np.uint16)
        else:
            out = rm.bf16_bits(y)
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if layout == "NHWC" else np.ascontiguousarray(out)


def test_model_output_helper_is_the_model():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (3, 9, 14), dtype=np.uint8)
    for dt in range(4):
        for lay in ("NCHW", "NHWC"):
            a = model_output(img, 5, 11, dt, [0.01] * 3, [-1.0] * 3, True, lay)
            assert np.array_equal(a.view(np.uint8), bm.resize(img, 5, 11, dt, [0.01] * 3, [-1.0] * 3, True, lay).view(np.uint8))


@pytest.mark.parametrize("n,m", AXES)
def test_emulated_taps_match_the_model(n, m):
    j, w, S = bm.taps(n, m)
    for i in sorted({0, 1 % m, m // 3, m // 2, m - 1}):
        lo, we, Se = eb.weights(i, n, m)
        dense = np.zeros(n, np.int64)
        np.add.at(dense, j[i], w[i])
        assert Se == S[i]
        assert dense[:lo].sum() == 0 and dense[lo + len(we):].sum() == 0, (i, lo)
        assert np.array_equal(dense[lo:lo + len(we)], we), i


def test_floor_division_below_zero():
    R = eb.lib().zjeb_R
    assert [R(-1, 1 << 30), R(0, 1 << 30), R(1 << 30, 1 << 30), R(-(1 << 16), 1 << 30), R(-(1 << 15) - 1, 1 << 30)] == \
        [0, 0, 1 << 14, -1 + 0, -1]
    for Cp, S in [(-123456789, 987654321), (-(1 << 47), (1 << 46) + 12345), (5, 7), (-5, 7), (-4, 7), (-3, 7)]:
        assert R(Cp, S) == (Cp * (1 << 14) + S // 2) // S


def test_lds_leaves_room_for_four_workgroups():
    assert 4 * eb.lib().zjeb_lds_bytes() <= 160 * 1024  # (a CU's LDS)


# source widths at the pieces' boundaries: 340 CHW / 341 RGB / 1024 grey pixels per piece here, and the triangle kernel's
# 680 / 682 / 2048; heights that stay small.  Output widths at the block's 64 columns, heights at its 4 rows.
WIDTHS = [1, 2, 3, 63, 64, 65, 340, 341, 342, 682, 683, 1024, 1025, 2049]
OUTS = [(1, 1), (7, 3), (8, 4), (9, 5), (64, 2), (65, 1)]


@pytest.mark.parametrize("channels,chw,dtype,layout", CASES)
def test_emulated_kernel_matches_the_model(channels, chw, dtype, layout):
    rng = np.random.default_rng(77 + channels + chw)  # (the same images for every dtype and layout: one model run each)
    sizes = [(w, 1 + (k % 3)) for k, w in enumerate(WIDTHS)] + [(37, 23), (5, 301)]
    bufs, pitches, chws = _images(rng, sizes, channels, chw, pad=5)
    flips = [bool(k % 2) for k in range(len(sizes))]
    scale = np.array([0.0039, 0.011, 0.027][:channels], np.float32)
    bias = np.array([-0.5, 1.25, -2.75][:channels], np.float32)
    s, b = rm.factors(channels, scale, bias)
    for (ow, oh) in OUTS:
        out = eb.resize(bufs, sizes, pitches, channels, chw, ow, oh, dtype, layout == "NHWC", s, b, flips)
        got = rm.raw_view(out, dtype).reshape(len(sizes), -1)
        for i, img in enumerate(chws):
            exp = model_output(img, ow, oh, dtype, scale, bias, flips[i], layout).reshape(-1)
            _check(got[i], exp, dtype, (i, sizes[i], ow, oh))


@pytest.mark.parametrize("size,out", [((65535, 1), (1, 1)), ((1, 65535), (1, 1)), ((3, 3), (33, 17)), ((3000, 2), (130, 1)),
                                      ((2, 700), (1, 9))])
def test_emulated_kernel_over_the_axis_ranges(size, out):
    """65535 -> 1 in either axis (the tap count has no maximum: 1024 windows of 256 row taps, 64 pieces of columns), an
    enlargement, and several pieces / windows with carries between them"""
    rng = np.random.default_rng(size[0] + out[0])
    for channels in ((1, 3) if max(size) < 65535 else (1,)):
        bufs, pitches, chws = _images(rng, [size], channels, False, pad=3)
        s, b = rm.factors(channels, [1.0] * channels, [0.0] * channels)
        for flip in (False, True):
            got = eb.resize(bufs, [size], pitches, channels, False, out[0], out[1], rm.F32, False, s, b, [flip])
            exp = model_output(chws[0], out[0], out[1], rm.F32, [1.0] * channels, [0.0] * channels, flip, "NCHW")
            _check(got, exp.reshape(-1), rm.F32, (size, out, flip))


def test_emulated_clamp_engages_under_the_negative_lobes():
    img = np.zeros((1, 4, 64), np.uint8)
    img[:, :, 1::2] = 255
    s, b = rm.factors(1, [1.0], [0.0])
    clamped = []
    out = eb.resize([img.reshape(-1)], [(64, 4)], [64], 1, False, 224, 4, rm.U8, False, s, b, clamped=clamped)
    v = bm.passes(img, 224, 4)[2]
    assert clamped == [int((v < 0).sum()), int((v > bm.V_MAX).sum())] and min(clamped) > 0
    assert np.array_equal(out, bm.resize(img, 224, 4, rm.U8).reshape(-1)) and out.min() == 0 and out.max() == 255


def test_emulated_identity_is_the_crop():
    rng = np.random.default_rng(8)
    for chw in (False, True):
        sizes = [(57, 33), (1000, 3)]
        bufs, pitches, chws = _images(rng, sizes, 3, chw, pad=3)
        s, b = rm.factors(3, [1.0] * 3, [0.0] * 3)
        for sz, buf, p, img in zip(sizes, bufs, pitches, chws):
            out = eb.resize([buf], [sz], [p], 3, chw, sz[0], sz[1], rm.U8, False, s, b)
            assert np.array_equal(out, img.reshape(-1))


@pytest.fixture(scope="module")
def zj():
    m = importlib.import_module("zune-jpeg_amd")
    if not os.path.exists(m.lib_path()):
        import __graft_entry__ as g
        g.build()
    return m


def test_filtered_entry_points_reject_bad_arguments_without_a_gpu(zj):
    """filter 4 with otherwise bad arguments (no context), and the values that are no filter, are ZJ_ERR_ARG"""
    L = zj.lib()
    ERR_ARG = -1
    assert zj.RESIZE_BICUBIC_AA == 4
    qt = np.ones((3, 64), np.int32)
    d = zj.FrameDesc.make(256, 128, 2, 2, 3, zj.ColorSpace.RGB, [qt[0], qt[1], qt[2]])
    buf = np.zeros(64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    ptrs = (C.c_void_p * 1)(p)
    wh = (C.c_uint * 2)(8, 8)
    sc = (C.c_float * 3)(1.0, 1.0, 1.0)
    win = (C.c_uint * 4)(0, 0, 8, 8)
    ori = (C.c_uint8 * 1)(1)
    for f in (4, 2, 3, 5, -1):
        assert L.zj_resize_filtered_device(None, 1, ptrs, wh, None, 3, 0, 4, 4, 2, 0, sc, sc, None, f, p, None) == ERR_ARG
        assert L.zj_decode_crops_resized_filtered_device(None, C.byref(d), 1, ptrs, ptrs, ptrs, win, 4, 4, 2, 0, sc, sc, None,
                                                         f, p, None) == ERR_ARG
        assert L.zj_decode_crops_resized_prescaled_device(None, C.byref(d), 1, ptrs, ptrs, ptrs, win, 4, 4, 2, 0, sc, sc, None,
                                                          f, 1, p, None) == ERR_ARG
        assert L.zj_decode_crops_resized_oriented_device(None, C.byref(d), 1, ptrs, ptrs, ptrs, win, 4, 4, 2, 0, sc, sc, None,
                                                         f, 0, ori, p, None) == ERR_ARG
        assert L.zj_decoder_finish_pixels_resized_crop_filtered_device(None, None, 0, 0, 8, 8, 4, 4, 2, 0, sc, sc, 0, f, p,
                                                                       1 << 20, None) == ERR_ARG


def test_interpolation_keyword(zj):
    assert zj.resize_filter() == zj.RESIZE_BILINEAR and zj.resize_filter(True) == zj.RESIZE_BILINEAR_AA
    assert zj.resize_filter(True, "bicubic") == zj.RESIZE_BICUBIC_AA
    with pytest.raises(ValueError, match="antialias=True"):
        zj.resize_filter(False, "bicubic")
    with pytest.raises(ValueError, match="bilinear"):
        zj.resize_filter(True, "lanczos")
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    dec = zj.Decoder()
    buf = np.zeros(64, np.uint8)
    for bad in ({"interpolation": "bicubic"}, {"interpolation": "nearest", "antialias": True}):
        # (the keyword is checked before anything is decoded, allocated or launched)
        with pytest.raises(ValueError):
            dec.finish_pixels_resized_crop_device(0, 0, 8, 8, 4, 4, zj.DTYPE_BF16, zj.TENSOR_NCHW, buf.ctypes.data, 1 << 20, **bad)
        with pytest.raises(ValueError):
            zj.Context.resize_device(None, [0], [(8, 8)], 3, 0, 4, 4, 2, 0, 0, **bad)
        with pytest.raises(ValueError):
            zj.Context.decode_crops_resized_device(None, None, [0], [0], [0], [(0, 0, 8, 8)], 4, 4, 2, 0, 0, **bad)
        with pytest.raises(ValueError):
            tensors.resize_to_tensor(None, [], (4, 4), **bad)
        with pytest.raises(ValueError):
            tensors.decode_resized_crops_to_tensor(None, None, [], [], (4, 4), **bad)
    dec.close()
