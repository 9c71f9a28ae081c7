"""CPU: the antialiased resize (ZJ_RESIZE_BILINEAR_AA) -- the numpy model of the definition
(tests/resize_aa_model.py) against its own properties and torch's F.interpolate(antialias=True), the kernel's arithmetic
(zune-jpeg_amd/csrc/zj_resize_aa.h, built by g++ as tests/emu_resize_aa) against the model bit for bit, and the argument
checks of the filtered entry points (no GPU needed)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import emu_resize_aa_c as ea
import resize_aa_model as am
import resize_model as rm

AXES = [(1, 1), (1, 7), (7, 1), (2, 3), (224, 224), (8192, 8192), (300, 299), (100, 224), (37, 8192), (4096, 224),
        (4095, 1), (65535, 1), (65535, 8192), (65535, 224), (1, 8192), (5, 2)]


@pytest.mark.parametrize("n,m", AXES)
def test_model_weights_are_non_negative_and_sum_to_2_14(n, m):
    j, w = am.taps(n, m)
    assert (w >= 0).all() and (w.sum(axis=1) == 1 << 14).all()
    assert (j >= 0).all() and (j < n).all()
    if n == m:  # the identity: one tap of 2^14 on j = i
        assert np.array_equal(j[w > 0], np.arange(n)) and (w[w > 0] == 1 << 14).all()


@pytest.mark.parametrize("n,m", AXES)
def test_emulated_taps_match_the_model(n, m):
    j, w = am.taps(n, m)
    for i in sorted({0, 1 % m, m // 3, m // 2, m - 1}):
        lo, we = ea.weights(i, n, m)
        dense = np.zeros(n, np.int64)
        np.add.at(dense, j[i], w[i])
        assert dense[:lo].sum() == 0 and dense[lo + len(we):].sum() == 0, (i, lo)
        assert np.array_equal(dense[lo:lo + len(we)], we), i


def test_identity_windows_give_the_crop():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (3, 33, 57), dtype=np.uint8)
    assert np.array_equal(am.resize(img, 57, 33, rm.U8), img)
    for dt in (rm.F32, rm.F16, rm.BF16):
        exp = np.ascontiguousarray(rm.resize(img, 57, 33, dt, [0.01] * 3, [-1.0] * 3))
        assert np.array_equal(am.resize(img, 57, 33, dt, [0.01] * 3, [-1.0] * 3).view(np.uint8), exp.view(np.uint8))


@pytest.mark.parametrize("src,dst,kind", [((4096, 3000), (224, 224), "noise"), ((300, 200), (299, 201), "noise"),
                                          ((100, 150), (224, 300), "noise"), ((640, 480), (224, 224), "smooth"),
                                          ((2000, 1500), (101, 99), "smooth"), ((4480, 1000), (224, 50), "noise"),
                                          ((224, 224), (224, 224), "noise"), ((2000, 2000), (1, 1), "noise"),
                                          ((37, 23), (224, 224), "smooth"), ((1000, 50), (99, 101), "noise")])
def test_model_is_torch_antialiased_bilinear(src, dst, kind):
    """within 0.05 grey levels of F.interpolate(bilinear, align_corners=False, antialias=True) on the same u8 image"""
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    rng = np.random.default_rng(src[0] * 7 + dst[1])
    if kind == "noise":
        img = rng.integers(0, 256, (3, src[1], src[0]), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:src[1], 0:src[0]]
        img = np.stack([127.5 + 127 * np.sin(xx / (17.0 + 5 * c) + yy / (23.0 + 3 * c)) for c in range(3)]).astype(np.uint8)
    got = am.values(img, dst[0], dst[1]).astype(np.float64) / 65536
    ref = F.interpolate(torch.from_numpy(img.astype(np.float32))[None], size=(dst[1], dst[0]), mode="bilinear",
                        align_corners=False, antialias=True)[0].double().numpy()
    err = np.abs(got - ref).max()
    assert err <= 0.05, err
    if src == dst:
        assert err == 0


def _images(rng, sizes, channels, chw, pad=0):
    """random images in their own layout at a pitch (pad bytes after each row), plus their [C, h, w] form"""
    bufs, pitches, chws = [], [], []
    for (w, h) in sizes:
        img = rng.integers(0, 256, (channels, h, w), dtype=np.uint8)
        if channels == 3 and not chw:
            rows = img.transpose(1, 2, 0).reshape(h, w * 3)
        elif channels == 3:
            rows = img.reshape(3 * h, w)
        else:
            rows = img.reshape(h, w)
        pitch = rows.shape[1] + pad
        buf = np.full((rows.shape[0], pitch), 0xEE, np.uint8)
        buf[:, :rows.shape[1]] = rows
        bufs.append(np.ascontiguousarray(buf).reshape(-1))
        pitches.append(pitch)
        chws.append(img)
    return bufs, pitches, chws


CASES = [(c, chw, dt, lay) for c in (1, 3) for chw in ((False, True) if c == 3 else (False,)) for dt in range(4)
         for lay in ("NCHW", "NHWC")]


def _check(got, exp, dtype, what):
    if dtype == rm.F32:
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), what
    else:
        assert np.array_equal(got, exp), what


@pytest.mark.parametrize("channels,chw,dtype,layout", CASES)
def test_emulated_kernel_matches_the_model(channels, chw, dtype, layout):
    """sizes whose source spans need several LDS pieces (wider than 682 RGB / 680 CHW / 2048 grey pixels), odd pitches,
    flips, up- and downscales"""
    rng = np.random.default_rng(31 + 10 * channels + 3 * dtype + chw)
    sizes = [(37, 23), (1500, 40), (5, 301), (1, 1), (2600, 3), (13, 64)]
    bufs, pitches, chws = _images(rng, sizes, channels, chw, pad=5)
    flips = [False, True, True, False, True, False]
    scale = rng.uniform(0.002, 0.03, channels).astype(np.float32)
    bias = rng.uniform(-3, 3, channels).astype(np.float32)
    s, b = rm.factors(channels, scale, bias)
    for (ow, oh) in [(70, 9), (19, 7), (1, 1), (3, 130)]:
        out = ea.resize(bufs, sizes, pitches, channels, chw, ow, oh, dtype, layout == "NHWC", s, b, flips)
        got = rm.raw_view(out, dtype).reshape(len(sizes), -1)
        for i, img in enumerate(chws):
            exp = am.resize(img, ow, oh, dtype, scale, bias, flips[i], layout).reshape(-1)
            _check(got[i], exp, dtype, (i, sizes[i], ow, oh))


@pytest.mark.parametrize("n,m", [(65535, 1), (65535, 8192), (1, 8192), (3000, 130)])
def test_emulated_kernel_over_the_whole_axis_ranges(n, m):
    """one row / one column of a source length n to a destination length m (65535 -> 1: the tap count has no maximum)"""
    rng = np.random.default_rng(n + m)
    for horizontal in (True, False):
        size = (n, 2) if horizontal else (2, n)
        bufs, pitches, chws = _images(rng, [size], 1, False, pad=3)
        out_wh = (m, 1) if horizontal else (1, m)
        s, b = rm.factors(1, [1.0], [0.0])
        out = ea.resize(bufs, [size], pitches, 1, False, out_wh[0], out_wh[1], rm.F32, False, s, b, [horizontal])
        exp = am.resize(chws[0], out_wh[0], out_wh[1], rm.F32, [1.0], [0.0], horizontal)
        _check(out, exp.reshape(-1), rm.F32, (n, m, horizontal))


def test_emulated_identity_is_the_bilinear_output():
    rng = np.random.default_rng(8)
    for chw in (False, True):
        bufs, pitches, chws = _images(rng, [(57, 33), (1000, 3)], 3, chw, pad=3)
        s, b = rm.factors(3, [0.004] * 3, [-2.0] * 3)
        for sz, buf, p, img in zip([(57, 33), (1000, 3)], bufs, pitches, chws):
            out = ea.resize([buf], [sz], [p], 3, chw, sz[0], sz[1], rm.BF16, False, s, b)
            assert np.array_equal(out.view(np.uint16), rm.resize(img, sz[0], sz[1], rm.BF16, [0.004] * 3, [-2.0] * 3).reshape(-1))


@pytest.fixture(scope="module")
def zj():
    m = importlib.import_module("zune-jpeg_amd")
    if not os.path.exists(m.lib_path()):
        import __graft_entry__ as g
        g.build()
    return m


def test_filtered_entry_points_reject_bad_arguments_without_a_gpu(zj):
    L = zj.lib()
    ERR_ARG = -1
    assert (zj.RESIZE_BILINEAR, zj.RESIZE_BILINEAR_AA) == (0, 1)
    qt = np.ones((3, 64), np.int32)
    d = zj.FrameDesc.make(256, 128, 2, 2, 3, zj.ColorSpace.RGB, [qt[0], qt[1], qt[2]])
    buf = np.zeros(64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    ptrs = (C.c_void_p * 1)(p)
    wh = (C.c_uint * 2)(8, 8)
    sc = (C.c_float * 3)(1.0, 1.0, 1.0)
    win = (C.c_uint * 4)(0, 0, 8, 8)
    for f in (0, 1, 2, -1):
        assert L.zj_resize_filtered_device(None, 1, ptrs, wh, None, 3, 0, 4, 4, 2, 0, sc, sc, None, f, p, None) == ERR_ARG
        assert L.zj_decode_crops_resized_filtered_device(None, C.byref(d), 1, ptrs, ptrs, ptrs, win, 4, 4, 2, 0, sc, sc, None,
                                                         f, p, None) == ERR_ARG
        assert L.zj_decoder_finish_pixels_resized_crop_filtered_device(None, None, 0, 0, 8, 8, 4, 4, 2, 0, sc, sc, 0, f, p,
                                                                       1 << 20, None) == ERR_ARG
    dec = zj.Decoder()
    with pytest.raises(Exception):
        dec.finish_pixels_resized_crop_device(0, 0, 8, 8, 4, 4, zj.DTYPE_BF16, zj.TENSOR_NCHW, buf.ctypes.data, 1 << 20,
                                              antialias=True)
