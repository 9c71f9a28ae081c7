"""CPU: the resize kernel's arithmetic (zune-jpeg_amd/csrc/zj_resize.h, built by g++ as tests/emu_resize) against the numpy
model of the definition (tests/resize_model.py), the model against torch's bilinear interpolation, and the argument checks
of the resized entry points (no GPU needed)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import emu_resize_c as er
import resize_model as rm

NS = [1, 2, 3, 7, 224, 4095, 65535]
MS = [1, 2, 224, 8192]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_taps_match_the_model(n, m):
    i0, f, i1 = rm.taps(n, m)
    L = er.lib()
    got = np.array([L.zjer_tap(i, n, m) for i in range(m)], np.int64)
    assert np.array_equal(got & 0xFFFF, i0)
    assert np.array_equal((got >> 16) & 255, f)
    assert np.array_equal((got & 0xFFFF) + (got >> 24), i1)
    assert (i1 < n).all() and (i0 >= 0).all()


def test_taps_of_equal_lengths_are_the_identity():
    for n in (1, 2, 3, 224, 8192):
        i0, f, i1 = rm.taps(n, n)
        assert np.array_equal(i0, np.arange(n)) and not f.any()


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


@pytest.mark.parametrize("channels,chw,dtype,layout", CASES)
def test_emulated_kernel_matches_the_model(channels, chw, dtype, layout):
    rng = np.random.default_rng(17 + 10 * channels + 3 * dtype + chw)
    sizes = [(37, 23), (224, 224), (5, 301), (1, 1), (300, 2), (13, 64)]
    bufs, pitches, chws = _images(rng, sizes, channels, chw, pad=5)
    flips = [False, True, True, False, True, False]
    scale = rng.uniform(0.002, 0.03, channels).astype(np.float32)
    bias = rng.uniform(-3, 3, channels).astype(np.float32)
    s, b = rm.factors(channels, scale, bias)
    for (ow, oh) in [(224, 224), (19, 7), (1, 1), (64, 300)]:
        out = er.resize(bufs, sizes, pitches, channels, chw, ow, oh, dtype, layout == "NHWC", s, b, flips)
        got = rm.raw_view(out, dtype).reshape(len(sizes), -1)
        for i, img in enumerate(chws):
            exp = rm.resize(img, ow, oh, dtype, scale, bias, flips[i], layout).reshape(-1)
            if dtype == rm.F32:
                assert np.array_equal(got[i].view(np.uint32), exp.view(np.uint32)), (i, ow, oh)
            else:
                assert np.array_equal(got[i], exp), (i, ow, oh)


@pytest.mark.parametrize("n", NS)
def test_emulated_kernel_over_the_whole_axis_ranges(n):
    """one row / one column of every source length n to every destination length m"""
    rng = np.random.default_rng(n)
    for m in MS:
        for horizontal in (True, False):
            size = (n, 2) if horizontal else (2, n)
            bufs, pitches, chws = _images(rng, [size], 1, False)
            out_wh = (m, 1) if horizontal else (1, m)
            s, b = rm.factors(1, [1.0], [0.0])
            out = er.resize(bufs, [size], pitches, 1, False, out_wh[0], out_wh[1], rm.F32, False, s, b, [horizontal])
            exp = rm.resize(chws[0], out_wh[0], out_wh[1], rm.F32, [1.0], [0.0], horizontal)
            assert np.array_equal(out.view(np.uint32), exp.reshape(-1).view(np.uint32))


def test_conversions_match_numpy():
    rng = np.random.default_rng(5)
    L = er.lib()
    ys = np.concatenate([rng.normal(0, 3, 2000), rng.normal(0, 3e4, 500), [65504, 65519.99, 65520, 65536, 1e6, -70000, 6e-8,
                                                                           3e-8, 2.9e-8, 1e-5, -1e-6, 0.0, -0.0]]).astype(np.float32)
    with np.errstate(over="ignore"):
        f16 = ys.astype(np.float16).view(np.uint16)
    assert np.array_equal(np.array([L.zjer_f16(float(y)) for y in ys], np.uint16), f16)
    assert np.array_equal(np.array([L.zjer_bf16(float(y)) for y in ys], np.uint16), rm.bf16_bits(ys))
    vs = rng.integers(0, 255 * 65536 + 1, 3000)
    s, b = np.float32(0.0173 / 65536), np.float32(-2.1179)
    exp = ((vs.astype(np.float32) * s).astype(np.float32) + b).astype(np.float32)
    got = np.array([L.zjer_f32(int(v), float(s), float(b)) for v in vs], np.float32)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_f16_overflows_to_inf():
    rng = np.random.default_rng(9)
    bufs, pitches, chws = _images(rng, [(40, 30)], 3, False)
    chws[0][:, :4, :] = 255
    bufs[0].reshape(30, 120)[:4, :] = 255
    scale = [1000.0, -1000.0, 1.0]
    s, b = rm.factors(3, scale, [0.0, 0.0, 0.0])
    out = er.resize(bufs, [(40, 30)], pitches, 3, False, 32, 24, rm.F16, False, s, b)
    exp = rm.resize(chws[0], 32, 24, rm.F16, scale, [0, 0, 0])
    got = out.view(np.uint16).reshape(exp.shape)
    assert np.array_equal(got, exp)
    assert (got[0] == 0x7C00).any() and (got[1] == 0xFC00).any()


def test_identity_windows_give_the_crop():
    rng = np.random.default_rng(3)
    for chw in (False, True):
        bufs, pitches, chws = _images(rng, [(57, 33)], 3, chw, pad=3)
        mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
        scale = np.float32(1 / (255 * std))
        bias = np.float32(-mean / std)
        s, b = rm.factors(3, scale, bias)
        out = er.resize(bufs, [(57, 33)], pitches, 3, chw, 57, 33, rm.F32, False, s, b)
        got = out.view(np.float32).reshape(3, 33, 57)
        crop = chws[0].astype(np.float32) * np.float32(65536)
        exp = (crop * s[:, None, None]).astype(np.float32) + b[:, None, None]
        assert np.array_equal(got, exp)
        u8 = er.resize(bufs, [(57, 33)], pitches, 3, chw, 57, 33, rm.U8, True, s, b)
        assert np.array_equal(u8.reshape(33, 57, 3), chws[0].transpose(1, 2, 0))


@pytest.mark.parametrize("src,dst", [((37, 23), (224, 224)), ((640, 480), (224, 224)), ((224, 224), (224, 224)),
                                     ((1000, 50), (99, 101)), ((3, 3), (8, 8))])
def test_model_is_torch_bilinear_within_two_u8_units(src, dst):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    rng = np.random.default_rng(src[0] + dst[1])
    img = rng.integers(0, 256, (3, src[1], src[0]), dtype=np.uint8)
    y = rm.resize(img, dst[0], dst[1], rm.F32, [1.0] * 3, [0.0] * 3)
    t = F.interpolate(torch.from_numpy(img.astype(np.float32))[None], size=(dst[1], dst[0]), mode="bilinear",
                      align_corners=False, antialias=False)[0].numpy()
    assert np.abs(y - t).max() < 2.0


@pytest.fixture(scope="module")
def zj():
    m = importlib.import_module("zune-jpeg_amd")
    if not os.path.exists(m.lib_path()):
        import __graft_entry__ as g
        g.build()
    return m


def _desc(zj, cs=0, layout=0, w=256, h=128, hs=2, vs=2, ncomp=3):
    qt = np.ones((3, 64), np.int32)
    return zj.FrameDesc.make(w, h, hs, vs, ncomp, zj.ColorSpace(cs), [qt[0], qt[1], qt[2]], out_layout=layout)


def test_resized_out_len(zj):
    d = _desc(zj)
    assert zj.resized_out_len(d, 224, 224, zj.DTYPE_BF16) == 3 * 224 * 224 * 2
    assert zj.resized_out_len(d, 224, 100, zj.DTYPE_F32) == 3 * 224 * 100 * 4
    assert zj.resized_out_len(d, 7, 5, zj.DTYPE_U8) == 3 * 35
    assert zj.resized_out_len(_desc(zj, cs=1, hs=1, vs=1, ncomp=1), 10, 10, zj.DTYPE_F16) == 200
    assert zj.resized_out_len(_desc(zj, cs=2), 8192, 1, zj.DTYPE_F16) == 3 * 8192 * 2
    assert zj.resized_out_len(_desc(zj, cs=5), 224, 224, zj.DTYPE_BF16) == 0  # RGBA
    assert zj.resized_out_len(_desc(zj, cs=6), 224, 224, zj.DTYPE_BF16) == 0  # RGBX
    assert zj.resized_out_len(d, 8193, 224, zj.DTYPE_BF16) == 0
    assert zj.resized_out_len(d, 0, 224, zj.DTYPE_BF16) == 0
    assert zj.resized_out_len(d, 224, 224, 4) == 0


def test_resized_entry_points_reject_bad_arguments_without_a_gpu(zj):
    L = zj.lib()
    ERR_ARG = -1
    d = _desc(zj)
    buf = np.zeros(64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    ptrs = (C.c_void_p * 1)(p)
    wh = (C.c_uint * 2)(8, 8)
    sc = (C.c_float * 3)(1.0, 1.0, 1.0)
    win = (C.c_uint * 4)(0, 0, 8, 8)
    # no context
    assert L.zj_resize_device(None, 1, ptrs, wh, None, 3, 0, 4, 4, 2, 0, sc, sc, None, p, None) == ERR_ARG
    assert L.zj_decode_crops_resized_device(None, C.byref(d), 1, ptrs, ptrs, ptrs, win, 4, 4, 2, 0, sc, sc, None, p,
                                            None) == ERR_ARG
    assert L.zj_decoder_finish_pixels_resized_crop_device(None, None, 0, 0, 8, 8, 4, 4, 2, 0, sc, sc, 0, p, 1 << 20,
                                                          None) == ERR_ARG
    # a context handle that is never dereferenced: every argument check comes before the first use of the context... except
    # the null checks above.  With a real context missing (no GPU here), the decoder entry point fails on its own arguments
    dec = zj.Decoder()
    with pytest.raises(Exception):
        dec.finish_pixels_resized_crop_device(0, 0, 8, 8, 4, 4, zj.DTYPE_BF16, zj.TENSOR_NCHW, buf.ctypes.data, 1 << 20)
