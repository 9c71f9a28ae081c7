"""GPU: bicubic antialiased resized crops (ZJ_RESIZE_BICUBIC_AA = 4 through the *_filtered_device, *_prescaled_device and
*_oriented_device entry points, the file path, and interpolation="bicubic" of the Python layer) on an MI355X.  Every output
must be, bit for bit, the numpy model of the definition (tests/resize_bicubic_model.py) applied to the u8
input -- for the crop entry points, to the crop that the library's own crop, reduced-size or oriented path writes for the
same window; guard bytes stay 0xAA."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import orient_model as om
import resize_bicubic_model as bm
import resize_model as rm
import scaled_model as sm
import test_gpu_resize as base

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD, ESZ = base.GUARD, base.ESZ
BICUBIC = 4


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)
    yield c
    c.close()


SIZES = [(1, 1), (65, 3), (683, 9), (2049, 2), (300, 200)]
OUTS = [(64, 48), (7, 5)]
_MIXED = {}


def mixed_images(torch, channels, chw):
    """the five images on the device and the model's v of each for both output sizes: made once per input layout, shared
    (read-only) by the dtype and tensor-layout cases"""
    key = (channels, chw)
    if key not in _MIXED:
        rng = np.random.default_rng(40 + channels + chw)
        dev, ptrs, pitches, chws = base._device_images(torch, rng, SIZES, channels, chw)
        vs = {}
        for out in OUTS:
            for i, img in enumerate(chws):
                vs[out, i] = bm.values(img, out[0], out[1])
                vs[out, i].setflags(write=False)
        _MIXED[key] = (dev, ptrs, pitches, chws, vs)
    return _MIXED[key]


def from_v(v, dtype, scale, bias, flip, layout):
    """the model's output conversion (resize_bicubic_model.resize) of a v computed before"""
    v = v[:, :, ::-1] if flip else v
    if dtype == rm.U8:
        out = ((v + 32768) >> 16).astype(np.uint8)
    else:
        s, b = rm.factors(v.shape[0], scale, bias)
        y = ((v.astype(np.float32) * s[:, None, None]).astype(np.float32) + b[:, None, None]).astype(np.float32)
        if dtype == rm.F32:
            out = y
        elif dtype == rm.F16:
            with np.errstate(over="ignore"):
                out = y.astype(np.float16).view(np.uint16)
        else:
            out = rm.bf16_bits(y)
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if layout == "NHWC" else np.ascontiguousarray(out)


@pytest.mark.parametrize("channels,chw,dtype,layout", base.CASES)
def test_bicubic_resize_filtered_device_matches_the_model(zj, ctx, torch, channels, chw, dtype, layout):
    """one launch of five images of their own sizes, pitches and offsets (several pieces of columns: 683 RGB, 2049 grey),
    through the C ABI with filter 4"""
    L = zj.lib()
    dev, ptrs, pitches, chws, vs = mixed_images(torch, channels, chw)
    n = len(SIZES)
    flips = [False, True, True, False, True]
    scale, bias = np.array([0.0039, 0.011, 0.027][:channels], np.float32), np.array([-0.5, 1.25, -2.75][:channels], np.float32)
    sc, bi = (C.c_float * 3)(*scale), (C.c_float * 3)(*bias)
    for (ow, oh) in OUTS:
        per = channels * ow * oh * ESZ[dtype]
        buf = base.out_buffer(torch, n * per)
        rc = L.zj_resize_filtered_device(ctx.handle, n, (C.c_void_p * n)(*ptrs), (C.c_uint * (2 * n))(*[v for s in SIZES for v in s]),
                                         (C.c_uint * n)(*pitches), channels, 1 if chw else 0, ow, oh, dtype,
                                         1 if layout == "NHWC" else 0, sc, bi, (C.c_uint8 * n)(*flips), BICUBIC,
                                         C.c_void_p(buf.data_ptr() + GUARD), None)
        assert rc == 0, rc
        ctx.sync()
        out = base.read_out(buf, n * per)  # (checks the guard bytes)
        for i in range(n):
            exp = from_v(vs[(ow, oh), i], dtype, scale, bias, flips[i], layout)
            base.check_image(out[i * per:(i + 1) * per], exp, dtype, f"image {i} {SIZES[i]} -> {ow}x{oh}")


FRAMES = [(256, 128, 2, 2), (96, 80, 1, 1)]


def windows(W, H):
    """windows of their own sizes; the first is at least twice 24 x 20 in both axes (a 1/2 prescale where one is allowed)"""
    return [(W - 50, H - 41, 50, 41), (3, 5, 31, 17), (0, 0, W, H), (W - 1, H - 1, 1, 1), (7, 2, 24, 20)]


def run_crops(zj, ctx, torch, d, dev, wins, size, dtype, entry, flips=None, k=0, oris=None):
    """one of the three crop entry points through the C ABI with filter 4"""
    L = zj.lib()
    n = len(wins)
    per = zj.resized_out_len(d, size[0], size[1], dtype)
    buf = base.out_buffer(torch, n * per)
    planes = [(C.c_void_p * n)(*([t.data_ptr()] * n)) for t in dev]
    win = (C.c_uint * (4 * n))(*[v for w in wins for v in w])
    fl = (C.c_uint8 * n)(*flips) if flips else None
    args = (ctx.handle, C.byref(d), n, *planes, win, size[0], size[1], dtype, 0, None, None, fl, BICUBIC)
    out = C.c_void_p(buf.data_ptr() + GUARD)
    if entry == "filtered":
        rc = L.zj_decode_crops_resized_filtered_device(*args, out, None)
    elif entry == "prescaled":
        rc = L.zj_decode_crops_resized_prescaled_device(*args, k, out, None)
    else:
        rc = L.zj_decode_crops_resized_oriented_device(*args, k, (C.c_uint8 * n)(*oris), out, None)
    assert rc == 0, (entry, rc)
    ctx.sync()
    a = base.read_out(buf, n * per)
    return [a[i * per:(i + 1) * per] for i in range(n)]


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H,hs,vs", FRAMES)
def test_bicubic_crop_entry_points_equal_the_model_of_the_crop(zj, ctx, torch, synth, W, H, hs, vs, gray):
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
    d = zj.FrameDesc.make(W, H, hs, vs, 3, zj.ColorSpace.GRAYSCALE if gray else zj.ColorSpace.RGB, qts)
    dev = [torch.from_numpy(np.ascontiguousarray(p, np.int16)).cuda() for p in planes]
    torch.cuda.synchronize()
    ch = 1 if gray else 3
    size = (24, 20)
    wins = windows(W, H)
    flips = [False, True, False, False, True]

    def crop(win, scale=1):
        """the library's own crop (or reduced-size decode) of a stored window, [C, h, w]"""
        x, y, w, h = win
        n = zj.crop_out_len(d, w, h) if scale == 1 else zj.scaled_crop_out_len(d, scale, w, h)
        buf = torch.empty((n,), dtype=torch.uint8, device="cuda")
        p = [t.data_ptr() for t in dev]
        if scale == 1:
            ctx.decode_crops_device(d, [p[0]], [p[1]], [p[2]], [(x, y)], w, h, [buf.data_ptr()])
        else:
            ctx.decode_crops_scaled_device(d, [p[0]], [p[1]], [p[2]], scale, [buf.data_ptr()], [win])
        ctx.sync()
        return buf.cpu().numpy().reshape(h, w, ch)

    # 1. filtered: the model of the crop
    for dtype in (rm.U8, rm.BF16):
        outs = run_crops(zj, ctx, torch, d, dev, wins, size, dtype, "filtered", flips)
        for i, win in enumerate(wins):
            exp = bm.resize(crop(win).transpose(2, 0, 1), size[0], size[1], dtype, None, None, flips[i])
            base.check_image(outs[i], exp, dtype, f"filtered {win}")
    # 2. prescaled (up to 1/2): the model of the reduced crop where the rule picks 1/2, the filtered bytes elsewhere
    outs = run_crops(zj, ctx, torch, d, dev, wins, size, rm.F32, "prescaled", flips, k=1)
    plain = run_crops(zj, ctx, torch, d, dev, wins, size, rm.F32, "filtered", flips)
    picked = [sm.prescale_log2(w, h, size[0], size[1], 1) for (_, _, w, h) in wins]
    assert 1 in picked and 0 in picked
    for i, win in enumerate(wins):
        if picked[i] == 0:
            assert np.array_equal(outs[i], plain[i]), win
            continue
        red = crop(sm.reduced_window(*win, 1, W, H), scale=2)
        exp = bm.resize(red.transpose(2, 0, 1), size[0], size[1], rm.F32, None, None, flips[i])
        base.check_image(outs[i], exp, rm.F32, f"prescaled {win}")
    # 3. oriented: windows in DISPLAYED pixels, the crop turned before the resize
    for o in (1, 3, 6):
        dw, dh = om.oriented_size(o, W, H)
        dwins = windows(dw, dh)
        outs = run_crops(zj, ctx, torch, d, dev, dwins, size, rm.U8, "oriented", None, k=0, oris=[o] * len(dwins))
        for i, win in enumerate(dwins):
            img = om.orient(crop(om.stored_window(o, W, H, win)), o)
            exp = bm.resize(np.ascontiguousarray(img.transpose(2, 0, 1)), size[0], size[1], rm.U8)
            base.check_image(outs[i], exp, rm.U8, f"orientation {o} {win}")


def test_bicubic_file_path_equals_the_model_of_the_crop(zj, ctx, torch):
    """zj_decoder_finish_pixels_resized_crop_filtered_device with filter 4 == the model on the file's own crop"""
    L = zj.lib()
    data = open(os.path.join(HERE, "golden", "test-baseline.jpg"), "rb").read()
    dec = zj.Decoder(zj.ZuneJpegOptions(), ctx)
    desc, _ = dec.prepare(data)
    x, y, w, h = 3, 5, min(desc.width - 3, 300), min(desc.height - 5, 177)
    assert w > 97 or h > 61
    ln = zj.crop_out_len(desc, w, h)
    cb = base.out_buffer(torch, ln)
    assert dec.finish_pixels_crop_device(x, y, w, h, cb.data_ptr() + GUARD, ln) == ln
    img = base.read_out(cb, ln).reshape(h, w, ln // (w * h)).transpose(2, 0, 1)
    ow, oh, dtype = 97, 61, rm.F16
    per = zj.resized_out_len(desc, ow, oh, dtype)
    buf = base.out_buffer(torch, per)
    n_ = C.c_size_t(0)
    dec.prepare(data)
    assert L.zj_decoder_finish_pixels_resized_crop_filtered_device(dec._d, ctx.handle, x, y, w, h, ow, oh, dtype, 1, None, None,
                                                                   1, BICUBIC, C.c_void_p(buf.data_ptr() + GUARD), per,
                                                                   C.byref(n_)) == 0
    torch.cuda.synchronize()
    assert n_.value == per
    exp = bm.resize(np.ascontiguousarray(img), ow, oh, dtype, None, None, True, "NHWC")
    base.check_image(base.read_out(buf, per), exp, dtype, "test-baseline.jpg")
    dec.close()


def test_bicubic_python_layer_and_identity(zj, ctx, torch, synth):
    """interpolation="bicubic" of decode_resized_crops_to_tensor is the C ABI's bytes, differs from the triangle filter on a
    window that is not flat, and leaves the defaults alone; a window of the output's size gives the crop"""
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    d, dev = base.frame_on_device(zj, torch, synth, 256, 128, 2, 2, "rgb", 0, seed=5)
    wins = [(0, 0, 256, 128), (11, 7, 150, 90), (100, 60, 64, 48)]
    out = tensors.decode_resized_crops_to_tensor(ctx, d, [dev] * 3, wins, (64, 48), dtype=torch.uint8, antialias=True,
                                                 interpolation="bicubic")
    tri = tensors.decode_resized_crops_to_tensor(ctx, d, [dev] * 3, wins, (64, 48), dtype=torch.uint8, antialias=True)
    tri2 = tensors.decode_resized_crops_to_tensor(ctx, d, [dev] * 3, wins, (64, 48), dtype=torch.uint8, antialias=True,
                                                  interpolation="bilinear")
    plain = tensors.decode_resized_crops_to_tensor(ctx, d, [dev] * 3, wins, (64, 48), dtype=torch.uint8)
    torch.cuda.synchronize()
    abi = run_crops(zj, ctx, torch, d, dev, wins, (64, 48), rm.U8, "filtered")
    for i in range(3):
        assert np.array_equal(out[i].cpu().numpy().reshape(-1), abi[i])
    assert not torch.equal(out[1], tri[1]) and torch.equal(tri, tri2)
    ref = base.run_resized(zj, ctx, torch, d, [dev] * 3, wins, 64, 48, rm.U8, "NCHW", None, None, None)
    assert np.array_equal(plain.cpu().numpy().reshape(3, -1), np.stack(ref))  # (the default: the bilinear entry point)
    crop = base.own_crop(zj, ctx, torch, d, dev, *wins[2])
    assert np.array_equal(out[2].cpu().numpy(), crop)  # (64 x 48 -> 64 x 48)
    hwc = [torch.from_numpy(np.ascontiguousarray(crop.transpose(1, 2, 0))).cuda()]
    same = tensors.resize_to_tensor(ctx, hwc, (64, 48), dtype=torch.uint8, antialias=True, interpolation="bicubic")
    torch.cuda.synchronize()
    assert np.array_equal(same[0].cpu().numpy(), crop)
