"""GPU: antialiased resized crops (ZJ_RESIZE_BILINEAR_AA: zj_resize_filtered_device, zj_decode_crops_resized_filtered_device,
zj_decoder_finish_pixels_resized_crop_filtered_device, the antialias=True keywords of the Python layer) on an MI355X.
Every output must be, bit for bit, the numpy model of the definition (tests/resize_aa_model.py) applied to the u8 input --
for the crop entry points, to the crop zj_decode_crops_device itself writes for the same window; guard bytes stay 0xAA.
ZJ_RESIZE_BILINEAR through the filtered entry points is the existing entry points' bytes; the tensors are within 0.05 grey
levels (plus the dtype's rounding) of torch's own F.interpolate(antialias=True) on the GPU."""
import ctypes as C
import importlib
import os
import zlib

import numpy as np
import pytest

import resize_aa_model as am
import resize_model as rm
import test_gpu_resize as base

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD, ESZ = base.GUARD, base.ESZ
AA = 1


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


def _run_resize(zj, ctx, torch, ptrs, sizes, pitches, channels, chw, ow, oh, dtype, layout, scale, bias, flips, antialias):
    n = len(ptrs)
    per = channels * ow * oh * ESZ[dtype]
    buf = base.out_buffer(torch, n * per)
    ctx.resize_device(ptrs, sizes, channels, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, ow, oh, dtype,
                      zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW, buf.data_ptr() + GUARD, scale, bias, flips,
                      pitches, antialias=antialias)
    ctx.sync()
    out = base.read_out(buf, n * per)
    return [out[i * per:(i + 1) * per] for i in range(n)]


@pytest.mark.parametrize("channels,chw,dtype,layout", base.CASES)
def test_aa_resize_device_matches_the_model(zj, ctx, torch, channels, chw, dtype, layout):
    """images of their own sizes, pitches and offsets; sources wider than one LDS piece (682 RGB / 680 CHW / 2048 grey
    pixels per piece); bf16: above the 128 images of one launch"""
    rng = np.random.default_rng(zlib.crc32(f"aa{channels}{chw}{dtype}{layout}".encode()))
    n = 24 if dtype != rm.BF16 else 140
    sizes = [(int(rng.integers(1, 400)), int(rng.integers(1, 300))) for _ in range(n)]
    sizes[:5] = [(1, 1), (224, 224), (1000, 3), (2500, 41), (3, 700)]
    dev, ptrs, pitches, chws = base._device_images(torch, rng, sizes, channels, chw)
    flips = [bool(rng.integers(2)) for _ in range(n)]
    scale, bias = base.random_factors(rng, channels)
    for (ow, oh) in [(224, 224), (37, 5), (130, 3)]:
        outs = _run_resize(zj, ctx, torch, ptrs, sizes, pitches, channels, chw, ow, oh, dtype, layout, scale, bias, flips, True)
        for i in range(n):
            exp = am.resize(chws[i], ow, oh, dtype, scale, bias, flips[i], layout)
            base.check_image(outs[i], exp, dtype, f"image {i} {sizes[i]} -> {ow}x{oh}")


@pytest.mark.parametrize("size,out", [((65535, 1), (1, 1)), ((65535, 1), (8192, 1)), ((1, 65535), (1, 1)),
                                      ((1, 65535), (3, 8192)), ((5000, 2), (1, 1)), ((2, 2), (8192, 7))])
def test_aa_whole_axis_ranges(zj, ctx, torch, size, out):
    """a 65535-pixel source to one output (the tap count has no maximum) and to 8192, in both axes; grey and RGB"""
    rng = np.random.default_rng(size[0] + out[0])
    for channels in (1, 3):
        dev, ptrs, pitches, chws = base._device_images(torch, rng, [size], channels, False)
        outs = _run_resize(zj, ctx, torch, ptrs, [size], pitches, channels, False, out[0], out[1], rm.F32, "NCHW",
                           [1.0] * channels, [0.0] * channels, [True], True)
        exp = am.resize(chws[0], out[0], out[1], rm.F32, [1.0] * channels, [0.0] * channels, True)
        base.check_image(outs[0], exp, rm.F32, f"{channels} x {size} -> {out}")


def test_bilinear_filter_is_the_existing_entry_points(zj, ctx, torch, synth):
    """ZJ_RESIZE_BILINEAR through the three filtered entry points: the bytes of the entry points without a filter"""
    L = zj.lib()
    rng = np.random.default_rng(5)
    sizes = [(300, 200), (17, 401), (224, 224), (1, 1)]
    dev, ptrs, pitches, chws = base._device_images(torch, rng, sizes, 3, False)
    per = 3 * 96 * 80 * 2
    a, b = base.out_buffer(torch, 4 * per), base.out_buffer(torch, 4 * per)
    n = len(sizes)
    args = (ctx.handle, n, (C.c_void_p * n)(*ptrs), (C.c_uint * (2 * n))(*[v for s in sizes for v in s]),
            (C.c_uint * n)(*pitches), 3, 0, 96, 80, rm.BF16, 0, None, None, (C.c_uint8 * n)(0, 1, 0, 1))
    assert L.zj_resize_device(*args, C.c_void_p(a.data_ptr() + GUARD), None) == 0
    assert L.zj_resize_filtered_device(*args, zj.RESIZE_BILINEAR, C.c_void_p(b.data_ptr() + GUARD), None) == 0
    ctx.sync()
    assert np.array_equal(base.read_out(a, 4 * per), base.read_out(b, 4 * per))
    d, fr = base.frame_on_device(zj, torch, synth, 520, 203, 2, 2, "rgb", 0, seed=3)
    wins = base.windows_of(rng, 520, 203, 6)
    win = (C.c_uint * 24)(*[v for w in wins for v in w])
    ys, cbs, crs = [(C.c_void_p * 6)(*([f.data_ptr()] * 6)) for f in fr]
    per = 3 * 64 * 48 * 4
    a, b = base.out_buffer(torch, 6 * per), base.out_buffer(torch, 6 * per)
    cargs = (ctx.handle, C.byref(d), 6, ys, cbs, crs, win, 64, 48, rm.F32, 1, None, None, None)
    assert L.zj_decode_crops_resized_device(*cargs, C.c_void_p(a.data_ptr() + GUARD), None) == 0
    assert L.zj_decode_crops_resized_filtered_device(*cargs, zj.RESIZE_BILINEAR, C.c_void_p(b.data_ptr() + GUARD), None) == 0
    ctx.sync()
    assert np.array_equal(base.read_out(a, 6 * per), base.read_out(b, 6 * per))
    data = open(os.path.join(HERE, "golden", "test-baseline.jpg"), "rb").read()
    dec = zj.Decoder(zj.ZuneJpegOptions(), ctx)
    desc, _ = dec.prepare(data)
    per = zj.resized_out_len(desc, 31, 17, rm.F16)
    a, b = base.out_buffer(torch, per), base.out_buffer(torch, per)
    n_ = C.c_size_t(0)
    fargs = (dec._d, ctx.handle, 3, 5, min(desc.width - 3, 100), min(desc.height - 5, 77), 31, 17, rm.F16, 0, None, None, 1)
    assert L.zj_decoder_finish_pixels_resized_crop_device(*fargs, C.c_void_p(a.data_ptr() + GUARD), per, C.byref(n_)) == 0
    dec.prepare(data)
    assert L.zj_decoder_finish_pixels_resized_crop_filtered_device(*fargs, zj.RESIZE_BILINEAR, C.c_void_p(b.data_ptr() + GUARD),
                                                                   per, C.byref(n_)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(base.read_out(a, per), base.read_out(b, per))
    dec.close()


@pytest.mark.parametrize("mode", ["none", "hv"])
@pytest.mark.parametrize("kind", list(base.KINDS))
@pytest.mark.parametrize("flags", [0, 7])
def test_aa_crops_resized_equal_the_model_of_the_crop(zj, ctx, torch, synth, mode, kind, flags):
    hs, vs = base.MODES[mode]
    rng = np.random.default_rng(zlib.crc32(f"aa-{mode}-{kind}-{flags}".encode()))
    W, H = (1040, 136) if flags else (520, 203)
    d, dev = base.frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed=W + hs)
    c = base.channels_of(zj, d)
    wins = base.windows_of(rng, W, H, 10)
    flips = [bool(i % 3 == 1) for i in range(len(wins))]
    crops = [base.own_crop(zj, ctx, torch, d, dev, *w) for w in wins]
    dtype = int(rng.integers(4))
    layout = "NHWC" if rng.integers(2) else "NCHW"
    scale, bias = base.random_factors(rng, c)
    for (ow, oh) in [(64, 48), (7, 300)]:
        per = zj.resized_out_len(d, ow, oh, dtype)
        buf = base.out_buffer(torch, len(wins) * per)
        ctx.decode_crops_resized_device(d, [dev[0].data_ptr()] * len(wins), [dev[1].data_ptr()] * len(wins),
                                        [dev[2].data_ptr()] * len(wins), wins, ow, oh, dtype,
                                        zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW, buf.data_ptr() + GUARD, scale,
                                        bias, flips, antialias=True)
        ctx.sync()
        out = base.read_out(buf, len(wins) * per)
        for i, w in enumerate(wins):
            exp = am.resize(crops[i], ow, oh, dtype, scale, bias, flips[i], layout)
            base.check_image(out[i * per:(i + 1) * per], exp, dtype, f"{kind} {mode} flags {flags} window {w} -> {ow}x{oh}")


@pytest.mark.parametrize("entropy", ["cpu", "gpu"])
def test_aa_file_path_equals_the_model_of_the_crop(zj, torch, entropy):
    """zj_decoder_finish_pixels_resized_crop_filtered_device == the model applied to the file's own crop of the window"""
    rng = np.random.default_rng(zlib.crc32(("aa" + entropy).encode()))
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    paths = [os.path.join(HERE, "golden", "test-baseline.jpg"), os.path.join(HERE, "golden", "ref", "medium_no_samp_2500x1786.jpg")]
    checked = 0
    try:
        for path in paths:
            data = open(path, "rb").read()
            o = zj.ZuneJpegOptions()
            if entropy == "gpu":
                o.entropy = zj.ENTROPY_GPU_ALWAYS
            dec = zj.Decoder(o, ctx)
            desc, _ = dec.prepare(data)
            W, H = desc.width, desc.height
            for k, (x, y, w, h) in enumerate(base.windows_of(rng, W, H, 5)):
                ln = zj.crop_out_len(desc, w, h)
                cb = base.out_buffer(torch, ln)
                dec.prepare(data)
                assert dec.finish_pixels_crop_device(x, y, w, h, cb.data_ptr() + GUARD, ln) == ln
                crop = base.read_out(cb, ln)
                c = ln // (w * h)
                img = crop.reshape(h, w, c).transpose(2, 0, 1)
                dtype, layout = k % 4, ("NHWC" if k % 2 else "NCHW")
                ow, oh = (224, 224) if k % 2 else (97, 61)
                scale, bias = base.random_factors(rng, c)
                per = zj.resized_out_len(desc, ow, oh, dtype)
                buf = base.out_buffer(torch, per)
                dec.prepare(data)
                assert dec.finish_pixels_resized_crop_device(x, y, w, h, ow, oh, dtype,
                                                             zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW,
                                                             buf.data_ptr() + GUARD, per, scale, bias, flip=bool(k % 3),
                                                             antialias=True) == per
                exp = am.resize(img, ow, oh, dtype, scale, bias, bool(k % 3), layout)
                base.check_image(base.read_out(buf, per), exp, dtype, f"{os.path.basename(path)} {entropy} {(x, y, w, h)}")
                checked += 1
            dec.close()
    finally:
        ctx.close()
    assert checked >= 8


def test_aa_tensors_are_torch_antialias_on_the_gpu(zj, ctx, torch, synth):
    """decode_resized_crops_to_tensor / resize_to_tensor (antialias=True) against F.interpolate(antialias=True) run by torch
    on the GPU over the same u8 crops: within 0.05 / 255 plus the dtype's rounding (the [0, 1] image: no mean / std)"""
    import torch.nn.functional as F
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    d, dev = base.frame_on_device(zj, torch, synth, 2048, 1536, 2, 2, "rgb", 0, seed=21)
    wins = [(0, 0, 2048, 1536), (100, 37, 1800, 1200), (5, 9, 224, 224), (1000, 700, 150, 90), (3, 3, 2000, 300)]
    crops = [torch.from_numpy(base.own_crop(zj, ctx, torch, d, dev, *w)).cuda() for w in wins]
    torch.cuda.synchronize()
    for dtype, ulp in ((torch.float32, 1e-6), (torch.bfloat16, 2.0 ** -8)):
        out = tensors.decode_resized_crops_to_tensor(ctx, d, [dev] * len(wins), wins, (224, 224), dtype=dtype, antialias=True)
        hwc = [c.permute(1, 2, 0).contiguous() for c in crops]
        out2 = tensors.resize_to_tensor(ctx, hwc, (224, 224), dtype=dtype, antialias=True)
        torch.cuda.synchronize()
        assert torch.equal(out, out2)
        for i, c in enumerate(crops):
            ref = F.interpolate(c[None].float(), size=(224, 224), mode="bilinear", align_corners=False, antialias=True)[0] / 255
            err = (out[i].float() - ref).abs().max().item()
            assert err <= 0.05 / 255 + ulp, (wins[i], dtype, err)
        plain = tensors.decode_resized_crops_to_tensor(ctx, d, [dev] * len(wins), wins, (224, 224), dtype=dtype)
        torch.cuda.synchronize()
        assert not torch.equal(plain, out)  # (the default stays the bilinear filter)


def test_aa_unknown_filters_launch_nothing(zj, ctx, torch, synth):
    L = zj.lib()
    buf = base.out_buffer(torch, 4096)
    p = C.c_void_p(buf.data_ptr() + GUARD)
    src = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * 1)(C.c_void_p(src.data_ptr()))
    wh = (C.c_uint * 2)(8, 8)
    h = ctx.handle
    for f in (2, -1, 1 << 20):
        assert L.zj_resize_filtered_device(h, 1, ptrs, wh, None, 1, 0, 4, 4, 3, 0, None, None, None, f, p, None) == -1
    assert L.zj_resize_filtered_device(h, 1, ptrs, wh, None, 1, 0, 8193, 4, 3, 0, None, None, None, AA, p, None) == -1
    assert L.zj_resize_filtered_device(h, 1, ptrs, (C.c_uint * 2)(0, 8), None, 1, 0, 4, 4, 3, 0, None, None, None, AA, p,
                                       None) == -1
    d, dev = base.frame_on_device(zj, torch, synth, 256, 128, 2, 2, "rgb", 0, seed=1)
    win = (C.c_uint * 4)(0, 0, 64, 64)
    planes = [(C.c_void_p * 1)(C.c_void_p(t.data_ptr())) for t in dev]
    assert L.zj_decode_crops_resized_filtered_device(h, C.byref(d), 1, *planes, win, 4, 4, 3, 0, None, None, None, 2, p,
                                                     None) == -1
    data = open(os.path.join(HERE, "golden", "test-baseline.jpg"), "rb").read()
    dec = zj.Decoder(zj.ZuneJpegOptions(), ctx)
    dec.prepare(data)
    n = C.c_size_t(0)
    assert L.zj_decoder_finish_pixels_resized_crop_filtered_device(dec._d, h, 0, 0, 8, 8, 4, 4, 3, 0, None, None, 0, 3, p, 4096,
                                                                   C.byref(n)) == -1
    dec.close()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xAA).all()
    # ... and the same calls with the antialiased filter do write
    assert L.zj_resize_filtered_device(h, 1, ptrs, wh, None, 1, 0, 4, 4, 3, 0, None, None, None, AA, p, None) == 0
    ctx.sync()
    assert (base.read_out(buf, 16) == 7).all()
