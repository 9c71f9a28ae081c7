"""GPU: u8 images in HBM into a normalised tensor, not resized (zj_to_tensor_device, tensors.to_normalized_tensor), and the
crop-tensor file calls of the files that pass through it -- gray shown as RGB, CMYK / YCCK, other samplings and stored RGB,
turned files -- on an MI355X.  The stage must be, byte for byte, zj_resize_device at the images' own size
(1 -> 3: after zj_gray_to_rgb_device); the file calls must be, byte for byte, the resized-crop file calls at out == window,
bilinear, which already decode all these files.  Every output lies between guard bytes that must stay untouched."""
import ctypes as C
import importlib
import os
import sys
import zlib

import numpy as np
import pytest

import orient_model as om
import resize_model as rm
import sampling_cases as sc
from test_gpu_cmyk import four_file
from test_gpu_crop_tensor import ESZ, GUARD, body, convert, factors, guarded, layout_code
from test_gpu_sampling import odd_file

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
CHANNELS = [(1, 1), (1, 3), (3, 3)]
COMBOS = [(dt, lay) for dt in (rm.F32, rm.F16, rm.BF16, rm.U8) for lay in ("NCHW", "NHWC")]
ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def tz():
    return importlib.import_module("zune-jpeg_amd.tensors")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def je():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import jpeg_enc
    return jpeg_enc


# ---- 1. the stage ---------------------------------------------------------------------------------------------------------
def images_on_device(torch, rng, n, w, h, cin, pads, mis):
    """n images side by side in one device buffer, image i at a dword boundary + mis[i], its rows w * cin + pads[i] apart,
    random bytes between them: (the buffer, device pointers, pitches, the images [n, h, w, cin] on the host)"""
    offs, pitches, at = [], [], 0
    for i in range(n):
        at = (at + 3) // 4 * 4 + mis[i % len(mis)]
        pitch = w * cin + pads[i % len(pads)]
        offs.append(at); pitches.append(pitch)
        at += pitch * (h - 1) + w * cin
    host = rng.integers(0, 256, at + 16, dtype=np.uint8)
    imgs = np.stack([np.lib.stride_tricks.as_strided(host[o:], (h, w, cin), (p, cin, 1)) for o, p in zip(offs, pitches)])
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    return dev, [dev.data_ptr() + o for o in offs], pitches, imgs


def run_stage(zj, ctx, torch, ptrs, w, h, pitches, cin, cout, dtype, layout, scale, bias, flips):
    per = cout * w * h * ESZ[dtype]
    buf = guarded(torch, len(ptrs) * per)
    ctx.to_tensor_device(ptrs, w, h, cin, cout, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, scale, bias, flips, pitches)
    ctx.sync()
    return body(torch, buf, len(ptrs) * per)


def run_identity_resize(zj, ctx, torch, ptrs, w, h, pitches, cin, cout, dtype, layout, scale, bias, flips):
    """zj_resize_device at out == in; 1 -> 3: zj_gray_to_rgb_device into tight images first"""
    n = len(ptrs)
    keep = None
    if cin != cout:
        keep = torch.empty(n * 3 * w * h, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        outs = [keep.data_ptr() + i * 3 * w * h for i in range(n)]
        ctx.gray_to_rgb_device(ptrs, [(w, h)] * n, zj.LAYOUT_HWC, outs, pitches)
        ptrs, pitches = outs, None
    per = cout * w * h * ESZ[dtype]
    buf = guarded(torch, n * per)
    ctx.resize_device(ptrs, [(w, h)] * n, cout, zj.LAYOUT_HWC, w, h, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, scale, bias,
                      flips, pitches)
    ctx.sync()
    return body(torch, buf, n * per)


def model(imgs, cout, dtype, layout, scale, bias, flips):
    x = imgs if imgs.shape[3] == cout else np.repeat(imgs, cout, axis=3)
    return convert(x, dtype, layout, scale, bias, flips)


@pytest.mark.parametrize("chans", CHANNELS, ids=["1to1", "1to3", "3to3"])
def test_stage_equals_the_identity_size_resize(zj, ctx, torch, chans):
    cin, cout = chans
    rng = np.random.default_rng(zlib.crc32(f"stage-{cin}-{cout}".encode()))
    for (w, h) in [(1, 1), (7, 3), (33, 17), (257, 5), (513, 9)]:
        for i, (dtype, layout) in enumerate(COMBOS):
            pads, mis, flips = [[0, 1, 13], [13, 0, 0], [0, 0, 0]][i % 3], [(i + k) % 4 for k in range(3)], [bool((i >> k) & 1) for k in range(3)]
            dev, ptrs, pitches, imgs = images_on_device(torch, rng, 3, w, h, cin, pads, mis)
            scale, bias = factors(rng, cout)
            args = (zj, ctx, torch, ptrs, w, h, pitches, cin, cout, dtype, layout, scale, bias, flips)
            got, ref = run_stage(*args), run_identity_resize(*args)
            what = f"{w}x{h} {cin}->{cout} dtype {dtype} {layout} pads {pads} misalign {mis} flips {flips}"
            assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} bytes differ from the identity-size resize"
            assert np.array_equal(got.cpu().numpy(), model(imgs, cout, dtype, layout, scale, bias, flips)), what


@pytest.mark.parametrize("chans", CHANNELS, ids=["1to1", "1to3", "3to3"])
def test_129_images_take_two_launches(zj, ctx, torch, chans):
    cin, cout = chans
    rng = np.random.default_rng(129 + cout)
    flips = [bool(rng.integers(2)) for _ in range(129)]
    for (dtype, layout) in [(rm.BF16, "NCHW"), (rm.F32, "NHWC")]:
        dev, ptrs, pitches, imgs = images_on_device(torch, rng, 129, 16, 8, cin, [0, 1, 13], [0, 1, 2, 3])
        scale, bias = factors(rng, cout)
        args = (zj, ctx, torch, ptrs, 16, 8, pitches, cin, cout, dtype, layout, scale, bias, flips)
        assert torch.equal(run_stage(*args), run_identity_resize(*args)), (chans, dtype, layout)


@pytest.mark.parametrize("chans", [(1, 3), (3, 3)], ids=["1to3", "3to3"])
def test_an_image_wider_than_the_resize_takes(zj, ctx, torch, chans):
    """8200 x 2 is past zj_resize_device's 8192: against the numpy conversion only"""
    cin, cout = chans
    rng = np.random.default_rng(8200)
    dev, ptrs, pitches, imgs = images_on_device(torch, rng, 2, 8200, 2, cin, [1, 0], [3, 1])
    for (dtype, layout) in [(rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NCHW")]:
        scale, bias = factors(rng, cout)
        got = run_stage(zj, ctx, torch, ptrs, 8200, 2, pitches, cin, cout, dtype, layout, scale, bias, [True, False])
        assert np.array_equal(got.cpu().numpy(), model(imgs, cout, dtype, layout, scale, bias, [True, False])), (chans, dtype, layout)
    with pytest.raises(zj.ZjError):
        ctx.resize_device(ptrs, [(8200, 2)] * 2, cin, zj.LAYOUT_HWC, 8200, 2, rm.U8, 0, dev.data_ptr(), None, None, None, pitches)


def test_stage_rejects_bad_arguments(zj, ctx, torch):
    L = zj.lib()
    rng = np.random.default_rng(5)
    dev, ptrs, pitches, imgs = images_on_device(torch, rng, 1, 8, 8, 3, [0], [0])
    buf = guarded(torch, 3 * 8 * 8 * 4)
    out = C.c_void_p(buf.data_ptr() + GUARD)
    ins = (C.c_void_p * 1)(ptrs[0])
    ok = (C.c_float * 3)(1.0, 1.0, 1.0)
    inf = (C.c_float * 3)(1.0, float("inf"), 1.0)
    nan = (C.c_float * 3)(float("nan"), 0.0, 0.0)
    h = ctx.handle
    call = lambda n, i, w, hh, pit, cin, cout, dt, lay, sc, bi, dst: L.zj_to_tensor_device(h, n, i, w, hh, pit, cin, cout, dt, lay, sc,
                                                                                          bi, None, dst, None)
    assert call(1, ins, 8, 8, None, 3, 3, 4, 0, ok, ok, out) == ARG          # no such dtype
    assert call(1, ins, 8, 8, None, 3, 3, 0, 2, ok, ok, out) == ARG          # no such layout
    assert call(1, ins, 8, 8, None, 3, 3, 0, 0, inf, ok, out) == ARG and call(1, ins, 8, 8, None, 3, 3, 0, 0, ok, nan, out) == ARG
    assert call(1, ins, 8, 8, (C.c_uint * 1)(23), 3, 3, 0, 0, ok, ok, out) == ARG  # a pitch below w * in_channels
    assert call(0, ins, 8, 8, None, 3, 3, 0, 0, ok, ok, out) == ARG
    assert call(1, None, 8, 8, None, 3, 3, 0, 0, ok, ok, out) == ARG and call(1, ins, 8, 8, None, 3, 3, 0, 0, ok, ok, None) == ARG
    assert call(1, (C.c_void_p * 1)(None), 8, 8, None, 3, 3, 0, 0, ok, ok, out) == ARG
    assert call(1, ins, 8, 8, None, 3, 1, 0, 0, ok, ok, out) == ARG and call(1, ins, 8, 8, None, 2, 2, 0, 0, ok, ok, out) == ARG
    assert call(1, ins, 0, 8, None, 3, 3, 0, 0, ok, ok, out) == ARG and call(1, ins, 8, 65536, None, 3, 3, 0, 0, ok, ok, out) == ARG
    assert call(1, ins, 8, 8, None, 3, 3, 0, 0, ok, ok, C.c_void_p(buf.data_ptr() + GUARD + 2)) == ARG  # not aligned to a float
    ctx.sync()
    assert bool((buf == 0xAA).all()), "a refused call wrote"
    assert call(1, ins, 8, 8, None, 3, 3, 0, 0, ok, ok, out) == 0
    ctx.sync()
    assert np.array_equal(body(torch, buf, 3 * 8 * 8 * 4).cpu().numpy(), model(imgs, 3, rm.F32, "NCHW", np.ones(3, np.float32), np.ones(3, np.float32), None))  # (scale and bias 1)


def test_tensors_wrapper(zj, tz, ctx, torch):
    """tensors.to_normalized_tensor against torch's own (x / 255 - mean) / std, within the 0.0156 of bf16
    (test_gpu_crop_tensor.py); row-strided inputs, [h, w] inputs shown in three channels, flips"""
    g = torch.Generator(device="cpu").manual_seed(3)
    h, w, n = 37, 53, 5
    big = torch.randint(0, 256, (n, h, w + 9, 3), dtype=torch.uint8, generator=g).cuda()
    imgs = [big[i, :, 4:4 + w] for i in range(n)]  # (row-strided views)
    flips = [bool(i & 1) for i in range(n)]
    x = torch.stack([im.flip(1) if f else im for im, f in zip(imgs, flips)]).float() / 255
    ref = (x - torch.tensor(MEAN, device="cuda")) / torch.tensor(STD, device="cuda")
    for dtype in (torch.bfloat16, torch.float32, torch.float16):
        for layout in ("NCHW", "NHWC"):
            out = tz.to_normalized_tensor(ctx, imgs, dtype=dtype, layout=layout, mean=MEAN, std=STD, flips=flips)
            torch.cuda.synchronize()
            assert out.dtype == dtype and out.is_contiguous()
            assert tuple(out.shape) == ((n, 3, h, w) if layout == "NCHW" else (n, h, w, 3))
            nhwc = out.permute(0, 2, 3, 1) if layout == "NCHW" else out
            assert float((nhwc.float() - ref).abs().max()) <= 0.0156
    u8 = tz.to_normalized_tensor(ctx, imgs, dtype=torch.uint8, layout="NHWC")
    torch.cuda.synchronize()
    assert torch.equal(u8, torch.stack(imgs))
    gray = [im[..., 1].contiguous() for im in imgs]  # [h, w]
    out = tz.to_normalized_tensor(ctx, gray, dtype=torch.float32, layout="NHWC", mean=MEAN, std=STD, channels=3)
    torch.cuda.synchronize()
    g3 = torch.stack(gray).unsqueeze(-1).expand(-1, -1, -1, 3).float() / 255
    assert float((out - (g3 - torch.tensor(MEAN, device="cuda")) / torch.tensor(STD, device="cuda")).abs().max()) <= 0.0156
    one = tz.to_normalized_tensor(ctx, gray, dtype=torch.uint8)
    torch.cuda.synchronize()
    assert tuple(one.shape) == (n, 1, h, w) and torch.equal(one[:, 0], torch.stack(gray))
    with pytest.raises(ValueError):
        tz.to_normalized_tensor(ctx, imgs, channels=1)
    with pytest.raises(ValueError):
        tz.to_normalized_tensor(ctx, [imgs[0], imgs[1][:-1]])


# ---- 2. the file calls ------------------------------------------------------------------------------------------------------
def options(zj, entropy="ENTROPY_CPU", flags=None):
    o = zj.ZuneJpegOptions()
    o.flags = (zj.FLAG_GRAY_TO_RGB | zj.FLAG_CMYK_TO_RGB | zj.FLAG_ANY_SAMPLING) if flags is None else flags
    o.entropy = getattr(zj, entropy)
    return o


def gray_file(je, synth, w=120, h=50, seed=3, orientation=None):
    data = je.encode_baseline(je.small_planes(w, h, 1, 1, 1, seed=seed), synth.quant_tables(85), w, h, 1, 1, 1)
    return om.splice(data, om.exif_segment(orientation)) if orientation else data


def colour_file(je, synth, w, h, hs, vs, seed, orientation=None):
    data = je.encode_baseline(je.small_planes(w, h, hs, vs, 3, seed=seed), synth.quant_tables(70 + seed % 20), w, h, hs, vs, 3)
    return om.splice(data, om.exif_segment(orientation)) if orientation else data


def tensor_call(zj, ctx, torch, blob, opt, win, dtype, layout, scale, bias, flip, oriented=False):
    """the crop-tensor file call: (status, the image's bytes on the device -- the poison if refused -- , the error text)"""
    x, y, w, h = win
    per = 3 * w * h * ESZ.get(dtype, 4)  # (no such dtype: a buffer all the same)
    buf = guarded(torch, per)
    dec = zj.Decoder(opt, ctx)
    try:
        dec.prepare(blob)
        try:
            n = dec.finish_pixels_crop_tensor_device(x, y, w, h, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, per, scale, bias,
                                                     flip, apply_orientation=oriented)
            assert n == per, "*out_len is not the image's size"
            rc, text = 0, ""
        except zj.ZjError as e:
            rc, text = e.status, str(e)
    finally:
        dec.close()
    return rc, body(torch, buf, per), text


def resized_call(zj, ctx, torch, blob, opt, win, dtype, layout, scale, bias, flip, oriented=False):
    """the reference: the resized-crop file call at out == window, bilinear, no prescale"""
    x, y, w, h = win
    per = 3 * w * h * ESZ[dtype]
    buf = guarded(torch, per)
    dec = zj.Decoder(opt, ctx)
    try:
        dec.prepare(blob)
        assert dec.finish_pixels_resized_crop_device(x, y, w, h, w, h, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, per, scale,
                                                     bias, flip, False, 1, oriented) == per
    finally:
        dec.close()
    return body(torch, buf, per)


def windows(W, H):
    """odd and even origins, one touching the right and bottom edges, one of width 1"""
    return [(1, 3, min(W - 1, 33), min(H - 3, 17)), (2, 2, W - 5, H - 4), (W - 21, H - 9, 21, 9), (5, 4, 1, 7), (0, 0, W, H)]


def check_file(zj, ctx, torch, blob, W, H, what, entropy="ENTROPY_CPU"):
    rng = np.random.default_rng(zlib.crc32(what.encode()))
    opt = options(zj, entropy)
    for i, win in enumerate(windows(W, H)):
        for (dtype, layout) in ((rm.F32, "NHWC"), (rm.BF16, "NCHW")):
            scale, bias = factors(rng, 3)
            flip = bool((i + dtype) & 1)
            rc, got, text = tensor_call(zj, ctx, torch, blob, opt, win, dtype, layout, scale, bias, flip)
            assert rc == 0, (what, win, rc, text)
            ref = resized_call(zj, ctx, torch, blob, opt, win, dtype, layout, scale, bias, flip)
            assert torch.equal(got, ref), f"{what} window {win} dtype {dtype} {layout} flip {flip}: {int((got != ref).sum())} bytes differ"


@pytest.mark.parametrize("entropy", ["ENTROPY_CPU", "ENTROPY_GPU_ALWAYS"])
def test_gray_file_shown_as_rgb(zj, ctx, torch, synth, je, entropy):
    check_file(zj, ctx, torch, gray_file(je, synth), 120, 50, f"gray {entropy}", entropy)


@pytest.mark.parametrize("case", [("hv", False, 0), ("h", True, 0), ("hv", True, 2), ("none", False, 2), ("v", False, None)],
                         ids=lambda c: f"{c[0]}-{'p' if c[1] else 'b'}-t{c[2]}")
def test_cmyk_and_ycck_files(zj, ctx, torch, synth, case):
    mode, prog, adobe = case
    W, H = (100, 75) if mode == "hv" else (48, 40)
    check_file(zj, ctx, torch, four_file(synth, W, H, mode, seed=7 + len(mode), progressive=prog, adobe=adobe, restart=0 if prog else 3),
               W, H, f"four {case}")


@pytest.mark.parametrize("case", [(sc.SAMPLINGS[0], False, None), (sc.SAMPLINGS[1], True, None), (sc.SAMPLINGS[3], False, None),
                                  (sc.SAMPLINGS[4], False, None), (sc.STANDARD[3], False, 0), (sc.STANDARD[0], True, 0)],
                         ids=lambda c: f"{sc.name(c[0])}-{'p' if c[1] else 'b'}-a{c[2]}")
def test_odd_sampled_and_stored_rgb_files(zj, ctx, torch, synth, case):
    samp, prog, adobe = case
    kw = {} if adobe is None else {"adobe": adobe}
    check_file(zj, ctx, torch, odd_file(synth, 100, 75, samp, seed=11, progressive=prog, **kw), 100, 75, f"odd {case}")


def test_what_stays_refused_and_what_stays_as_it_was(zj, ctx, torch, synth, je):
    """a gray file with the flag and a YCbCr decoder: ZJ_ERR_UNSUPPORTED, nothing written; as GRAYSCALE: the one-channel
    tensor of the fused kernel; a colour file with the flags set: the bytes of a decoder without them"""
    blob = gray_file(je, synth)
    o = options(zj)
    o.out_colorspace = zj.ColorSpace.YCbCr
    rc, got, text = tensor_call(zj, ctx, torch, blob, o, (0, 0, 16, 16), rm.F32, "NCHW", None, None, False)
    assert rc == UNSUPPORTED and "GRAY_TO_RGB" in text and bool((got == 0xAA).all())
    rc, got, text = tensor_call(zj, ctx, torch, blob, options(zj), (110, 0, 16, 16), rm.F32, "NCHW", None, None, False)
    assert rc == ARG and bool((got == 0xAA).all())  # a window that leaves the image
    rc, got, text = tensor_call(zj, ctx, torch, blob, options(zj), (0, 0, 16, 16), 4, "NCHW", None, None, False)
    assert rc == ARG  # no such dtype
    # without the flag a gray file of a colour decoder stays refused, turned or not, with a text that names the flag
    for o in (None, 6):
        rc, got, text = tensor_call(zj, ctx, torch, gray_file(je, synth, orientation=o), options(zj, flags=0), (0, 0, 16, 16), rm.F32,
                                    "NCHW", None, None, False, oriented=True)
        assert rc == UNSUPPORTED and "GRAY_TO_RGB" in text and bool((got == 0xAA).all()), (o, rc, text)
    colour = colour_file(je, synth, 97, 61, 2, 2, 4)
    win = (3, 5, 33, 17)
    rc0, plain, _ = tensor_call(zj, ctx, torch, colour, options(zj, flags=0), win, rm.BF16, "NCHW", None, None, True)
    rc1, flagged, _ = tensor_call(zj, ctx, torch, colour, options(zj), win, rm.BF16, "NCHW", None, None, True)
    assert rc0 == 0 and rc1 == 0 and torch.equal(plain, flagged)


# ---- 3. orientation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", range(1, 9))
def test_oriented_call_equals_the_resized_oriented_call(zj, ctx, torch, synth, je, o):
    rng = np.random.default_rng(80 + o)
    files = [("colour", colour_file(je, synth, 40, 24, 2, 2, o, orientation=o), 40, 24),
             ("gray", gray_file(je, synth, orientation=o), 120, 50),
             ("cmyk", four_file(synth, 48, 40, "hv", seed=9, adobe=2, orientation=o), 48, 40)]
    opt = options(zj)
    for name, blob, W, H in files:
        dw, dh = om.oriented_size(o, W, H)
        win = (3, 2, dw - 7, dh - 5)  # displayed pixels, not the whole image
        for (dtype, layout, flip) in ((rm.F32, "NHWC", True), (rm.BF16, "NCHW", False)):
            scale, bias = factors(rng, 3)
            rc, got, text = tensor_call(zj, ctx, torch, blob, opt, win, dtype, layout, scale, bias, flip, oriented=True)
            assert rc == 0, (name, o, rc, text)
            ref = resized_call(zj, ctx, torch, blob, opt, win, dtype, layout, scale, bias, flip, oriented=True)
            assert torch.equal(got, ref), f"{name} orientation {o} dtype {dtype} {layout}: {int((got != ref).sum())} bytes differ"
            if o == 1:  # the un-oriented call as it is
                rc, plain, _ = tensor_call(zj, ctx, torch, blob, opt, win, dtype, layout, scale, bias, flip, oriented=False)
                assert rc == 0 and torch.equal(got, plain)


# ---- 4. the batch call --------------------------------------------------------------------------------------------------------
def batch_files(synth, je):
    """twelve files: (blob, fails) -- ordinary 4:2:0 / 4:4:4, gray, CMYK, odd, two turned, one damaged"""
    plain = colour_file(je, synth, 96, 72, 2, 2, 1)
    return [plain, colour_file(je, synth, 97, 61, 1, 1, 2), gray_file(je, synth), colour_file(je, synth, 200, 40, 2, 1, 3),
            four_file(synth, 100, 75, "hv", 21, adobe=2), odd_file(synth, 100, 75, sc.SAMPLINGS[0], 21),
            colour_file(je, synth, 64, 48, 2, 2, 5, orientation=6), plain[:300], gray_file(je, synth, 72, 120, 5, orientation=8),
            colour_file(je, synth, 80, 64, 1, 2, 6), colour_file(je, synth, 57, 33, 2, 2, 7), colour_file(je, synth, 130, 90, 2, 2, 8)]


I_DAMAGED, I_LEAVES = 7, 10


def test_batch_of_every_kind(zj, tz, ctx, torch, synth, je):
    blobs = batch_files(synth, je)
    n, w, h = len(blobs), 24, 16
    assert n == 12
    opt = options(zj)
    rng = np.random.default_rng(12)
    origins = [(1 + k % 3, 2 + k % 2) for k in range(n)]
    origins[I_LEAVES] = (57 - w + 1, 0)  # leaves the 57 x 33 image
    flips = [bool(k % 2) for k in range(n)]
    scale, bias = factors(rng, 3)
    for (dtype, layout) in [(rm.BF16, "NCHW"), (rm.F32, "NHWC")]:
        per = 3 * w * h * ESZ[dtype]
        decs = []
        for k, b in enumerate(blobs):
            dec = zj.Decoder(opt, ctx)
            try:
                dec.prepare(b)
            except zj.ZjError:
                assert k == I_DAMAGED
            decs.append(dec)
        buf = guarded(torch, n * per)
        rcs = zj.finish_pixels_crop_tensor_batch(decs, ctx, origins, w, h, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, n * per,
                                                 scale, bias, flips, apply_orientation=True)
        for d in decs:
            d.close()
        got = body(torch, buf, n * per)
        for k in range(n):
            img = got[k * per:(k + 1) * per]
            if k == I_DAMAGED:
                assert rcs[k] != 0 and bool((img == 0xAA).all())
                continue
            rc, one, text = tensor_call(zj, ctx, torch, blobs[k], opt, origins[k] + (w, h), dtype, layout, scale, bias, flips[k], oriented=True)
            assert rcs[k] == rc, (k, rcs, text)
            assert torch.equal(img, one), (dtype, layout, k)  # (a failed file: the poison in both)
            assert (rc != 0) == (k == I_LEAVES), (k, rc, text)
    # the same through the tensors wrapper
    good = [k for k in range(n) if k not in (I_DAMAGED, I_LEAVES)]
    out = tz.decode_files_cropped_to_tensor(ctx, [blobs[k] for k in good], [origins[k] for k in good], (w, h), dtype=torch.float32,
                                            layout="NHWC", mean=MEAN, std=STD, flips=[flips[k] for k in good], options=opt, workers=2,
                                            apply_orientation=True)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (len(good), h, w, 3)
    s, b = tz.normalize_factors(3, MEAN, STD)
    for i, k in enumerate(good):
        rc, one, _ = tensor_call(zj, ctx, torch, blobs[k], opt, origins[k] + (w, h), rm.F32, "NHWC", s, b, flips[k], oriented=True)
        assert rc == 0 and torch.equal(out[i].reshape(-1).view(torch.uint8), one), k
    with pytest.raises(zj.DecodeError) as e:  # the window that leaves its image is the first failure of these
        tz.decode_files_cropped_to_tensor(ctx, [blobs[0], blobs[2], blobs[I_LEAVES], blobs[4]], [origins[0], origins[2], origins[I_LEAVES], origins[4]],
                                          (w, h), options=opt, workers=2, apply_orientation=True)
    assert "file 2" in str(e.value)
    with pytest.raises(zj.DecodeError) as e:
        tz.decode_files_cropped_to_tensor(ctx, [blobs[0], blobs[I_DAMAGED], blobs[2]], [(0, 0)] * 3, (w, h), options=opt, workers=2,
                                          apply_orientation=True)
    assert "file 1" in str(e.value)
    # origins=None: the DISPLAYED size must be `size`
    turned = blobs[6]  # 64 x 48 stored, orientation 6: 48 x 64 displayed
    whole = tz.decode_files_cropped_to_tensor(ctx, [turned], None, (48, 64), dtype=torch.uint8, layout="NHWC", options=opt, apply_orientation=True)
    torch.cuda.synchronize()
    assert tuple(whole.shape) == (1, 64, 48, 3)
    with pytest.raises(ValueError):
        tz.decode_files_cropped_to_tensor(ctx, [turned], None, (64, 48), options=opt, apply_orientation=True)
