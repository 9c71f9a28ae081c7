"""GPU: crop windows decoded straight into a normalised tensor (zj_decode_crops_tensor_device,
tensors.decode_crops_to_normalized_tensor) on an MI355X.  The output must be, byte for byte, what the
library's own older paths give: zj_decode_crops_resized_device with out == window (the definition), and the numpy
conversion (tests/resize_model.py's factors and roundings) of the u8 crop zj_decode_crops_device writes for the window.
Guard bytes in front of image 0 and behind the last stay untouched."""
import importlib
import zlib

import numpy as np
import pytest

import resize_model as rm
from test_gpu_crop import TAIL_WIDTHS

pytestmark = pytest.mark.gpu
MODES = {"none": (1, 1), "h": (2, 1), "v": (1, 2), "hv": (2, 2)}
KINDS = {"rgb": 0, "gray": 1, "ycbcr": 2}
GUARD = 256
ESZ = {rm.F32: 4, rm.F16: 2, rm.BF16: 2, rm.U8: 1}
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


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


def frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed, index=0):
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=seed, frame_index=index)
    d = zj.FrameDesc.make(W, H, hs, vs, 3, KINDS[kind], qts)
    d.flags = flags
    dev = [torch.from_numpy(np.ascontiguousarray(p, np.int16)).cuda() for p in planes]
    torch.cuda.synchronize()  # (the uploads are torch's, the reads the library's stream)
    return d, dev


def ptrs(frames):
    return [f[0].data_ptr() for f in frames], [f[1].data_ptr() for f in frames], [f[2].data_ptr() for f in frames]


def guarded(torch, nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


def body(torch, buf, nbytes):
    """the tensor's bytes (still on the device) after checking the guards"""
    assert bool((buf[:GUARD] == 0xAA).all()) and bool((buf[GUARD + nbytes:] == 0xAA).all()), "a byte outside the tensor was written"
    return buf[GUARD:GUARD + nbytes]


def layout_code(zj, layout):
    return zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW


def run_tensor(zj, ctx, torch, d, frames, origins, w, h, dtype, layout, scale, bias, flips):
    ch = zj.num_components(d.out_colorspace)
    per = zj.crop_tensor_out_len(d, w, h, dtype)
    assert per == ch * w * h * ESZ[dtype]
    buf = guarded(torch, len(frames) * per)
    y, cb, cr = ptrs(frames)
    ctx.decode_crops_tensor_device(d, y, cb, cr, origins, w, h, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, scale, bias,
                                   flips)
    ctx.sync()
    return body(torch, buf, len(frames) * per)


def run_resized_identity(zj, ctx, torch, d, frames, origins, w, h, dtype, layout, scale, bias, flips):
    ch = zj.num_components(d.out_colorspace)
    per = ch * w * h * ESZ[dtype]
    buf = guarded(torch, len(frames) * per)
    y, cb, cr = ptrs(frames)
    ctx.decode_crops_resized_device(d, y, cb, cr, [(x, yy, w, h) for (x, yy) in origins], w, h, dtype, layout_code(zj, layout),
                                    buf.data_ptr() + GUARD, scale, bias, flips)
    ctx.sync()
    return body(torch, buf, len(frames) * per)


def run_u8_crops(zj, ctx, torch, d, frames, origins, w, h):
    """[N, h, w, C] uint8 on the host: zj_decode_crops_device's crops"""
    ch = zj.num_components(d.out_colorspace)
    ln = zj.crop_out_len(d, w, h, 0)
    assert ln == w * h * ch
    buf = guarded(torch, len(frames) * ln)
    y, cb, cr = ptrs(frames)
    ctx.decode_crops_device(d, y, cb, cr, origins, w, h, [buf.data_ptr() + GUARD + i * ln for i in range(len(frames))], 0)
    ctx.sync()
    return body(torch, buf, len(frames) * ln).cpu().numpy().reshape(len(frames), h, w, ch)


def convert(crops, dtype, layout, scale, bias, flips):
    """the definition over u8 crops [N, h, w, C]: the tensor's bytes"""
    n, h, w, ch = crops.shape
    x = crops
    if flips is not None:
        x = np.stack([c[:, ::-1] if f else c for c, f in zip(crops, flips)])
    if dtype == rm.U8:
        out = x
    else:
        s, b = rm.factors(ch, scale, bias)
        v = (x.astype(np.uint32) << 16).astype(np.float32)
        yv = (v * s).astype(np.float32)
        yv = (yv + b).astype(np.float32)
        if dtype == rm.F32:
            out = yv
        elif dtype == rm.F16:
            with np.errstate(over="ignore"):
                out = yv.astype(np.float16)
        else:
            out = rm.bf16_bits(yv)
    if layout == "NCHW":
        out = out.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1)


def same(torch, got, exp_dev=None, exp_host=None, what=""):
    if exp_dev is not None and not torch.equal(got, exp_dev):
        raise AssertionError(f"{what}: {int((got != exp_dev).sum())} bytes differ from the identity-size resized call")
    if exp_host is not None:
        g = got.cpu().numpy()
        if not np.array_equal(g, exp_host):
            bad = np.nonzero(g != exp_host)[0]
            raise AssertionError(f"{what}: {bad.size} bytes differ from the converted u8 crop, first at {bad[:6].tolist()}")


def factors(rng, ch):
    return rng.uniform(0.002, 0.03, ch).astype(np.float32), rng.uniform(-3, 3, ch).astype(np.float32)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_random_windows_equal_the_existing_paths(zj, ctx, torch, synth, mode, kind):
    hs, vs = MODES[mode]
    ch = 1 if kind == "gray" else 3
    rng = np.random.default_rng(zlib.crc32(f"tensor-{mode}-{kind}".encode()))
    for (W, H, flags) in [(2500, 120, 0), (1040, 72, 7), (13, 9, 0)]:
        d, dev = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed=W)
        if zj.crop_out_len(d, 1, 1) == 0:  # (a reference panic: the new call refuses the frame as the crop does)
            assert zj.crop_tensor_out_len(d, 1, 1, rm.F32) == 0
            with pytest.raises(zj.ZjError):
                ctx.decode_crops_tensor_device(d, *ptrs([dev]), [(0, 0)], 1, 1, rm.F32, 0, dev[0].data_ptr())
            continue
        for _ in range(4):  # 4 sizes x 50 windows
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for _ in range(50)]
            dtype, layout = int(rng.integers(4)), ("NCHW", "NHWC")[int(rng.integers(2))]
            flips = [bool(rng.integers(2)) for _ in range(50)] if rng.integers(4) else None
            scale, bias = factors(rng, ch)
            args = (zj, ctx, torch, d, [dev] * 50, origins, w, h, dtype, layout, scale, bias, flips)
            got = run_tensor(*args)
            crops = run_u8_crops(zj, ctx, torch, d, [dev] * 50, origins, w, h)
            same(torch, got, run_resized_identity(*args), convert(crops, dtype, layout, scale, bias, flips),
                 f"{mode} {kind} {W}x{H} flags {flags} window {w}x{h} dtype {dtype} {layout}")


@pytest.mark.parametrize("W", TAIL_WIDTHS)
@pytest.mark.parametrize("mode", ["h", "hv"])
def test_tail_widths(zj, ctx, torch, synth, W, mode):
    """the row ends with the hole and the early RGB tail: windows over the row's end, bf16 NCHW and f32 NHWC"""
    hs, vs = MODES[mode]
    H = 40
    d, dev = frame_on_device(zj, torch, synth, W, H, hs, vs, "rgb", 0, seed=W)
    rng = np.random.default_rng(W)
    scale, bias = factors(rng, 3)
    for (dtype, layout) in [(rm.BF16, "NCHW"), (rm.F32, "NHWC")]:
        for w in (1, 5, 16, 21, 23, 40, min(W, 300), W):
            origins = [(W - w, 0), (W - w, H - 7), (W - w, 17)]
            flips = [False, True, True]
            args = (zj, ctx, torch, d, [dev] * 3, origins, w, 7, dtype, layout, scale, bias, flips)
            crops = run_u8_crops(zj, ctx, torch, d, [dev] * 3, origins, w, 7)
            same(torch, run_tensor(*args), run_resized_identity(*args), convert(crops, dtype, layout, scale, bias, flips),
                 f"tail {mode} W {W} w {w} dtype {dtype}")


@pytest.mark.parametrize("n", [1, 31, 32, 33, 100])
def test_batch_sizes(zj, ctx, torch, synth, n):
    """the ZJ_SCATTER_MAX split and the dense image stride: every frame its own origin and flip"""
    W, H = 2500, 72
    rng = np.random.default_rng(n)
    distinct = [frame_on_device(zj, torch, synth, W, H, 2, 2, "rgb", 0, seed=21, index=i) for i in range(min(n, 5))]
    d = distinct[0][0]
    frames = [distinct[i % len(distinct)][1] for i in range(n)]
    w, h = 225, 41  # (odd: an image of bf16 starts on a 2-byte boundary only)
    origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for _ in range(n)]
    flips = [bool(rng.integers(2)) for _ in range(n)]
    scale, bias = factors(rng, 3)
    args = (zj, ctx, torch, d, frames, origins, w, h, rm.BF16, "NCHW", scale, bias, flips)
    crops = run_u8_crops(zj, ctx, torch, d, frames, origins, w, h)
    same(torch, run_tensor(*args), run_resized_identity(*args), convert(crops, rm.BF16, "NCHW", scale, bias, flips), f"batch of {n}")


def test_whole_frame(zj, ctx, torch, synth):
    """4096 x 64 in 4:2:0 -> f32 NCHW, against the conversion of the full device decode"""
    import ctypes as C
    W, H = 4096, 64
    d, dev = frame_on_device(zj, torch, synth, W, H, 2, 2, "rgb", 0, seed=4)
    full = torch.full((zj.lib().zj_out_len(C.byref(d)),), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_planes_device(d, 1, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), full.data_ptr())
    ctx.sync()
    crops = full.cpu().numpy().reshape(1, H, W, 3)
    scale, bias = np.float32(1 / (255 * np.float32(STD))), np.float32(-np.float32(MEAN) / np.float32(STD))
    got = run_tensor(zj, ctx, torch, d, [dev], [(0, 0)], W, H, rm.F32, "NCHW", scale, bias, None)
    same(torch, got, None, convert(crops, rm.F32, "NCHW", scale, bias, None), "whole frame")


def test_rejects_bad_arguments(zj, ctx, torch, synth):
    """each with its status, and nothing written"""
    import ctypes as C
    L = zj.lib()
    d, dev = frame_on_device(zj, torch, synth, 64, 32, 2, 2, "rgb", 0, seed=2)
    buf = guarded(torch, 3 * 8 * 8 * 4)
    out = C.c_void_p(buf.data_ptr() + GUARD)
    P = lambda t: (C.c_void_p * 1)(t.data_ptr())
    y, cb, cr = P(dev[0]), P(dev[1]), P(dev[2])
    org = (C.c_uint * 2)(0, 0)
    ok = (C.c_float * 3)(1.0, 1.0, 1.0)
    inf = (C.c_float * 3)(1.0, float("inf"), 1.0)
    nan = (C.c_float * 3)(float("nan"), 0.0, 0.0)
    h = ctx.handle
    call = lambda desc, n, yy, o, w, hh, dt, lay, sc, bi, dst: L.zj_decode_crops_tensor_device(
        h, C.byref(desc), n, yy, cb, cr, o, w, hh, dt, lay, sc, bi, None, dst, None)
    ARG, UNSUPPORTED = -1, -2
    assert call(d, 1, y, org, 8, 8, 4, 0, ok, ok, out) == ARG           # no such dtype
    assert call(d, 1, y, org, 8, 8, 0, 2, ok, ok, out) == ARG           # no such layout
    assert call(d, 1, y, org, 8, 8, 0, 0, inf, ok, out) == ARG and call(d, 1, y, org, 8, 8, 0, 0, ok, nan, out) == ARG
    assert call(d, 0, y, org, 8, 8, 0, 0, ok, ok, out) == ARG and call(d, 1, None, org, 8, 8, 0, 0, ok, ok, out) == ARG
    assert call(d, 1, y, None, 8, 8, 0, 0, ok, ok, out) == ARG and call(d, 1, y, org, 8, 8, 0, 0, ok, ok, None) == ARG
    assert call(d, 1, y, org, 0, 8, 0, 0, ok, ok, out) == ARG and call(d, 1, y, org, 65, 8, 0, 0, ok, ok, out) == ARG
    assert call(d, 1, y, (C.c_uint * 2)(60, 0), 8, 8, 0, 0, ok, ok, out) == ARG   # leaves the frame
    assert call(d, 1, y, org, 8, 8, 0, 0, ok, ok, C.c_void_p(buf.data_ptr() + GUARD + 2)) == ARG  # not aligned to a float
    for cs, layout, pitch in ((5, 0, 0), (0, 1, 0), (0, 0, 256)):  # RGBA; CHW planes; a frame pitch
        e = zj.FrameDesc.make(64, 32, 2, 2, 3, cs, [np.ones(64, np.int32)] * 3)
        e.out_layout, e.out_pitch = layout, pitch
        assert call(e, 1, y, org, 8, 8, 0, 0, ok, ok, out) == UNSUPPORTED
        assert zj.crop_tensor_out_len(e, 8, 8, 0) == 0
    ctx.sync()
    assert bool((buf == 0xAA).all()), "a refused call wrote"
    assert call(d, 1, y, org, 8, 8, 0, 0, ok, ok, out) == 0
    ctx.sync()


def test_tensors_wrapper(zj, ctx, torch, synth):
    """tensors.decode_crops_to_normalized_tensor: shapes, dtypes, equality with the raw call, and torch's own
    (x / 255 - mean) / std within the bf16 rounding profiles/resize_crop.txt records for the resized path (0.0156)"""
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    W, H, n, w, h = 600, 300, 6, 224, 224
    rng = np.random.default_rng(9)
    frames = []
    for i in range(n):
        d, dev = frame_on_device(zj, torch, synth, W, H, 2, 2, "rgb", 0, seed=31, index=i)
        frames.append(tuple(dev))
    origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for _ in range(n)]
    flips = [bool(i & 1) for i in range(n)]
    u8 = tensors.decode_crops_to_tensor(ctx, d, frames, origins, (w, h))
    torch.cuda.synchronize()
    x = torch.stack([u8[i].flip(1) if flips[i] else u8[i] for i in range(n)]).float() / 255
    ref = (x - torch.tensor(MEAN, device="cuda")) / torch.tensor(STD, device="cuda")
    scale, bias = tensors.normalize_factors(3, MEAN, STD)
    for dtype, code in ((torch.bfloat16, rm.BF16), (torch.float32, rm.F32), (torch.float16, rm.F16)):
        for layout in ("NCHW", "NHWC"):
            out = tensors.decode_crops_to_normalized_tensor(ctx, d, frames, origins, (w, h), dtype=dtype, layout=layout,
                                                            mean=MEAN, std=STD, flips=flips)
            torch.cuda.synchronize()
            assert out.dtype == dtype and out.is_contiguous()
            assert tuple(out.shape) == ((n, 3, h, w) if layout == "NCHW" else (n, h, w, 3))
            raw = run_tensor(zj, ctx, torch, d, frames, origins, w, h, code, layout, np.float32(scale), np.float32(bias), flips)
            assert torch.equal(out.view(torch.uint8).reshape(-1), raw)
            nhwc = out.permute(0, 2, 3, 1) if layout == "NCHW" else out
            assert float((nhwc.float() - ref).abs().max()) <= 0.0156
    out = tensors.decode_crops_to_normalized_tensor(ctx, d, frames, origins, (w, h), dtype=torch.uint8, layout="NHWC")
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and torch.equal(out, u8)
    with pytest.raises(ValueError):
        tensors.decode_crops_to_normalized_tensor(ctx, d, frames, origins, (W + 1, h))


# ---- the file path ------------------------------------------------------------------------------------------------------
def _files():
    import glob
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return [os.path.join(g, "test-baseline.jpg")] + sorted(glob.glob(os.path.join(g, "ref", "*.jp*g")))


def _opts(zj, entropy, cs=None):
    o = zj.ZuneJpegOptions()
    if entropy == "gpu":
        o.entropy = zj.ENTROPY_GPU_ALWAYS
    if cs is not None:
        o.out_colorspace = cs
    return o


@pytest.mark.parametrize("entropy", ["cpu", "gpu"])
def test_file_call_equals_the_converted_full_decode(zj, torch, entropy):
    """zj_decoder_finish_pixels_crop_tensor_device under the CPU walker and under device entropy == the conversion of the
    window of the same decoder's full device decode; it also equals the resized file call at out == window"""
    import ctypes as C
    import os
    rng = np.random.default_rng(zlib.crc32(f"file-{entropy}".encode()))
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    checked = 0
    try:
        for path in _files():
            data = open(path, "rb").read()
            dec = zj.Decoder(_opts(zj, entropy), ctx)
            try:
                desc, info = dec.prepare(data)
            except zj.ZjError:
                dec.close()
                continue
            if info.components == 1:  # (a one-component file has its tensor with a decoder that asks for GRAYSCALE)
                dec.close()
                dec = zj.Decoder(_opts(zj, entropy, zj.ColorSpace.GRAYSCALE), ctx)
                desc, info = dec.prepare(data)
            n = zj.lib().zj_out_len(C.byref(desc))
            W, H = desc.width, desc.height
            ch = n // (W * H)
            if ch not in (1, 3) or zj.crop_tensor_out_len(desc, 1, 1, 0) == 0:
                dec.close()
                continue
            full = torch.empty(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert dec.finish_pixels_device(full.data_ptr(), n) == n
            img = full.cpu().numpy().reshape(H, W, ch)
            for k in range(4):
                w, h = int(rng.integers(1, min(W, 700) + 1)), int(rng.integers(1, min(H, 500) + 1))
                x, y = (int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) if k else (W - w, H - h)
                dtype, layout, flip = k % 4, ("NHWC" if k % 2 else "NCHW"), bool(k % 3)
                scale, bias = factors(rng, ch)
                per = zj.crop_tensor_out_len(desc, w, h, dtype)
                buf = guarded(torch, per)
                dec.prepare(data)
                assert dec.finish_pixels_crop_tensor_device(x, y, w, h, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, per,
                                                            scale, bias, flip) == per
                got = body(torch, buf, per)
                what = f"{os.path.basename(path)} {entropy} window {(x, y, w, h)} dtype {dtype} {layout}"
                same(torch, got, None, convert(img[None, y:y + h, x:x + w], dtype, layout, scale, bias, [flip]), what)
                buf2 = guarded(torch, per)
                dec.prepare(data)
                assert dec.finish_pixels_resized_crop_device(x, y, w, h, w, h, dtype, layout_code(zj, layout),
                                                             buf2.data_ptr() + GUARD, per, scale, bias, flip=flip) == per
                same(torch, got, body(torch, buf2, per), None, what)
                checked += 1
            # a buffer one byte short, a window that leaves the image: refused, nothing written
            buf = guarded(torch, 64)
            dec.prepare(data)
            for args in ((0, 0, 2, 2, 0, 0, buf.data_ptr() + GUARD, ch * 16 - 1), (W - 1, 0, 2, 2, 0, 0, buf.data_ptr() + GUARD, 64)):
                with pytest.raises(zj.ZjError) as e:
                    dec.finish_pixels_crop_tensor_device(*args)
                assert e.value.status == -1
            assert bool((buf == 0xAA).all())
            dec.close()
    finally:
        ctx.close()
    assert checked >= 12


def test_file_call_refuses_what_only_the_resized_calls_finish(zj, torch):
    """a one-component file asked for RGB is ZJ_ERR_UNSUPPORTED with a text that names the flag; as GRAYSCALE it has a
    one-channel tensor"""
    import ctypes as C
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "tools"))
    import jpeg_enc
    synth = importlib.import_module("zune-jpeg_amd.synth")
    W, H = 120, 50
    data = jpeg_enc.encode_baseline(jpeg_enc.small_planes(W, H, 1, 1, 1, seed=3), synth.quant_tables(85), W, H, 1, 1, 1)
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    try:
        buf = guarded(torch, 3 * 16 * 16 * 4)
        dec = zj.Decoder(_opts(zj, "cpu", zj.ColorSpace.RGB), ctx)
        dec.prepare(data)
        with pytest.raises(zj.ZjError) as e:
            dec.finish_pixels_crop_tensor_device(0, 0, 16, 16, rm.F32, 0, buf.data_ptr() + GUARD, 3 * 16 * 16 * 4)
        assert e.value.status == -2 and "GRAY_TO_RGB" in str(e.value)
        assert bool((buf == 0xAA).all())
        dec.close()
        dec = zj.Decoder(_opts(zj, "cpu", zj.ColorSpace.GRAYSCALE), ctx)
        desc, _ = dec.prepare(data)
        n = zj.lib().zj_out_len(C.byref(desc))
        full = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert dec.finish_pixels_device(full.data_ptr(), n) == n == W * H
        img = full.cpu().numpy().reshape(H, W, 1)
        dec.prepare(data)
        per = 33 * 17 * 2
        buf = guarded(torch, per)
        assert dec.finish_pixels_crop_tensor_device(80, 30, 33, 17, rm.BF16, 1, buf.data_ptr() + GUARD, per, [0.01], [-1.5], True) == per
        same(torch, body(torch, buf, per), None,
             convert(img[None, 30:47, 80:113], rm.BF16, "NHWC", np.float32([0.01]), np.float32([-1.5]), [True]), "gray file")
        dec.close()
    finally:
        ctx.close()


def test_files_wrapper(zj, ctx, torch):
    """tensors.decode_files_cropped_to_tensor: image k is the single-file call's; origins=None wants files of exactly `size`"""
    import ctypes as C
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    import os
    want = ("test-baseline.jpg", "medium_horiz_samp_2500x1786.jpg", "medium_no_samp_2500x1786.jpg", "speed_bench_hv_subsampling.jpg")
    paths = [p for p in _files() if os.path.basename(p) in want]
    assert len(paths) == 4
    blobs = [open(p, "rb").read() for p in paths]
    w, h = 96, 64
    rng = np.random.default_rng(4)
    decs = []
    sizes = []
    for b in blobs:
        d = zj.Decoder(zj.ZuneJpegOptions(), ctx)
        desc, _ = d.prepare(b)
        sizes.append((desc.width, desc.height))
        d.close()
    origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for (W, H) in sizes]
    flips = [True, False, True, False][:len(blobs)]
    out = tensors.decode_files_cropped_to_tensor(ctx, blobs, origins, (w, h), dtype=torch.float16, layout="NHWC", mean=MEAN, std=STD,
                                                 flips=flips, workers=2, decoders=decs)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and tuple(out.shape) == (len(blobs), h, w, 3) and len(decs) == len(blobs)
    scale, bias = tensors.normalize_factors(3, MEAN, STD)
    per = 3 * w * h * 2
    for k, b in enumerate(blobs):
        buf = guarded(torch, per)
        dec = zj.Decoder(zj.ZuneJpegOptions(), ctx)
        dec.prepare(b)
        assert dec.finish_pixels_crop_tensor_device(origins[k][0], origins[k][1], w, h, rm.F16, 1, buf.data_ptr() + GUARD, per, scale,
                                                    bias, flips[k]) == per
        dec.close()
        assert torch.equal(out[k].reshape(-1).view(torch.uint8), body(torch, buf, per)), k
    whole = tensors.decode_files_cropped_to_tensor(ctx, blobs[:1], None, sizes[0], dtype=torch.uint8, layout="NHWC")
    torch.cuda.synchronize()
    n = 3 * sizes[0][0] * sizes[0][1]
    full = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dec = zj.Decoder(zj.ZuneJpegOptions(), ctx)
    dec.prepare(blobs[0])
    assert dec.finish_pixels_device(full.data_ptr(), n) == n
    dec.close()
    assert torch.equal(whole.reshape(-1), full)
    with pytest.raises(ValueError):
        tensors.decode_files_cropped_to_tensor(ctx, blobs[:2], None, (sizes[0][0] + 1, sizes[0][1]))
    with pytest.raises(zj.DecodeError) as e:  # a damaged file in the middle: named by its index
        tensors.decode_files_cropped_to_tensor(ctx, [blobs[0], blobs[1][:300], blobs[2]], [(0, 0)] * 3, (w, h))
    assert "file 1" in str(e.value)


# ---- frames of mixed geometry, files in batches ----------------------------------------------------------------------------
def test_mixed_call_equals_the_one_geometry_call(zj, ctx, torch, synth):
    """40 frames of different sizes, modes, tables and flags, one window size: image f is the one-geometry call's for frame f
    alone; one refused frame in the middle (a window that leaves it) leaves nothing written"""
    rng = np.random.default_rng(40)
    w, h = 96, 40
    modes = list(MODES.values())
    descs, frames, origins = [], [], []
    for i in range(40):
        W, H = int(rng.integers(w, 1300)), int(rng.integers(h, 200))
        if i % 9 == 0:
            W = [257, 261, 513, 517, 1029][(i // 9) % 5]
        hs, vs = modes[i % 4]
        d, dev = frame_on_device(zj, torch, synth, W, H, hs, vs, "rgb", 7 if i % 5 == 0 else 0, seed=500 + i, index=i)
        if zj.crop_out_len(d, 1, 1) == 0:
            continue
        descs.append(d); frames.append(dev)
        origins.append((W - w, H - h) if i % 4 == 0 else (int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))))
    n = len(frames)
    assert n >= 36
    flips = [bool(i % 3 == 0) for i in range(n)]
    for (dtype, layout) in [(rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NCHW")]:
        scale, bias = factors(rng, 3)
        per = 3 * w * h * ESZ[dtype]
        buf = guarded(torch, n * per)
        y, cb, cr = ptrs(frames)
        ctx.decode_crops_tensor_mixed_device(descs, y, cb, cr, origins, w, h, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD,
                                             scale, bias, flips)
        ctx.sync()
        got = body(torch, buf, n * per)
        for f in range(n):
            one = run_tensor(zj, ctx, torch, descs[f], [frames[f]], [origins[f]], w, h, dtype, layout, scale, bias, [flips[f]])
            assert torch.equal(got[f * per:(f + 1) * per], one), (dtype, layout, f, descs[f].width, descs[f].height)
    bad = list(origins)
    bad[n // 2] = (descs[n // 2].width - w + 1, 0)
    buf = guarded(torch, n * per)
    with pytest.raises(zj.ZjError) as e:
        ctx.decode_crops_tensor_mixed_device(descs, *ptrs(frames), bad, w, h, rm.U8, 0, buf.data_ptr() + GUARD, None, None, flips)
    ctx.sync()
    assert e.value.status == -1 and bool((buf == 0xAA).all()), "a refused mixed call wrote"


@pytest.mark.parametrize("entropy", ["cpu", "mixed"])
def test_batch_file_call(zj, torch, synth, entropy):
    """about 20 synthetic and real files of different sizes in one batch call, a damaged file and a gray file among colour
    ones in the middle: rcs, the untouched images of the failed files, every other image the single-file call's.
    entropy "mixed": every third decoder leaves its scan for the device (those go file by file)."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "tools"))
    import jpeg_enc
    rng = np.random.default_rng(zlib.crc32(f"batch-{entropy}".encode()))
    w, h = 64, 48
    blobs = []
    for i in range(14):
        W, H = int(rng.integers(w, 700)), int(rng.integers(h, 300))
        hs, vs = list(MODES.values())[i % 4]
        blobs.append(jpeg_enc.encode_baseline(jpeg_enc.small_planes(W, H, hs, vs, 3, seed=i), synth.quant_tables(60 + 2 * i), W, H, hs, vs, 3))
    want = ("test-baseline.jpg", "medium_horiz_samp_2500x1786.jpg", "medium_no_samp_2500x1786.jpg", "medium_vertical_samp_2500x1786.jpg",
            "speed_bench_hv_subsampling.jpg")
    blobs += [open(p, "rb").read() for p in _files() if os.path.basename(p) in want]
    gray = jpeg_enc.encode_baseline(jpeg_enc.small_planes(120, 90, 1, 1, 1, seed=3), synth.quant_tables(85), 120, 90, 1, 1, 1)
    damaged = blobs[2][:300]  # (cut inside its tables: a file cut in its scan still decodes, as in the reference)
    i_bad, i_gray = 8, 11
    blobs.insert(i_bad, damaged)
    blobs.insert(i_gray, gray)
    n = len(blobs)
    assert n >= 20
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    try:
        decs, sizes, failed_prepare = [], [], set()
        for k, b in enumerate(blobs):
            dec = zj.Decoder(_opts(zj, "gpu" if entropy == "mixed" and k % 3 == 1 else "cpu"), ctx)
            try:
                desc, _ = dec.prepare(b)
                sizes.append((desc.width, desc.height))
            except zj.ZjError:
                failed_prepare.add(k)
                sizes.append((w, h))
            decs.append(dec)
        origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for (W, H) in sizes]
        flips = [bool(k % 2) for k in range(n)]
        scale, bias = factors(rng, 3)
        for (dtype, layout) in [(rm.BF16, "NCHW"), (rm.F32, "NHWC")]:
            per = 3 * w * h * ESZ[dtype]
            buf = guarded(torch, n * per)
            for k, b in enumerate(blobs):  # (a refused file leaves its decoder in error: every call starts from prepared files)
                if k not in failed_prepare:
                    decs[k].prepare(b)
            rcs = zj.finish_pixels_crop_tensor_batch(decs, ctx, origins, w, h, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD,
                                                     n * per, scale, bias, flips)
            got = body(torch, buf, n * per)
            assert i_gray not in failed_prepare
            assert rcs[i_gray] == -2, (rcs, zj.lib().zj_decoder_error(decs[i_gray]._d))  # ZJ_ERR_UNSUPPORTED for the gray file only
            assert "GRAY_TO_RGB" in zj.lib().zj_decoder_error(decs[i_gray]._d).decode()
            for k in range(n):
                img = got[k * per:(k + 1) * per]
                if k == i_gray or rcs[k]:
                    assert rcs[k] != 0 and bool((img == 0xAA).all()), f"file {k}: status {rcs[k]}, image written"
                    continue
                one = guarded(torch, per)
                dec = zj.Decoder(_opts(zj, "cpu"), ctx)
                dec.prepare(blobs[k])
                assert dec.finish_pixels_crop_tensor_device(origins[k][0], origins[k][1], w, h, dtype, layout_code(zj, layout),
                                                            one.data_ptr() + GUARD, per, scale, bias, flips[k]) == per
                dec.close()
                assert torch.equal(img, body(torch, one, per)), (entropy, dtype, layout, k)
            bad = [k for k in range(n) if rcs[k]]
            assert i_bad in bad and set(bad) <= {i_bad, i_gray} | failed_prepare, rcs
        # a buffer one image short: the call itself is refused
        with pytest.raises(zj.ZjError):
            zj.finish_pixels_crop_tensor_batch(decs, ctx, origins, w, h, rm.U8, 0, buf.data_ptr() + GUARD, (n - 1) * 3 * w * h)
        for d in decs:
            d.close()
    finally:
        ctx.close()
