"""GPU: resized crop decode (zj_resize_device, zj_decode_crops_resized_device, zj_decoder_finish_pixels_resized_crop_device,
tensors.decode_resized_crops_to_tensor / resize_to_tensor) on an MI355X.  Every output must be, bit for bit, the numpy
model of the definition (tests/resize_model.py) applied to the u8 input -- for the crop entry points, to the crop that
zj_decode_crops_device itself writes for the same window; guard bytes around every output stay untouched."""
import ctypes as C
import glob
import importlib
import os
import zlib

import numpy as np
import pytest

import resize_model as rm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {"none": (1, 1), "h": (2, 1), "v": (1, 2), "hv": (2, 2)}
KINDS = {"rgb": (0, 0), "gray": (1, 0), "ycbcr": (2, 0), "chw": (0, 1)}
GUARD = 256
ESZ = {0: 4, 1: 2, 2: 2, 3: 1}


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


def channels_of(zj, d):
    return zj.num_components(d.out_colorspace)


def is_chw(zj, d):
    return d.out_layout == 1 and channels_of(zj, d) == 3


def out_buffer(torch, nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


def read_out(buf, nbytes):
    a = buf.cpu().numpy()
    assert (a[:GUARD] == 0xAA).all() and (a[GUARD + nbytes:] == 0xAA).all(), "an output byte outside the tensor was written"
    return a[GUARD:GUARD + nbytes]


def check_image(got_bytes, exp, dtype, what):
    got = rm.raw_view(got_bytes, dtype).reshape(exp.shape)
    if dtype == rm.F32:
        ok = np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    else:
        ok = np.array_equal(got, exp)
    if not ok:
        raise AssertionError(f"{what}: {(got.view(np.uint8) != exp.view(np.uint8)).sum()} bytes differ from the model")


def random_factors(rng, ch):
    return rng.uniform(0.002, 0.03, ch).astype(np.float32), rng.uniform(-3, 3, ch).astype(np.float32)


# ---- zj_resize_device over u8 images in device memory ------------------------------------------------------------------
CASES = [(c, chw, dt, lay) for c in (1, 3) for chw in ((False, True) if c == 3 else (False,)) for dt in range(4)
         for lay in ("NCHW", "NHWC")]


def _device_images(torch, rng, sizes, channels, chw):
    """the images at their own pitches and (unaligned) offsets in one device buffer: (buffer, pointers, pitches, [C,h,w])"""
    blobs, pitches, chws = [], [], []
    for (w, h) in sizes:
        img = rng.integers(0, 256, (channels, h, w), dtype=np.uint8)
        rows = img.transpose(1, 2, 0).reshape(h, w * channels) if (channels == 3 and not chw) else img.reshape(-1, w)
        pitch = rows.shape[1] + int(rng.integers(0, 40))
        buf = np.full((rows.shape[0], pitch), 0xEE, np.uint8)
        buf[:, :rows.shape[1]] = rows
        blobs.append(buf.reshape(-1))
        pitches.append(pitch)
        chws.append(img)
    offs, o = [], 0
    for b in blobs:
        o += int(rng.integers(0, 16))
        offs.append(o)
        o += b.size
    host = np.zeros(o + 16, np.uint8)
    for off, b in zip(offs, blobs):
        host[off:off + b.size] = b
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return dev, [dev.data_ptr() + off for off in offs], pitches, chws


@pytest.mark.parametrize("channels,chw,dtype,layout", CASES)
def test_resize_device_matches_the_model(zj, ctx, torch, channels, chw, dtype, layout):
    rng = np.random.default_rng(zlib.crc32(f"{channels}{chw}{dtype}{layout}".encode()))
    n = 40 if dtype != rm.BF16 else 150  # (above ZJ_SCATTER_MAX; 150: above the 128 images of one launch)
    sizes = [(int(rng.integers(1, 400)), int(rng.integers(1, 300))) for _ in range(n)]
    sizes[:3] = [(1, 1), (224, 224), (1000, 3)]
    dev, ptrs, pitches, chws = _device_images(torch, rng, sizes, channels, chw)
    flips = [bool(rng.integers(2)) for _ in range(n)]
    scale, bias = random_factors(rng, channels)
    for (ow, oh) in [(224, 224), (37, 5)]:
        per = channels * ow * oh * ESZ[dtype]
        buf = out_buffer(torch, n * per)
        ctx.resize_device(ptrs, sizes, channels, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, ow, oh, dtype,
                          zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW, buf.data_ptr() + GUARD, scale, bias, flips,
                          pitches)
        ctx.sync()
        out = read_out(buf, n * per)
        for i in range(n):
            exp = rm.resize(chws[i], ow, oh, dtype, scale, bias, flips[i], layout)
            check_image(out[i * per:(i + 1) * per], exp, dtype, f"image {i} {sizes[i]} -> {ow}x{oh}")


def test_resize_device_rejects_bad_arguments(zj, ctx, torch):
    L = zj.lib()
    buf = out_buffer(torch, 4096)
    p = C.c_void_p(buf.data_ptr() + GUARD)
    ptrs = (C.c_void_p * 1)(p)
    wh = (C.c_uint * 2)(8, 8)
    ok = (C.c_float * 3)(1.0, 1.0, 1.0)
    bad = (C.c_float * 3)(1.0, float("inf"), 1.0)
    nan = (C.c_float * 3)(float("nan"), 1.0, 1.0)
    h = ctx.handle
    assert L.zj_resize_device(h, 1, ptrs, wh, None, 3, 0, 4, 4, 2, 0, ok, ok, None, p, None) == 0
    ctx.sync()
    for args in [(1, ptrs, wh, None, 3, 0, 4, 4, 2, 0, bad, ok), (1, ptrs, wh, None, 3, 0, 4, 4, 2, 0, ok, nan),
                 (1, ptrs, wh, None, 2, 0, 4, 4, 2, 0, ok, ok), (1, ptrs, wh, None, 3, 2, 4, 4, 2, 0, ok, ok),
                 (1, ptrs, wh, None, 3, 0, 8193, 4, 2, 0, ok, ok), (1, ptrs, wh, None, 3, 0, 4, 0, 2, 0, ok, ok),
                 (1, ptrs, wh, None, 3, 0, 4, 4, 4, 0, ok, ok), (1, ptrs, wh, None, 3, 0, 4, 4, 2, 2, ok, ok),
                 (0, ptrs, wh, None, 3, 0, 4, 4, 2, 0, ok, ok), (1, None, wh, None, 3, 0, 4, 4, 2, 0, ok, ok),
                 (1, ptrs, (C.c_uint * 2)(0, 8), None, 3, 0, 4, 4, 2, 0, ok, ok),
                 (1, ptrs, wh, (C.c_uint * 1)(7), 3, 0, 4, 4, 2, 0, ok, ok)]:
        assert L.zj_resize_device(h, *args, None, p, None) == -1, args
    assert L.zj_resize_device(h, 1, ptrs, wh, None, 3, 0, 4, 4, 2, 0, ok, ok, None, None, None) == -1


# ---- crops resized: the model of zj_decode_crops_device's own crop -----------------------------------------------------
def frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed, index=0):
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=seed, frame_index=index)
    cs, layout = KINDS[kind] if kind in KINDS else (5, 0)
    d = zj.FrameDesc.make(W, H, hs, vs, 3, cs, qts)
    d.flags, d.out_layout = flags, layout
    dev = [torch.from_numpy(np.ascontiguousarray(p, np.int16)).cuda() for p in planes]
    torch.cuda.synchronize()
    return d, dev


def own_crop(zj, ctx, torch, d, frame, x, y, w, h):
    """zj_decode_crops_device's crop of one window, as [C, h, w] uint8"""
    ln = zj.crop_out_len(d, w, h)
    buf = torch.full((ln,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_crops_device(d, [frame[0].data_ptr()], [frame[1].data_ptr()], [frame[2].data_ptr()], [(x, y)], w, h,
                            [buf.data_ptr()])
    ctx.sync()
    a = buf.cpu().numpy()
    c = channels_of(zj, d)
    if c == 1:
        return a.reshape(1, h, w)
    return a.reshape(3, h, w) if is_chw(zj, d) else a.reshape(h, w, 3).transpose(2, 0, 1)


def full_image(zj, ctx, torch, d, frame):
    """the full device decode of one frame, as [C, H, W] uint8"""
    n = zj.lib().zj_out_len(C.byref(d))
    buf = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_planes_device(d, 1, frame[0].data_ptr(), frame[1].data_ptr(), frame[2].data_ptr(), buf.data_ptr())
    ctx.sync()
    a = buf.cpu().numpy()
    c, W, H = channels_of(zj, d), d.width, d.height
    if c == 1:
        return a.reshape(1, H, W)
    return a.reshape(3, H, W) if is_chw(zj, d) else a.reshape(H, W, c).transpose(2, 0, 1)


def run_resized(zj, ctx, torch, d, frames, windows, ow, oh, dtype, layout, scale, bias, flips, stream=None):
    c = channels_of(zj, d)
    per = zj.resized_out_len(d, ow, oh, dtype)
    assert per == c * ow * oh * ESZ[dtype]
    buf = out_buffer(torch, len(frames) * per)
    ctx.decode_crops_resized_device(d, [f[0].data_ptr() for f in frames], [f[1].data_ptr() for f in frames],
                                    [f[2].data_ptr() for f in frames], windows, ow, oh, dtype,
                                    zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW, buf.data_ptr() + GUARD, scale,
                                    bias, flips, stream)
    if stream is None:
        ctx.sync()
    else:
        torch.cuda.synchronize()
    out = read_out(buf, len(frames) * per)
    return [out[i * per:(i + 1) * per] for i in range(len(frames))]


def windows_of(rng, W, H, n):
    """different sizes in one batch: the whole frame, the corners (frame edges, the last strip), random ones"""
    out = [(0, 0, W, H), (W - 1, H - 1, 1, 1), (0, H - 17, min(W, 50), 17), (W - 33, 0, 33, min(H, 70))]
    while len(out) < n:
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        out.append((int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1)), w, h))
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("flags", [0, 7])
def test_crops_resized_equal_the_model_of_the_crop(zj, ctx, torch, synth, mode, kind, flags):
    hs, vs = MODES[mode]
    rng = np.random.default_rng(zlib.crc32(f"{mode}-{kind}-{flags}".encode()))
    W, H = (1040, 136) if flags else (520, 203)
    d, dev = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed=W + hs)
    c = channels_of(zj, d)
    wins = windows_of(rng, W, H, 12)
    flips = [bool(i % 3 == 1) for i in range(len(wins))]
    crops = [own_crop(zj, ctx, torch, d, dev, *w) for w in wins]
    img = full_image(zj, ctx, torch, d, dev)
    dtype = int(rng.integers(4))
    layout = "NHWC" if rng.integers(2) else "NCHW"
    scale, bias = random_factors(rng, c)
    for (ow, oh) in [(64, 48), (7, 300)]:
        outs = run_resized(zj, ctx, torch, d, [dev] * len(wins), wins, ow, oh, dtype, layout, scale, bias, flips)
        for i, w in enumerate(wins):
            what = f"{kind} {mode} flags {flags} window {w} -> {ow}x{oh} dtype {dtype} {layout}"
            exp = rm.resize(crops[i], ow, oh, dtype, scale, bias, flips[i], layout)
            check_image(outs[i], exp, dtype, what)
            # (and of the full decode's window: a wrong crop would make a wrong expectation above)
            x, y, ww, hh = w
            exp = rm.resize(img[:, y:y + hh, x:x + ww], ow, oh, dtype, scale, bias, flips[i], layout)
            check_image(outs[i], exp, dtype, what + " (full decode's window)")


def tail_geometry(W, hs):
    """(p', position) of an RGB row of width W (zj_device.h: store_unit_generic)"""
    P = -(-W // (8 * hs)) * 8 * hs
    position = 48 * max(P // 16 - 1, 0)
    diff = max(64 - (3 * W - position), 0)
    return (position - diff if position > diff else 0), position


def tail_windows(W, H, hs, rng):
    """windows at a row's end: the whole frame, right-aligned ones, ones that start or end at the pixels of bytes p' - 1,
    p', p' + 48, position and 3W - 1, random ones"""
    pp, position = tail_geometry(W, hs)
    out = [(0, 0, W, H)] + [(W - w, int(rng.integers(H - 7)), w, 7) for w in (1, 2, 5, 8, 16, 17, 31, 48) if w <= W]
    for b in (pp - 1, pp, pp + 48, position, 3 * W - 1):
        q = min(max(b // 3, 0), W - 1)
        out += [(q, 0, W - q, H), (0, 3, q + 1, H - 3), (q, 1, min(W - q, 20), 9), (max(q - 19, 0), 2, min(q + 1, 20), 11)]
    while len(out) < 40:
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        out.append((int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1)), w, h))
    return out


@pytest.mark.parametrize("W", [256, 257, 258, 261, 262, 513, 517, 1029, 1281, 2053, 4101])
@pytest.mark.parametrize("mode", ["h", "hv"])
def test_tail_width_resized_crops_equal_the_model_of_the_full_decode(zj, ctx, torch, synth, W, mode):
    """4:2:2 / 4:2:0 widths W = 1..5 mod 256 (the early RGB tail starts on a column boundary) and neighbours: the resized
    crops == the model of the full device decode's window (not of the crop, which would share a wrong crop's bytes)"""
    hs, vs = MODES[mode]
    H = 64
    rng = np.random.default_rng(W * hs * vs)
    for kind in ("rgb", "chw"):
        for flags in (0, 6, 7):
            d, dev = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed=W)
            img = full_image(zj, ctx, torch, d, dev)
            wins = tail_windows(W, H, hs, rng)
            flips = [bool(i % 3 == 1) for i in range(len(wins))]
            dtype = (flags + hs) % 4
            layout = "NHWC" if flags % 2 else "NCHW"
            scale, bias = random_factors(rng, 3)
            for (ow, oh) in [(32, 24), (5, 70)]:
                outs = run_resized(zj, ctx, torch, d, [dev] * len(wins), wins, ow, oh, dtype, layout, scale, bias, flips)
                for i, (x, y, w, h) in enumerate(wins):
                    exp = rm.resize(img[:, y:y + h, x:x + w], ow, oh, dtype, scale, bias, flips[i], layout)
                    check_image(outs[i], exp, dtype, f"{kind} {W} {mode} flags {flags} window {(x, y, w, h)} -> {ow}x{oh}")


def test_crops_resized_scattered_frames_and_every_dtype(zj, ctx, torch, synth):
    rng = np.random.default_rng(77)
    W, H = 800, 96
    frames, descs = [], []
    for i in range(40):  # (above ZJ_SCATTER_MAX: two crop launches)
        d, dev = frame_on_device(zj, torch, synth, W, H, 2, 2, "rgb", 0, seed=5, index=i)
        frames.append(dev)
    wins = windows_of(rng, W, H, 40)
    flips = [bool(rng.integers(2)) for _ in wins]
    crops = [own_crop(zj, ctx, torch, d, frames[i], *w) for i, w in enumerate(wins)]
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    scale = np.float32(1 / (255 * np.array(std)))
    bias = np.float32(-np.array(mean) / np.array(std))
    for dtype in range(4):
        for layout in ("NCHW", "NHWC"):
            outs = run_resized(zj, ctx, torch, d, frames, wins, 224, 224, dtype, layout, scale, bias, flips)
            for i in range(len(wins)):
                check_image(outs[i], rm.resize(crops[i], 224, 224, dtype, scale, bias, flips[i], layout), dtype, f"frame {i}")


def test_crops_resized_split_past_the_scratch_cap(zj, ctx, torch, synth):
    """six 4096 x 4096 RGB windows are 302 MB of crops: more than one launch group (256 MB) -- the buffer is reused"""
    d, dev = frame_on_device(zj, torch, synth, 4096, 4096, 2, 2, "rgb", 0, seed=4)
    wins = [(0, 0, 4096, 4096)] * 5 + [(1, 3, 4095, 4093)]
    flips = [False, True, False, True, False, True]
    crop = own_crop(zj, ctx, torch, d, dev, 0, 0, 4096, 4096)
    crop2 = own_crop(zj, ctx, torch, d, dev, 1, 3, 4095, 4093)
    outs = run_resized(zj, ctx, torch, d, [dev] * 6, wins, 96, 80, rm.BF16, "NCHW", [0.01] * 3, [-1.0] * 3, flips)
    for i in range(6):
        exp = rm.resize(crop2 if i == 5 else crop, 96, 80, rm.BF16, [0.01] * 3, [-1.0] * 3, flips[i])
        check_image(outs[i], exp, rm.BF16, f"window {i}")


def test_crops_resized_reject_bad_arguments(zj, ctx, torch, synth):
    d, dev = frame_on_device(zj, torch, synth, 256, 128, 2, 2, "rgb", 0, seed=1)
    buf = out_buffer(torch, 1 << 16)
    o = buf.data_ptr() + GUARD

    def call(desc, wins, ow=16, oh=16, dtype=2, layout=0, scale=None):
        try:
            ctx.decode_crops_resized_device(desc, [dev[0].data_ptr()] * len(wins), [dev[1].data_ptr()] * len(wins),
                                            [dev[2].data_ptr()] * len(wins), wins, ow, oh, dtype, layout, o, scale)
            return 0
        except zj.ZjError as e:
            return e.status

    assert call(d, [(0, 0, 256, 128)]) == 0
    ctx.sync()
    for wins, kw in [([(1, 0, 256, 128)], {}), ([(0, 0, 0, 5)], {}), ([(0, 120, 16, 9)], {}), ([(0, 0, 8, 8)], {"ow": 8193}),
                     ([(0, 0, 8, 8)], {"dtype": 7}), ([(0, 0, 8, 8)], {"layout": 3}),
                     ([(0, 0, 8, 8)], {"scale": [1.0, float("nan"), 1.0]})]:
        assert call(d, wins, **kw) != 0, (wins, kw)
    rgba, dev2 = frame_on_device(zj, torch, synth, 256, 128, 2, 2, "rgba", 0, seed=1)
    assert zj.resized_out_len(rgba, 16, 16, 2) == 0
    assert call(rgba, [(0, 0, 8, 8)]) != 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[GUARD + 3 * 16 * 16 * 2:] == 0xAA).all()


def test_crops_resized_follow_the_callers_stream(zj, ctx, torch, synth):
    """two calls on two streams of the caller, back to back: the second's crops must not overwrite the buffer while the
    first's resize still reads it (the buffer's reuse is ordered on the caller's streams)"""
    d, dev = frame_on_device(zj, torch, synth, 2048, 1024, 2, 2, "rgb", 0, seed=8)
    rng = np.random.default_rng(8)
    wa, wb = windows_of(rng, 2048, 1024, 24), windows_of(rng, 2048, 1024, 24)[::-1]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    per = zj.resized_out_len(d, 224, 224, rm.F32)
    outs = []
    for s, wins in ((s1, wa), (s2, wb)):
        buf = out_buffer(torch, len(wins) * per)
        ctx.decode_crops_resized_device(d, [dev[0].data_ptr()] * 24, [dev[1].data_ptr()] * 24, [dev[2].data_ptr()] * 24,
                                        wins, 224, 224, rm.F32, 0, buf.data_ptr() + GUARD, None, None, None, s.cuda_stream)
        outs.append((buf, wins))
    torch.cuda.synchronize()
    for buf, wins in outs:
        out = read_out(buf, len(wins) * per)
        for i, w in enumerate(wins[:8]):
            exp = rm.resize(own_crop(zj, ctx, torch, d, dev, *w), 224, 224, rm.F32)
            check_image(out[i * per:(i + 1) * per], exp, rm.F32, f"window {w}")


# ---- the file path ------------------------------------------------------------------------------------------------------
def _files():
    g = os.path.join(HERE, "golden")
    return [os.path.join(g, "test-baseline.jpg")] + sorted(glob.glob(os.path.join(g, "ref", "*.jp*g")))


@pytest.mark.parametrize("entropy", ["cpu", "gpu"])
def test_file_path_equals_the_planes_path(zj, torch, entropy):
    """zj_decoder_finish_pixels_resized_crop_device == the model of the full decode's window (== the crop of the planes
    path), on a context whose scratch holds another file's planes before every call"""
    rng = np.random.default_rng(zlib.crc32(entropy.encode()))
    g = os.path.join(HERE, "golden", "ref")
    poisons = [os.path.join(g, "speed_bench.jpg"), os.path.join(g, "medium_no_samp_2500x1786.jpg")]
    ref_ctx, crop_ctx = zj.Context(zj.BACKEND_HIP, 0), zj.Context(zj.BACKEND_HIP, 0)

    def opts():
        o = zj.ZuneJpegOptions()
        if entropy == "gpu":
            o.entropy = zj.ENTROPY_GPU_ALWAYS
        return o

    def poison_scratch(path):
        src = poisons[1] if os.path.basename(path) == os.path.basename(poisons[0]) else poisons[0]
        pd = zj.Decoder(zj.ZuneJpegOptions(), crop_ctx)
        desc, _ = pd.prepare(open(src, "rb").read())
        n = zj.lib().zj_out_len(C.byref(desc))
        b = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert pd.finish_pixels_device(b.data_ptr(), n) == n
        pd.close()

    checked = 0
    try:
        for path in _files():
            data = open(path, "rb").read()
            ref_dec = zj.Decoder(opts(), ref_ctx)
            try:
                desc, _ = ref_dec.prepare(data)
            except zj.ZjError:
                ref_dec.close()
                continue
            n = zj.lib().zj_out_len(C.byref(desc))
            full = torch.empty(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert ref_dec.finish_pixels_device(full.data_ptr(), n) == n
            ref_dec.close()
            W, H = desc.width, desc.height
            c = n // (W * H)
            img = full.cpu().numpy().reshape(H, W, c).transpose(2, 0, 1)
            dec = zj.Decoder(opts(), crop_ctx)
            for k, (x, y, w, h) in enumerate(windows_of(rng, W, H, 6)[:3] + windows_of(rng, W, H, 6)[4:]):
                dtype = k % 4
                layout = "NHWC" if k % 2 else "NCHW"
                ow, oh = (224, 224) if k % 2 else (97, 61)
                scale, bias = random_factors(rng, c)
                poison_scratch(path)
                dec.prepare(data)
                per = zj.resized_out_len(desc, ow, oh, dtype)
                buf = out_buffer(torch, per)
                got = dec.finish_pixels_resized_crop_device(x, y, w, h, ow, oh, dtype,
                                                            zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW,
                                                            buf.data_ptr() + GUARD, per, scale, bias, flip=bool(k % 3))
                assert got == per
                out = read_out(buf, per)
                exp = rm.resize(img[:, y:y + h, x:x + w], ow, oh, dtype, scale, bias, bool(k % 3), layout)
                check_image(out, exp, dtype, f"{os.path.basename(path)} {entropy} window {(x, y, w, h)}")
                checked += 1
            dec.close()
    finally:
        ref_ctx.close()
        crop_ctx.close()
    assert checked >= 10


@pytest.mark.parametrize("entropy", ["cpu", "gpu"])
def test_file_path_at_a_tail_width(zj, torch, synth, entropy):
    """a 4:2:0 baseline file 517 pixels wide (tools/jpeg_enc.py; its RGB rows end 1 byte past `position`, the tail on a
    column boundary): finish_pixels_crop_device == finish_pixels_device sliced, and finish_pixels_resized_crop_device ==
    the model of that slice"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import jpeg_enc
    W, H = 517, 100
    data = jpeg_enc.encode_baseline(jpeg_enc.small_planes(W, H, 2, 2, 3, seed=5), synth.quant_tables(85), W, H, 2, 2, 3)
    rng = np.random.default_rng(zlib.crc32(entropy.encode()))
    ctx = zj.Context(zj.BACKEND_HIP, 0)

    def opts():
        o = zj.ZuneJpegOptions()
        if entropy == "gpu":
            o.entropy = zj.ENTROPY_GPU_ALWAYS
        return o
    try:
        dec = zj.Decoder(opts(), ctx)
        desc, _ = dec.prepare(data)
        assert (desc.width, desc.height, desc.h_max, desc.v_max) == (W, H, 2, 2)
        n = zj.lib().zj_out_len(C.byref(desc))
        full = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert dec.finish_pixels_device(full.data_ptr(), n) == n
        ref = full.cpu().numpy().reshape(H, W * 3)
        img = ref.reshape(H, W, 3).transpose(2, 0, 1)
        for k, (x, y, w, h) in enumerate(tail_windows(W, H, 2, rng)):
            dec.prepare(data)
            ln = zj.crop_out_len(desc, w, h)
            buf = out_buffer(torch, ln)
            assert dec.finish_pixels_crop_device(x, y, w, h, buf.data_ptr() + GUARD, ln) == ln
            got = read_out(buf, ln)
            assert np.array_equal(got, ref[y:y + h, 3 * x:3 * (x + w)].reshape(-1)), (entropy, x, y, w, h)
            dtype, layout = k % 4, ("NHWC" if k % 2 else "NCHW")
            ow, oh = (224, 224) if k % 5 == 0 else (31, 17)
            scale, bias = random_factors(rng, 3)
            dec.prepare(data)
            per = zj.resized_out_len(desc, ow, oh, dtype)
            buf = out_buffer(torch, per)
            assert dec.finish_pixels_resized_crop_device(x, y, w, h, ow, oh, dtype,
                                                         zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW,
                                                         buf.data_ptr() + GUARD, per, scale, bias, flip=bool(k % 3)) == per
            exp = rm.resize(img[:, y:y + h, x:x + w], ow, oh, dtype, scale, bias, bool(k % 3), layout)
            check_image(read_out(buf, per), exp, dtype, f"{entropy} window {(x, y, w, h)} -> {ow}x{oh}")
        dec.close()
    finally:
        ctx.close()


# ---- tensors --------------------------------------------------------------------------------------------------------------
def test_decode_resized_crops_to_tensor(zj, ctx, torch, synth):
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    for kind in ("rgb", "chw", "gray"):
        d, dev = frame_on_device(zj, torch, synth, 640, 480, 2, 2, kind, 0, seed=9)
        c = channels_of(zj, d)
        m, sd = (mean, std) if c == 3 else ([0.5], [0.25])
        wins = [(0, 0, 224, 224), (416, 256, 224, 224), (100, 37, 224, 224), (3, 5, 300, 200)]
        s = torch.cuda.Stream()
        for layout in ("NCHW", "NHWC"):
            out = tensors.decode_resized_crops_to_tensor(ctx, d, [dev] * 4, wins, (224, 224), layout=layout, mean=m, std=sd,
                                                         flips=[False, False, True, False], stream=s)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            shape = (4, c, 224, 224) if layout == "NCHW" else (4, 224, 224, c)
            assert tuple(out.shape) == shape and out.dtype == torch.bfloat16 and out.is_cuda and out.is_contiguous()
            nchw = out if layout == "NCHW" else out.permute(0, 3, 1, 2)
            for i, (x, y, w, h) in enumerate(wins[:3]):
                crop = torch.from_numpy(own_crop(zj, ctx, torch, d, dev, x, y, w, h)).float()
                if i == 2:
                    crop = crop.flip(-1)
                exp = (crop / 255 - torch.tensor(m)[:, None, None]) / torch.tensor(sd)[:, None, None]
                got = nchw[i].float().cpu()
                ulp = (exp.abs() * 2 ** -7).clamp(min=1e-5)  # one bf16 ulp (an upper bound of it)
                assert ((got - exp).abs() <= ulp).all(), (kind, layout, i)
            crop = own_crop(zj, ctx, torch, d, dev, *wins[3])
            sc, bi = tensors.normalize_factors(c, m, sd)
            check_image(nchw[3].contiguous().view(torch.int16).cpu().numpy().view(np.uint8).reshape(-1),
                        rm.resize(crop, 224, 224, rm.BF16, sc, bi), rm.BF16, kind)
        f32 = tensors.decode_resized_crops_to_tensor(ctx, d, [dev], [(0, 0, 640, 480)], (128, 96), dtype=torch.float32)
        torch.cuda.synchronize()
        assert tuple(f32.shape) == (1, c, 96, 128) and f32.dtype == torch.float32
        u8 = tensors.decode_resized_crops_to_tensor(ctx, d, [dev], [(0, 0, 640, 480)], (128, 96), dtype=torch.uint8)
        torch.cuda.synchronize()
        assert u8.dtype == torch.uint8


def test_resize_to_tensor(zj, ctx, torch):
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (w, h) in [(300, 200), (17, 401), (224, 224)]]
    dev = [torch.from_numpy(a).cuda() for a in imgs]
    dev[1] = torch.zeros((401, 40, 3), dtype=torch.uint8, device="cuda")[:, 5:22]  # rows at a pitch
    dev[1].copy_(torch.from_numpy(imgs[1]).cuda())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    out = tensors.resize_to_tensor(ctx, dev, (160, 120), dtype=torch.float16, flips=[True, False, False], stream=s)
    s.synchronize()
    assert tuple(out.shape) == (3, 3, 120, 160) and out.dtype == torch.float16
    sc, bi = tensors.normalize_factors(3)
    for i, a in enumerate(imgs):
        exp = rm.resize(a.transpose(2, 0, 1), 160, 120, rm.F16, sc, bi, i == 0)
        assert np.array_equal(out[i].cpu().numpy().view(np.uint16), exp), i
    chw = [torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).cuda() for a in imgs]
    torch.cuda.synchronize()
    o2 = tensors.resize_to_tensor(ctx, chw, (160, 120), dtype=torch.float16, in_layout="CHW", flips=[True, False, False])
    torch.cuda.synchronize()
    assert torch.equal(o2, out)
