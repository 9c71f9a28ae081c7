"""GPU: crop-window decode (zj_decode_crops_device, zj_decoder_finish_pixels_crop_device, tensors.decode_crops_to_tensor)
on an MI355X.  A crop must be exactly the bytes of the same library's full device decode inside the window; guard bytes
around every output and the pitch padding stay untouched."""
import ctypes as C
import glob
import importlib
import os
import sys
import zlib

import numpy as np
import pytest

import oracle_c as oc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {"none": (1, 1), "h": (2, 1), "v": (1, 2), "hv": (2, 2)}
KINDS = {"rgb": (0, 0), "gray": (1, 0), "ycbcr": (2, 0), "rgba": (5, 0), "chw": (0, 1)}
GUARD = 256


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


def bpp_of(zj, d):
    ncomp = zj.num_components(d.out_colorspace)
    return 1 if (d.out_layout == 1 and ncomp == 3) else ncomp


def full_device(zj, ctx, torch, d, planes):
    """the full device decode of one frame: [H, row] (HWC) or [3, H, W] (CHW), on the host"""
    out_len = zj.lib().zj_out_len(C.byref(d))
    out = torch.full((out_len,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the library writes on its own stream: torch's fill must be done before)
    ctx.decode_planes_device(d, 1, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), out.data_ptr())
    ctx.sync()
    a = out.cpu().numpy()
    return a.reshape(3, d.height, d.width) if bpp_of(zj, d) == 1 and zj.num_components(d.out_colorspace) == 3 else a.reshape(d.height, -1)


def run_crops(zj, ctx, torch, d, frames, origins, w, h, out_pitch=0):
    """every crop in one buffer with GUARD poisoned bytes around each; returns the crops (host) after checking the guards"""
    ln = zj.crop_out_len(d, w, h, out_pitch)
    assert ln > 0
    slot = ln + 2 * GUARD
    buf = torch.full((len(frames) * slot + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    base = buf.data_ptr()
    ctx.decode_crops_device(d, [f[0].data_ptr() for f in frames], [f[1].data_ptr() for f in frames],
                            [f[2].data_ptr() for f in frames], origins, w, h,
                            [base + i * slot + GUARD + (i % 3) for i in range(len(frames))], out_pitch)
    ctx.sync()
    a = buf.cpu().numpy()
    outs = []
    for i in range(len(frames)):
        o = i * slot + GUARD + (i % 3)
        assert (a[o - GUARD:o] == 0xAA).all() and (a[o + ln:o + ln + GUARD - 3] == 0xAA).all(), f"crop {i} wrote outside its bytes"
        outs.append(a[o:o + ln])
    return outs


def check(zj, d, full, crops, origins, w, h, out_pitch=0):
    b = bpp_of(zj, d)
    chw = b == 1 and zj.num_components(d.out_colorspace) == 3
    pitch = out_pitch or w * b
    for i, ((x, y), got) in enumerate(zip(origins, crops)):
        rows = got.reshape(3, h, pitch) if chw else got.reshape(h, pitch)
        exp = full[:, y:y + h, x:x + w] if chw else full[y:y + h, x * b:(x + w) * b]
        if not np.array_equal(rows[..., :w * b], exp):
            raise AssertionError(f"crop {i} {w}x{h} at ({x},{y}) of {d.width}x{d.height}: {(rows[..., :w * b] != exp).sum()} bytes differ")
        assert (rows[..., w * b:] == 0xAA).all(), "pitch padding written"


def frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed, index=0):
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=seed, frame_index=index)
    cs, layout = KINDS[kind]
    d = zj.FrameDesc.make(W, H, hs, vs, 3, cs, qts)
    d.flags, d.out_layout = flags, layout
    dev = [torch.from_numpy(np.ascontiguousarray(p, np.int16)).cuda() for p in planes]
    torch.cuda.synchronize()  # (the uploads are torch's, the reads the library's stream)
    return d, dev, planes, qts


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_random_windows_equal_sliced_full_decode(zj, ctx, torch, synth, mode, kind):
    hs, vs = MODES[mode]
    rng = np.random.default_rng(zlib.crc32(f"{mode}-{kind}".encode()))
    for (W, H, flags) in [(2500, 120, 0), (1040, 72, 7), (13, 9, 0), (4096, 64, 7)]:
        d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed=W)
        try:
            full = full_device(zj, ctx, torch, d, dev)
        except zj.ZjError:  # (a reference panic, ZJ_ERR_PANIC: the crop refuses the frame as well)
            assert zj.crop_out_len(d, 1, 1) == 0
            continue
        if kind in ("rgb", "gray", "ycbcr") and flags == 0:
            f = oc.make_frame(W, H, hs, vs, 3, KINDS[kind][0], qts)
            rc, exp = oc.decode_planes(f, planes)
            if rc == 0:
                assert np.array_equal(full.reshape(-1), exp), "full device decode != oracle"
            else:
                continue
        for _ in range(4):  # 4 sizes x 50 windows
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for _ in range(50)]
            pitch = 0 if rng.integers(2) else (w * bpp_of(zj, d) + int(rng.integers(1, 200)))
            crops = run_crops(zj, ctx, torch, d, [dev] * 50, origins, w, h, pitch)
            check(zj, d, full, crops, origins, w, h, pitch)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 100])
def test_scattered_batches_each_frame_its_origin(zj, ctx, torch, synth, n):
    W, H = 2500, 72
    rng = np.random.default_rng(n)
    frames, fulls = [], []
    for i in range(n):
        d, dev, _, _ = frame_on_device(zj, torch, synth, W, H, 2, 2, "rgb", 0, seed=21, index=i)
        frames.append(dev)
        if i < 40 or i % 7 == 0:
            fulls.append((i, full_device(zj, ctx, torch, d, dev)))
    w, h = 224, 40
    origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for _ in range(n)]
    crops = run_crops(zj, ctx, torch, d, frames, origins, w, h)
    for i, full in fulls:
        check(zj, d, full, [crops[i]], [origins[i]], w, h)


def test_whole_frame_window_4096(zj, ctx, torch, synth):
    d, dev, _, _ = frame_on_device(zj, torch, synth, 4096, 4096, 2, 2, "rgb", 0, seed=4)
    full = full_device(zj, ctx, torch, d, dev)
    crops = run_crops(zj, ctx, torch, d, [dev], [(0, 0)], 4096, 4096)
    assert np.array_equal(crops[0], full.reshape(-1))


ROOT = os.path.dirname(HERE)


def _files():
    g = os.path.join(HERE, "golden")
    return [os.path.join(g, "test-baseline.jpg"), os.path.join(g, "test-progressive.jpg")] + \
        sorted(glob.glob(os.path.join(g, "ref", "*.jp*g")))


def _gray_file(synth):
    """a single-component baseline file (tools/jpeg_enc.py): the decoder's GRAYSCALE output whatever colour is asked for"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import jpeg_enc
    w, h = 200, 136
    planes = jpeg_enc.small_planes(w, h, 1, 1, 1, seed=17)
    return jpeg_enc.encode_baseline(planes, synth.quant_tables(85), w, h, 1, 1, 1)


def _windows(rng, W, H):
    """the whole frame, then windows whose rows start and end away from the first and the last strip (32 rows at most),
    so that an upload of the wrong strips, at the wrong offset or of the wrong length shows; then a random one"""
    out = [(0, 0, W, H)]
    if H >= 4 * 32:
        y0 = int(rng.integers(32, H - 2 * 32))
        h = int(rng.integers(1, H - 32 - y0 + 1))
        w = int(rng.integers(1, W + 1))
        out.append((int(rng.integers(W - w + 1)), y0, w, h))
        out.append((0, H // 2, W, min(H - H // 2 - 1, 40) or 1))
    w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
    out.append((int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1)), w, h))
    return out


@pytest.mark.parametrize("entropy", ["cpu", "gpu"])
def test_file_path_crops(zj, torch, synth, entropy):
    """zj_decoder_finish_pixels_crop_device == the full finish_pixels_device, sliced.  The crops run on a context of their
    own whose scratch planes hold ANOTHER, larger file's planes before every crop (a full decode of it on that context), so
    that with CPU entropy only the strips the crop uploads itself can be right: a strip left out, put at the wrong offset or
    cut short shows as wrong pixels."""
    rng = np.random.default_rng(zlib.crc32(entropy.encode()))
    g = os.path.join(HERE, "golden", "ref")
    poisons = [os.path.join(g, "speed_bench.jpg"), os.path.join(g, "large_vertical_samp_7680_4320.jpg")]
    files = [(os.path.basename(p), open(p, "rb").read()) for p in _files()] + [("gray (jpeg_enc)", _gray_file(synth))]
    ref_ctx, crop_ctx = zj.Context(zj.BACKEND_HIP, 0), zj.Context(zj.BACKEND_HIP, 0)

    def opts(colour=None):
        o = zj.ZuneJpegOptions()
        if entropy == "gpu":
            o.entropy = zj.ENTROPY_GPU_ALWAYS
        if colour is not None:
            o.out_colorspace = colour
        return o

    def poison_scratch(name):
        src = poisons[1] if name == os.path.basename(poisons[0]) else poisons[0]
        pd = zj.Decoder(zj.ZuneJpegOptions(), crop_ctx)  # (CPU entropy: its planes go to the context's scratch)
        desc, _ = pd.prepare(open(src, "rb").read())
        n = zj.lib().zj_out_len(C.byref(desc))
        buf = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert pd.finish_pixels_device(buf.data_ptr(), n) == n
        pd.close()

    checked = 0
    try:
        for name, data in files:
            colour = zj.ColorSpace.RGBA if name.startswith("gray") else None
            ref_dec = zj.Decoder(opts(colour), ref_ctx)
            try:
                desc, _ = ref_dec.prepare(data)
            except zj.ZjError:
                ref_dec.close()
                continue  # (a file the decoder refuses on the full path too)
            n = zj.lib().zj_out_len(C.byref(desc))
            full = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert ref_dec.finish_pixels_device(full.data_ptr(), n) == n
            ref_dec.close()
            ref = full.cpu().numpy()
            W, H = desc.width, desc.height
            b = n // (W * H)
            if name.startswith("gray"):
                assert desc.in_components == 1 and desc.out_colorspace == int(zj.ColorSpace.GRAYSCALE) and b == 1
            dec = zj.Decoder(opts(colour), crop_ctx)
            for (x, y, w, h) in _windows(rng, W, H):
                poison_scratch(name)
                dec.prepare(data)
                ln = zj.crop_out_len(desc, w, h)
                out = torch.full((ln + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                assert dec.finish_pixels_crop_device(x, y, w, h, out.data_ptr() + GUARD, ln) == ln
                a = out.cpu().numpy()
                assert (a[:GUARD] == 0xAA).all() and (a[GUARD + ln:] == 0xAA).all()
                if b == 3 and desc.out_layout == 1:
                    exp = ref.reshape(3, H, W)[:, y:y + h, x:x + w].reshape(-1)
                else:
                    exp = ref.reshape(H, W * b)[y:y + h, x * b:(x + w) * b].reshape(-1)
                assert np.array_equal(a[GUARD:GUARD + ln], exp), (name, entropy, x, y, w, h)
                checked += 1
            dec.close()
    finally:
        ref_ctx.close()
        crop_ctx.close()
    assert checked >= len(files)


def test_decode_crops_to_tensor(zj, ctx, torch, synth):
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    for kind in ("rgb", "chw", "gray"):
        d, dev, _, _ = frame_on_device(zj, torch, synth, 640, 480, 2, 2, kind, 0, seed=9)
        storage, view = tensors.output_tensor(d, 1, "cuda")
        ctx.decode_planes_device(d, 1, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), storage.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        origins = [(0, 0), (416, 256), (100, 37)]
        s = torch.cuda.Stream()
        out = tensors.decode_crops_to_tensor(ctx, d, [dev] * 3, origins, (224, 224), stream=s)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        shape = {"rgb": (3, 224, 224, 3), "chw": (3, 3, 224, 224), "gray": (3, 224, 224)}[kind]
        assert tuple(out.shape) == shape and out.is_contiguous() and out.dtype == torch.uint8
        for i, (x, y) in enumerate(origins):
            if kind == "rgb":
                exp = view[0, y:y + 224, x:x + 224]
            else:
                exp = view[0, ..., y:y + 224, x:x + 224]
            assert torch.equal(out[i], exp), (kind, i)


# ---- the row ends where the early RGB tail starts on a column boundary --------------------------------------------------
# 4:2:2 / 4:2:0 widths W = 1..5 mod 256, W > 256: the bytes [p' + 48, position) of every RGB row are the previous column's
# (zj_plan.h: make_crop_plan's hole).  256 and 262 are unaffected neighbours.
TAIL_WIDTHS = [256, 257, 258, 261, 262, 513, 517, 1029, 1281, 2053, 4101]


def tail_geometry(W, hs):
    """(p', position) of an RGB row of width W (zj_device.h: store_unit_generic)"""
    P = -(-W // (8 * hs)) * 8 * hs
    position = 48 * max(P // 16 - 1, 0)
    diff = max(64 - (3 * W - position), 0)
    return (position - diff if position > diff else 0), position


def tail_windows(W, H, hs):
    """(w, h, origins) launches of many windows each: the whole frame; every right-aligned width 1..48; windows that start
    or end at the pixels of bytes p' - 1, p', p' + 48, position and 3W - 1"""
    pp, position = tail_geometry(W, hs)
    h = 8
    rows = list(range(H - h + 1))[:64]
    wins = [(W, H, [(0, 0)])]
    wins += [(w, h, [(W - w, y) for y in rows]) for w in range(1, min(W, 48) + 1)]
    for b in (pp - 1, pp, pp + 48, position, 3 * W - 1):
        q = min(max(b // 3, 0), W - 1)
        wins += [(W - q, h, [(q, y) for y in rows]), (q + 1, h, [(0, y) for y in rows]),
                 (min(W - q, 20), h, [(q, y) for y in rows]), (min(q + 1, 20), h, [(max(q - 19, 0), y) for y in rows])]
    return wins


@pytest.mark.parametrize("W", TAIL_WIDTHS)
@pytest.mark.parametrize("mode", ["h", "hv"])
def test_tail_width_crops_equal_sliced_full_decode(zj, ctx, torch, synth, W, mode):
    """crops at the tail widths == the sliced full device decode, byte for byte.  Before every launch the same kernel crops
    another frame whole, so that staging a workgroup reads without having written holds that frame's bytes, not these."""
    hs, vs = MODES[mode]
    H = 64
    for kind in ("rgb", "rgba", "chw"):
        for flags in (0, 6, 7):
            d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed=W)
            _, other, _, _ = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed=W + 1, index=1)
            full = full_device(zj, ctx, torch, d, dev)
            if kind == "rgb" and flags == 0:
                rc, exp = oc.decode_planes(oc.make_frame(W, H, hs, vs, 3, oc.RGB, qts), planes)
                assert rc == 0 and np.array_equal(full.reshape(-1), exp), "full device decode != oracle"
            scratch = torch.empty(zj.crop_out_len(d, W, H), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            for (w, h, origins) in tail_windows(W, H, hs):
                ctx.decode_crops_device(d, [other[0].data_ptr()], [other[1].data_ptr()], [other[2].data_ptr()], [(0, 0)], W, H,
                                        [scratch.data_ptr()])  # (the context's stream: before the launch below)
                crops = run_crops(zj, ctx, torch, d, [dev] * len(origins), origins, w, h)
                try:
                    check(zj, d, full, crops, origins, w, h)
                except AssertionError as e:
                    raise AssertionError(f"{kind} {mode} flags {flags}: {e}") from None
