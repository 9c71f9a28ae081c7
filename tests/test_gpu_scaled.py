"""GPU: the reduced-size decode (zj_decode_crops_scaled_device, zj_decode_crops_resized_prescaled_device,
tensors.decode_scaled_to_tensor) on an MI355X.  A reduced crop must be, bit for bit, the numpy definition
(tests/scaled_model.py); a prescaled resized crop the resize models (tests/resize_model.py, tests/resize_aa_model.py) applied
to the definition's reduced crop at the reduced window; guard bytes around every output and the pitch padding stay
untouched."""
import ctypes as C
import glob
import importlib
import os
import zlib

import numpy as np
import pytest

import resize_aa_model as am
import resize_model as rm
import scaled_model as sm

pytestmark = pytest.mark.gpu
MODES = {"none": (1, 1), "h": (2, 1), "v": (1, 2), "hv": (2, 2)}
KINDS = {"rgb": (sm.RGB, 0), "gray": (sm.GRAYSCALE, 0), "ycbcr": (sm.YCBCR, 0), "chw": (sm.RGB, 1)}
GUARD = 256
TILE_PX = {("none", False): 512, ("h", False): 1024, ("v", False): 512, ("hv", False): 512,
           ("none", True): 2048, ("h", True): 2048, ("v", True): 1024, ("hv", True): 1024}


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


def frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags=0, seed=1, index=0, ncomp=3):
    planes, qts = synth.make_frame(W, H, hs, vs, ncomp, seed=seed, frame_index=index)
    cs, layout = KINDS[kind]
    d = zj.FrameDesc.make(W, H, hs, vs, ncomp, cs, qts)
    d.flags, d.out_layout = flags, layout
    dev = [torch.from_numpy(np.ascontiguousarray(p, np.int16)).cuda() for p in planes]
    torch.cuda.synchronize()  # (the uploads are torch's, the reads the library's stream)
    return d, dev, planes, qts


def model(W, H, hs, vs, qts, planes, sl, kind, flags=0, ncomp=3):
    cs, layout = KINDS[kind]
    return sm.decode_scaled(W, H, hs, vs, ncomp, cs, qts, planes, sl, chw=layout == 1, clamp_dc=bool(flags & 2))


def run_scaled(zj, ctx, torch, d, frames, scale, windows=None, out_pitch=0):
    """every crop in one buffer with GUARD poisoned bytes around each, at unaligned addresses; returns the crops (host)"""
    n = len(frames)
    rw, rh = zj.scaled_size(d, scale)
    wins = windows if windows is not None else [(0, 0, rw, rh)] * n
    lens = [zj.scaled_crop_out_len(d, scale, w[2], w[3], out_pitch) for w in wins]
    assert all(lens)
    offs, o = [], GUARD
    for i, ln in enumerate(lens):
        offs.append(o + (i % 3))
        o += ln + GUARD + 3
    buf = torch.full((o + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    base = buf.data_ptr()
    ptr = lambda f, c: f[c].data_ptr() if len(f) > c else None
    cb = [ptr(f, 1) for f in frames] if len(frames[0]) > 1 else None
    cr = [ptr(f, 2) for f in frames] if len(frames[0]) > 1 else None
    ctx.decode_crops_scaled_device(d, [f[0].data_ptr() for f in frames], cb, cr, scale, [base + x for x in offs], windows, out_pitch)
    ctx.sync()
    a = buf.cpu().numpy()
    written = np.zeros(a.size, bool)
    outs = []
    for x, ln in zip(offs, lens):
        written[x:x + ln] = True
        outs.append(a[x:x + ln])
    assert (a[~written] == 0xAA).all(), "a crop wrote outside its bytes"
    return outs


def check(outs, exp, wins, kind, out_pitch=0, what=""):
    chw = kind == "chw"
    bpp = 1 if chw or kind == "gray" else 3
    for got, (x, y, w, h) in zip(outs, wins):
        pitch = out_pitch or w * bpp
        rows = got.reshape(3, h, pitch) if chw else got.reshape(h, pitch)
        want = exp[:, y:y + h, x:x + w] if chw else exp[y:y + h, x:x + w].reshape(h, w * bpp)
        body = rows[..., :w * bpp]
        if not np.array_equal(body, want):
            raise AssertionError(f"{what} window {(x, y, w, h)}: {(body != want).sum()} bytes differ from the model")
        assert (rows[..., w * bpp:] == 0xAA).all(), "pitch padding written"


def windows_of(rw, rh, rng, extra=4):
    w2, h2 = max(1, rw // 2), max(1, rh // 2)
    wins = [(0, 0, rw, rh), (0, 0, 1, 1), (rw - 1, rh - 1, 1, 1), (rw - 1, 0, 1, 1), (0, rh - 1, 1, 1),
            (0, 0, w2, h2), (rw - w2, 0, w2, h2), (0, rh - h2, w2, h2), (rw - w2, rh - h2, w2, h2),
            (0, rh // 3, rw, 1), (rw // 3, 0, 1, rh)]
    for _ in range(extra):
        w, h = int(rng.integers(1, rw + 1)), int(rng.integers(1, rh + 1))
        wins.append((int(rng.integers(rw - w + 1)), int(rng.integers(rh - h + 1)), w, h))
    return wins


# ---- 7. zj_decode_crops_scaled_device equals the model -----------------------------------------------------------
@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mode", list(MODES))
def test_scaled_equals_the_model(zj, ctx, torch, synth, mode, kind, scale):
    """a SUBSET of the emulation test's cases (tests/test_scaled_emu.py runs all of them on the CPU): every third small
    width and height, three of its four frames around the tile width, windows at every edge and corner, of one pixel, two of
    its three windows across the tile seam; a padded pitch"""
    hs, vs = MODES[mode]
    sl = {2: 1, 4: 2, 8: 3}[scale]
    rng = np.random.default_rng(zlib.crc32(f"{mode}-{kind}-{scale}".encode()))
    T = TILE_PX[(mode, kind == "gray")]
    small = [(W, (7 * W) % 40 + 1) for W in range(1, 41, 3)] + [((11 * H) % 40 + 1, H) for H in range(2, 41, 3)]
    for (W, H) in small:
        d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, seed=W * 41 + H)
        assert zj.scaled_size(d, scale) == sm.scaled_size(W, H, sl)
        rw, rh = sm.scaled_size(W, H, sl)
        check(run_scaled(zj, ctx, torch, d, [dev], scale), model(W, H, hs, vs, qts, planes, sl, kind), [(0, 0, rw, rh)], kind,
              what=f"{mode} {kind} 1/{scale} {W}x{H}")
    for (W, H, flags) in [(T - 1, 19, 0), (T + 1, 33, 7), (2 * T + 5, 17, 2), (100, 70, 0)]:
        d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags=flags, seed=W + H)
        exp = model(W, H, hs, vs, qts, planes, sl, kind, flags)
        rw, rh = sm.scaled_size(W, H, sl)
        wins = windows_of(rw, rh, rng)
        if rw > T // scale:
            wins += [(T // scale - 1, 0, 2, rh), (T // scale, rh - 1, rw - T // scale, 1)]
        what = f"{mode} {kind} 1/{scale} {W}x{H} flags {flags}"
        check(run_scaled(zj, ctx, torch, d, [dev] * len(wins), scale, wins), exp, wins, kind, what=what)
        w, h = min(rw, 37), min(rh, 11)
        bpp = 1 if kind in ("chw", "gray") else 3
        pitch = (w * bpp + 127) // 128 * 128 + 3
        pw = [(0, 0, w, h), (rw - w, rh - h, w, h)]
        check(run_scaled(zj, ctx, torch, d, [dev] * 2, scale, pw, out_pitch=pitch), exp, pw, kind, out_pitch=pitch, what=what + " pitch")


@pytest.mark.parametrize("n", [1, 32, 33])
def test_scaled_batches_of_scattered_frames(zj, ctx, torch, synth, n):
    W, H, hs, vs = 300, 100, 2, 2
    rng = np.random.default_rng(n)
    frames, exps, wins = [], [], []
    for i in range(n):
        d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, hs, vs, "rgb", seed=17, index=i)
        frames.append(dev)
        exps.append(model(W, H, hs, vs, qts, planes, 1, "rgb"))
        w, h = int(rng.integers(1, 151)), int(rng.integers(1, 51))
        wins.append((int(rng.integers(150 - w + 1)), int(rng.integers(50 - h + 1)), w, h))
    outs = run_scaled(zj, ctx, torch, d, frames, 2, wins)
    for i in range(n):
        check([outs[i]], exps[i], [wins[i]], "rgb", what=f"frame {i} of {n}")


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_scaled_whole_4096_frame(zj, ctx, torch, synth, scale):
    sl = {2: 1, 4: 2, 8: 3}[scale]
    d, dev, planes, qts = frame_on_device(zj, torch, synth, 4096, 4096, 2, 2, "rgb", seed=4)
    exp = model(4096, 4096, 2, 2, qts, planes, sl, "rgb")
    check(run_scaled(zj, ctx, torch, d, [dev], scale), exp, [(0, 0, 4096 // scale, 4096 // scale)], "rgb", what=f"4096^2 1/{scale}")


@pytest.mark.parametrize("W,H", [(65535, 8), (8, 65535)])
def test_scaled_slivers(zj, ctx, torch, synth, W, H):
    for scale, sl in ((2, 1), (4, 2), (8, 3)):
        for mode in ("hv", "none"):
            hs, vs = MODES[mode]
            d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, hs, vs, "rgb", seed=6)
            rw, rh = sm.scaled_size(W, H, sl)
            exp = model(W, H, hs, vs, qts, planes, sl, "rgb")
            check(run_scaled(zj, ctx, torch, d, [dev], scale), exp, [(0, 0, rw, rh)], "rgb", what=f"{W}x{H} {mode} 1/{scale}")


def test_scaled_single_component(zj, ctx, torch, synth):
    d, dev, planes, qts = frame_on_device(zj, torch, synth, 45, 23, 1, 1, "gray", seed=4, ncomp=1)
    for scale, sl in ((2, 1), (4, 2), (8, 3)):
        rw, rh = sm.scaled_size(45, 23, sl)
        check(run_scaled(zj, ctx, torch, d, [dev], scale), model(45, 23, 1, 1, qts, planes, sl, "gray", ncomp=1), [(0, 0, rw, rh)], "gray")
    dz, devz, planes, qts = frame_on_device(zj, torch, synth, 45, 23, 1, 1, "rgb", seed=4, ncomp=1)
    outs = run_scaled(zj, ctx, torch, dz, [devz], 2, [(1, 1, 20, 10)], out_pitch=70)
    rows = outs[0].reshape(10, 70)
    assert (rows[:, :60] == 0).all() and (rows[:, 60:] == 0xAA).all()


# ---- 11. argument errors: nothing is launched --------------------------------------------------------------------
def test_scaled_argument_errors_launch_nothing(zj, ctx, torch, synth):
    d, dev, planes, qts = frame_on_device(zj, torch, synth, 100, 50, 2, 2, "rgb", seed=1)
    buf = torch.full((1 << 16,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    o = buf.data_ptr() + GUARD
    L = zj.lib()
    P = C.c_void_p * 1
    ys, cbs, crs, outs = P(dev[0].data_ptr()), P(dev[1].data_ptr()), P(dev[2].data_ptr()), P(o)

    def scaled(desc, sl, win, pitch=0):
        w = (C.c_uint * 4)(*win) if win is not None else None
        return L.zj_decode_crops_scaled_device(ctx.handle, C.byref(desc), 1, ys, cbs, crs, sl, w, outs, pitch, None)

    assert scaled(d, 0, None) == -1 and scaled(d, 4, None) == -1
    for win in [(0, 0, 0, 5), (0, 0, 5, 0), (46, 0, 5, 5), (0, 21, 5, 5), (50, 0, 1, 1)]:
        assert scaled(d, 1, win) == -1, win
    assert scaled(d, 1, (0, 0, 10, 10), pitch=29) == -1
    dp, _, _, _ = frame_on_device(zj, torch, synth, 100, 50, 2, 2, "rgb", seed=1)
    dp.out_pitch = 384
    assert scaled(dp, 1, None) == -1
    rgba = zj.FrameDesc.make(100, 50, 2, 2, 3, 5, qts)
    assert scaled(rgba, 1, None) == -2 and zj.scaled_crop_out_len(rgba, 2, 4, 4) == 0
    win = (C.c_uint * 4)(0, 0, 64, 32)

    def prescaled(desc, filt, k, ow=16, dtype=2):
        return L.zj_decode_crops_resized_prescaled_device(ctx.handle, C.byref(desc), 1, ys, cbs, crs, win, ow, 16, dtype, 0, None,
                                                          None, None, filt, k, C.c_void_p(o), None)

    assert prescaled(d, 0, -1) == -1 and prescaled(d, 0, 4) == -1 and prescaled(d, 5, 1) == -1
    assert prescaled(d, 1, 3, ow=8193) == -1 and prescaled(d, 1, 3, dtype=9) == -1
    assert prescaled(rgba, 0, 3) == -2
    ctx.sync()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xAA).all()
    with pytest.raises(ValueError):
        ctx.decode_crops_scaled_device(d, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], 3, [o])
    with pytest.raises(ValueError):
        ctx.decode_crops_resized_device(d, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], [(0, 0, 64, 32)], 16,
                                        16, 2, 0, o, max_prescale=3)


# ---- 8. the prescaled resized entry point ------------------------------------------------------------------------
def run_resized(zj, ctx, torch, d, frames, wins, ow, oh, dtype, layout, scale, bias, flips, antialias, max_prescale):
    per = zj.resized_out_len(d, ow, oh, dtype)
    n = len(wins)
    buf = torch.full((n * per + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_crops_resized_device(d, [f[0].data_ptr() for f in frames], [f[1].data_ptr() for f in frames],
                                    [f[2].data_ptr() for f in frames], wins, ow, oh, dtype, 1 if layout == "NHWC" else 0,
                                    buf.data_ptr() + GUARD, scale, bias, flips, None, antialias, max_prescale)
    ctx.sync()
    a = buf.cpu().numpy()
    assert (a[:GUARD] == 0xAA).all() and (a[GUARD + n * per:] == 0xAA).all()
    return [a[GUARD + i * per:GUARD + (i + 1) * per] for i in range(n)]


def check_image(got_bytes, exp, dtype, what):
    got = rm.raw_view(got_bytes, dtype).reshape(exp.shape)
    ok = np.array_equal(got.view(np.uint32), exp.view(np.uint32)) if dtype == rm.F32 else np.array_equal(got, exp)
    if not ok:
        raise AssertionError(f"{what}: {(got.view(np.uint8) != exp.view(np.uint8)).sum()} bytes differ from the model")


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("kind", ["rgb", "chw", "gray", "ycbcr"])
@pytest.mark.parametrize("mode", ["hv", "none", "h"])
def test_prescaled_resized_equals_the_models(zj, ctx, torch, synth, mode, kind, antialias):
    """a batch that mixes s = 1, 2, 4, 8; every dtype, both tensor layouts, flips; max_prescale 1 equals the entry point
    without prescaling byte for byte"""
    hs, vs = MODES[mode]
    W, H = 1030, 517
    rng = np.random.default_rng(zlib.crc32(f"{mode}-{kind}-{antialias}".encode()))
    d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, seed=W + hs)
    c = 1 if kind == "gray" else 3
    chw = kind == "chw"
    ow, oh = 40, 30
    # windows for s = 8, 4, 2, 1 (ow x s <= w < 2 ow x s ...), at the frame's edges and inside, and one limited by its height
    wins = [(0, 0, W, H), (W - 330, H - 250, 330, 250), (5, 3, 321, 241), (7, 9, 170, 130), (W - 81, H - 61, 81, 61),
            (100, 100, 79, 300), (3, 5, 40, 30), (11, 2, 1000, 65), (W - 161, 0, 161, 121)]
    for _ in range(5):
        w, h = int(rng.integers(ow, W + 1)), int(rng.integers(oh, H + 1))
        wins.append((int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1)), w, h))
    flips = [bool(i % 3 == 1) for i in range(len(wins))]
    scale, bias = rng.uniform(0.002, 0.03, c).astype(np.float32), rng.uniform(-3, 3, c).astype(np.float32)
    reduced = {sl: model(W, H, hs, vs, qts, planes, sl, kind) for sl in (1, 2, 3)}
    model_resize = am.resize if antialias else rm.resize
    seen = set()
    for dtype in range(4):
        layout = "NHWC" if dtype % 2 else "NCHW"
        for max_prescale in (8, 2):
            outs = run_resized(zj, ctx, torch, d, [dev] * len(wins), wins, ow, oh, dtype, layout, scale, bias, flips, antialias, max_prescale)
            for i, (x, y, w, h) in enumerate(wins):
                k = sm.prescale_log2(w, h, ow, oh, {8: 3, 2: 1}[max_prescale])
                seen.add(k)
                if k == 0:
                    continue  # (checked against the unprescaled call below)
                rx, ry, rw_, rh_ = sm.reduced_window(x, y, w, h, k, W, H)
                img = reduced[k]
                crop = img[:, ry:ry + rh_, rx:rx + rw_] if chw else img[ry:ry + rh_, rx:rx + rw_].transpose(2, 0, 1)
                exp = model_resize(np.ascontiguousarray(crop), ow, oh, dtype, scale, bias, flips[i], layout)
                check_image(outs[i], exp, dtype, f"{mode} {kind} aa {antialias} window {wins[i]} 1/{1 << k} dtype {dtype} {layout}")
            plain = run_resized(zj, ctx, torch, d, [dev] * len(wins), wins, ow, oh, dtype, layout, scale, bias, flips, antialias, 1)
            for i, (x, y, w, h) in enumerate(wins):
                if sm.prescale_log2(w, h, ow, oh, {8: 3, 2: 1}[max_prescale]) == 0:
                    assert np.array_equal(outs[i], plain[i]), f"window {wins[i]} at scale 1 differs from the unprescaled call"
    assert seen == {0, 1, 2, 3}


def test_prescale_zero_is_the_filtered_entry_point(zj, ctx, torch, synth):
    """max_prescale_log2 = 0 through the C ABI equals zj_decode_crops_resized_filtered_device byte for byte"""
    W, H = 800, 600
    d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, 2, 2, "rgb", seed=3)
    wins = [(0, 0, 800, 600), (13, 7, 500, 333), (700, 500, 100, 100)]
    n = len(wins)
    L = zj.lib()
    P = C.c_void_p * n
    ys, cbs, crs = P(*[dev[0].data_ptr()] * n), P(*[dev[1].data_ptr()] * n), P(*[dev[2].data_ptr()] * n)
    win = (C.c_uint * (4 * n))(*[v for w in wins for v in w])
    per = zj.resized_out_len(d, 64, 48, rm.BF16)
    for filt in (0, 1):
        a = torch.full((n * per,), 0xAA, dtype=torch.uint8, device="cuda")
        b = torch.full((n * per,), 0x55, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.zj_decode_crops_resized_filtered_device(ctx.handle, C.byref(d), n, ys, cbs, crs, win, 64, 48, rm.BF16, 0, None, None,
                                                         None, filt, C.c_void_p(a.data_ptr()), None) == 0
        assert L.zj_decode_crops_resized_prescaled_device(ctx.handle, C.byref(d), n, ys, cbs, crs, win, 64, 48, rm.BF16, 0, None, None,
                                                          None, filt, 0, C.c_void_p(b.data_ptr()), None) == 0
        ctx.sync()
        assert torch.equal(a, b)


# ---- 9. the file path ----------------------------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
_MODEL = {}


def _files():
    g = os.path.join(HERE, "golden")
    return [os.path.join(g, "test-baseline.jpg")] + sorted(glob.glob(os.path.join(g, "ref", "*.jp*g")))


def file_model(zj, path, sl):
    """the model over the front-end's own planes of the file (the decoder's default options: the reference's values)"""
    if (path, sl) not in _MODEL:
        desc, planes, info = zj.Decoder().decode_coefficients(open(path, "rb").read())
        qts = [np.array(q) for q in np.ctypeslib.as_array(desc.qt)]
        _MODEL[(path, sl)] = sm.decode_scaled(info.width, info.height, info.h_max, info.v_max, info.components, sm.RGB, qts,
                                              [np.array(p) for p in planes], sl)
    return _MODEL[(path, sl)]


@pytest.mark.parametrize("entropy", ["cpu", "gpu"])
def test_file_path_equals_the_model_over_the_front_ends_planes(zj, torch, entropy):
    """every fixture JPEG the front-end decodes, Huffman stage on the CPU (only the window's plane rows are uploaded, into a
    scratch that holds another file's planes) and on the device: zj_decoder_finish_pixels_scaled_device and
    zj_decoder_finish_pixels_resized_crop_prescaled_device equal the model / the resize models of the model's reduced crop"""
    rng = np.random.default_rng(zlib.crc32(entropy.encode()))
    g = os.path.join(HERE, "golden", "ref")
    poisons = [os.path.join(g, "speed_bench.jpg"), os.path.join(g, "medium_no_samp_2500x1786.jpg")]
    fctx = zj.Context(zj.BACKEND_HIP, 0)

    def opts():
        o = zj.ZuneJpegOptions()
        if entropy == "gpu":
            o.entropy = zj.ENTROPY_GPU_ALWAYS
        return o

    def poison_scratch(path):
        src = poisons[1] if os.path.basename(path) == os.path.basename(poisons[0]) else poisons[0]
        pd = zj.Decoder(zj.ZuneJpegOptions(), fctx)
        desc, _ = pd.prepare(open(src, "rb").read())
        n = zj.lib().zj_out_len(C.byref(desc))
        b = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert pd.finish_pixels_device(b.data_ptr(), n) == n
        pd.close()

    def guarded(nbytes):
        buf = torch.full((nbytes + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return buf

    def read(buf, nbytes):
        a = buf.cpu().numpy()
        assert (a[:GUARD] == 0xAA).all() and (a[GUARD + nbytes:] == 0xAA).all(), "a byte outside the output was written"
        return a[GUARD:GUARD + nbytes]

    checked = 0
    try:
        for path in _files():
            data = open(path, "rb").read()
            dec = zj.Decoder(opts(), fctx)
            try:
                desc, _ = dec.prepare(data)
            except zj.ZjError:  # (not a file the front-end decodes: arithmetic coding)
                dec.close()
                continue
            W, H = desc.width, desc.height
            name = os.path.basename(path)
            scales = (1, 2, 3) if W * H <= 6000000 else (2,)
            for sl in scales:
                exp = file_model(zj, path, sl)
                rh, rw = exp.shape[:2]
                w, h = int(rng.integers(1, rw + 1)), int(rng.integers(1, max(2, rh // 3)))
                wins = [None, (int(rng.integers(rw - w + 1)), int(rng.integers(rh - h + 1)), w, h), (rw - 1, rh - 1, 1, 1)]
                for win in wins[(0 if sl == scales[0] else 1):]:
                    x, y, ww, hh = win if win is not None else (0, 0, rw, rh)
                    n = zj.scaled_crop_out_len(desc, 1 << sl, ww, hh)
                    buf = guarded(n)
                    poison_scratch(path)
                    dec.prepare(data)
                    assert dec.finish_pixels_scaled_device(1 << sl, buf.data_ptr() + GUARD, n, win) == n
                    got = read(buf, n).reshape(hh, ww, 3)
                    assert np.array_equal(got, exp[y:y + hh, x:x + ww]), f"{name} {entropy} 1/{1 << sl} window {win}"
                    checked += 1
            # the prescaled resized crop: a window that decodes at 1/2 or below, both filters
            ow, oh = 48, 40
            for k_try, antialias, dtype in (((3, True, rm.BF16), (1, False, rm.F32)) if desc.in_components == 3 else ()):
                w, h = min(W, int(rng.integers(ow << k_try, (ow << k_try) * 2))), min(H, int(rng.integers(oh << k_try, (oh << k_try) * 2)))
                x, y = int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))
                k = sm.prescale_log2(w, h, ow, oh, k_try)
                if k == 0 or (k not in scales):
                    continue
                rx, ry, cw, ch = sm.reduced_window(x, y, w, h, k, W, H)
                crop = np.ascontiguousarray(file_model(zj, path, k)[ry:ry + ch, rx:rx + cw].transpose(2, 0, 1))
                per = zj.resized_out_len(desc, ow, oh, dtype)
                buf = guarded(per)
                poison_scratch(path)
                dec.prepare(data)
                assert dec.finish_pixels_resized_crop_device(x, y, w, h, ow, oh, dtype, zj.TENSOR_NCHW, buf.data_ptr() + GUARD, per,
                                                             [0.01] * 3, [-1.0] * 3, flip=True, antialias=antialias,
                                                             max_prescale=1 << k_try) == per
                exp = (am.resize if antialias else rm.resize)(crop, ow, oh, dtype, [0.01] * 3, [-1.0] * 3, True, "NCHW")
                check_image(read(buf, per), exp, dtype, f"{name} {entropy} prescaled window {(x, y, w, h)} 1/{1 << k}")
                checked += 1
            # argument errors leave the output alone
            buf = guarded(64)
            dec.prepare(data)
            for bad in ((4, None), (2, (0, 0, 0, 0)), (2, (zj.scaled_size(desc, 2)[0], 0, 1, 1))):
                with pytest.raises((zj.ZjError, ValueError)):
                    dec.finish_pixels_scaled_device(bad[0] if bad[0] != 4 else 16, buf.data_ptr() + GUARD, 64, bad[1])
            read(buf, 64)
            dec.close()
    finally:
        fctx.close()
    assert checked >= 20


# ---- 10. tensors ---------------------------------------------------------------------------------------------------
def test_scaled_tensors(zj, ctx, torch, synth):
    tz = importlib.import_module("zune-jpeg_amd.tensors")
    W, H = 203, 77
    for kind, shape in (("rgb", (3, 20, 30, 3)), ("chw", (3, 3, 20, 30)), ("gray", (3, 20, 30))):
        frames, exps = [], []
        for i in range(3):
            d, dev, planes, qts = frame_on_device(zj, torch, synth, W, H, 2, 2, kind, seed=9, index=i)
            frames.append(tuple(dev))
            exps.append(model(W, H, 2, 2, qts, planes, 1, kind))
        wins = [(0, 0, 30, 20), (72, 19, 30, 20), (5, 6, 30, 20)]
        side = torch.cuda.Stream()
        for stream in (None, side):
            t = tz.decode_scaled_to_tensor(ctx, d, frames, 2, wins, stream=stream)
            (stream or torch.cuda.current_stream()).synchronize()
            assert t.shape == shape and t.dtype == torch.uint8 and t.is_contiguous()
            for i, (x, y, w, h) in enumerate(wins):
                e = exps[i][:, y:y + h, x:x + w] if kind == "chw" else exps[i][y:y + h, x:x + w].reshape(t[i].shape)
                assert np.array_equal(t[i].cpu().numpy(), e)
        whole = tz.decode_scaled_to_tensor(ctx, d, frames, 4)
        torch.cuda.synchronize()
        rw, rh = sm.scaled_size(W, H, 2)
        assert whole.shape[0] == 3 and tuple(whole.shape[-2:] if kind != "rgb" else whole.shape[1:3]) == (rh, rw)
    with pytest.raises(ValueError):
        tz.decode_scaled_to_tensor(ctx, d, frames, 2, [(0, 0, 30, 20), (0, 0, 31, 20), (0, 0, 30, 20)])
    for bad in (1, 3, 16, 0):
        with pytest.raises(ValueError):
            tz.decode_scaled_to_tensor(ctx, d, frames, bad)
    with pytest.raises(ValueError):
        tz.decode_scaled_to_tensor(ctx, d, frames, 2, [(0, 0, 200, 20)] * 3)
    with pytest.raises(ValueError):
        tz.decode_resized_crops_to_tensor(ctx, d, frames, [(0, 0, 100, 50)] * 3, (16, 16), max_prescale=3)


# What prescaling costs end to end: the prescaled antialiased, normalised bf16 tensor against F.interpolate(antialias=True)
# of the full decode, on a smooth synthetic frame, next to the 0.0156 of the unprescaled path.
# MEASURED on an MI355X; asserted: that value plus one bf16 step at the normalised range (2^-6).
PRESCALE_MEASURED = 0.0446  # (max_prescale=1 in the same run: 0.0078)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def smooth_planes(W, H):
    """a smooth 4:4:4 frame: slow sinusoids per component, transformed block by block (orthonormal 8 x 8 DCT) and kept
    at table entries of 1, chroma small enough that no RGB value clamps"""
    a8 = sm.float_matrix(8)  # x = A8 X per axis, A8 orthonormal: X = A8^T x
    bw, bh = (W + 7) // 8, (H + 7) // 8
    yy, xx = np.mgrid[0:bh * 8, 0:bw * 8].astype(np.float64)
    planes = []
    for c, amp in enumerate((70.0, 18.0, 18.0)):
        f = amp * (0.6 * np.sin(xx / (41.0 + 9 * c) + c) + 0.4 * np.cos(yy / (57.0 - 5 * c) + 0.3 * xx / 100.0))
        blocks = f.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        coef = np.einsum("nk,abnm,ml->abkl", a8, blocks, a8)
        planes.append(np.rint(coef).astype(np.int16).reshape(-1))
    return planes, [np.ones(64, np.int32)] * 3


def test_prescaled_tensor_against_interpolate(zj, ctx, torch, synth):
    import torch.nn.functional as F
    tz = importlib.import_module("zune-jpeg_amd.tensors")
    W, H = 2048, 1536
    planes, qts = smooth_planes(W, H)
    d = zj.FrameDesc.make(W, H, 1, 1, 3, sm.RGB, qts)
    d.flags = 7
    dev = tuple(torch.from_numpy(p).cuda() for p in planes)
    torch.cuda.synchronize()
    full = tz.decode_to_tensor(ctx, d, list(dev), 1)
    torch.cuda.synchronize()
    img = full[0].permute(2, 0, 1).float().div(255)[None]
    wins = [(0, 0, W, H), (100, 60, 1800, 1400), (300, 200, 900, 700), (64, 32, 448, 448)]
    worst = {}
    for mp in (1, 8):
        t = tz.decode_resized_crops_to_tensor(ctx, d, [dev] * len(wins), wins, (224, 224), dtype=torch.bfloat16, mean=MEAN,
                                              std=STD, antialias=True, max_prescale=mp)
        torch.cuda.synchronize()
        w = 0.0
        for i, (x, y, ww, hh) in enumerate(wins):
            ref = F.interpolate(img[:, :, y:y + hh, x:x + ww], size=(224, 224), mode="bilinear", antialias=True, align_corners=False)
            ref = (ref - torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)) / torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
            w = max(w, float((t[i].float() - ref[0]).abs().max()))
        worst[mp] = w
    print(f"prescaled antialiased tensor vs F.interpolate(antialias=True): max_prescale=1 {worst[1]:.4f}, max_prescale=8 {worst[8]:.4f}")
    assert worst[8] <= PRESCALE_MEASURED + 2.0 ** -6
