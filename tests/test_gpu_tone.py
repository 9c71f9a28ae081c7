"""GPU: per-image tone curves on an MI355X, every comparison on bytes or counts against the numpy model
(tests/tone_model.py, which tests/test_tone_model.py pins to Pillow's ImageOps).
1. zj_histogram_device: the emulation's width and height set in both layouts with padded pitches, odd offsets and a padding
   value no image uses; one flat 1024 x 1024 image (2^20 in one bin through many workgroups); 129 images in one call.
2. zj_tone_luts_device over synthetic histograms uploaded from the host: all 32 640 (lo, hi) pairs of autocontrast against
   the Python-double formula, the equalize set with the 65535^2 total, the ops that need no histogram with d_hist NULL.
3. zj_lut_device: permutation tables, in place and apart, poisoned surroundings, odd source offsets.
4. zj_tone_device: every op on 37 x 3, 130 x 5 and 300 x 200, twice on one context with different sizes.
5. One far-offset case per kernel (tests/far_cases.py).
6. The plane call and the file-batch call against their stages; tone NULL is the coloured call; a refused op fails its file.
7. The tensors wrappers."""
import ctypes as C
import importlib

import numpy as np
import pytest

import far_cases as fc
import tone_model as tm
from tone_cases import HEIGHTS, WIDTHS, Arena, permutations, stretches

pytestmark = pytest.mark.gpu
POISON, PAD = 0xA5, 250      # PAD: what the padding between rows holds; the images use 0..199 where that matters
ERR_ARG, ERR_UNSUPPORTED = -1, -2
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ALL_OPS = [(tm.IDENTITY, 0), (tm.INVERT, 0), (tm.POSTERIZE, 3), (tm.SOLARIZE, 100), (tm.AUTOCONTRAST, 0), (tm.EQUALIZE, 0),
           (tm.POSTERIZE, 8), (tm.SOLARIZE, 0), (tm.SOLARIZE, 256), (tm.POSTERIZE, 1)]


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def tz():
    return importlib.import_module("zune-jpeg_amd.tensors")


@pytest.fixture(scope="module")
def synth():
    return importlib.import_module("zune-jpeg_amd.synth")


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
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import jpeg_enc
    return jpeg_enc


def layout_of(zj, chw):
    return zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC


def cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hist_of(zj, ctx, torch, ar):
    d = cuda(torch, ar.buf)
    hist = torch.full((len(ar.sizes), ar.channels, 256), -1, dtype=torch.int32, device="cuda")   # (overwritten, not added to)
    torch.cuda.synchronize()
    ctx.histogram_device([d.data_ptr() + o for o in ar.off], ar.sizes, ar.channels, layout_of(zj, ar.chw), hist.data_ptr(), ar.pitch)
    ctx.sync()
    assert np.array_equal(d.cpu().numpy(), ar.buf), "the histogram wrote to its input"
    return hist.cpu().numpy().view(np.uint32).astype(np.int64)


# ---- 1. the histogram ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,chw", [(3, False), (3, True), (1, False)], ids=["HWC", "CHW", "L"])
def test_histogram_equals_the_model(zj, ctx, torch, channels, chw):
    """widths around the 16-pixel run, heights 1 and 3, and one image a run larger than a workgroup's share (2049 runs);
    padded pitches whose padding holds a value no image uses"""
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(16 * 2049, 1), (16 * 683, 3)]
    ar = Arena(sizes, channels, chw, np.random.default_rng(3 + channels + chw), PAD, 0, 200)
    got = hist_of(zj, ctx, torch, ar)
    for i in range(len(sizes)):
        assert np.array_equal(got[i], tm.histogram(ar.image(i), chw)), (i, sizes[i])
    assert got[:, :, 200:].sum() == 0, "padding was counted"


@pytest.mark.parametrize("channels,chw", [(3, False), (3, True), (1, False)], ids=["HWC", "CHW", "L"])
def test_histogram_of_stretches_of_equal_neighbours(zj, ctx, torch, channels, chw):
    """rows made of stretches of one value, 1 to 40 pixels long: a stretch inside a lane's run is one add of its length"""
    rng = np.random.default_rng(31 + channels + chw)
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(300, 7), (4097, 2)]
    ar = stretches(rng, Arena(sizes, channels, chw, rng, PAD, 0, 200))
    got = hist_of(zj, ctx, torch, ar)
    for i in range(len(sizes)):
        assert np.array_equal(got[i], tm.histogram(ar.image(i), chw)), (i, sizes[i])


def test_histogram_of_a_flat_image_sums_across_workgroups(zj, ctx, torch):
    """1024 x 1024 of one value: 2^20 in one bin of each channel, from 32 workgroups"""
    img = torch.empty((1024, 1024, 3), dtype=torch.uint8, device="cuda")
    img[..., 0], img[..., 1], img[..., 2] = 7, 255, 0
    hist = torch.empty((1, 3, 256), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):   # (the second call overwrites the first one's counts)
        ctx.histogram_device([img.data_ptr()], [(1024, 1024)], 3, zj.LAYOUT_HWC, hist.data_ptr())
    ctx.sync()
    want = np.zeros((1, 3, 256), np.int64)
    want[0, 0, 7] = want[0, 1, 255] = want[0, 2, 0] = 1 << 20
    assert np.array_equal(hist.cpu().numpy(), want)


def test_histogram_of_129_images_takes_a_second_launch(zj, ctx, torch):
    rng = np.random.default_rng(9)
    sizes = [(int(rng.integers(1, 90)), int(rng.integers(1, 12))) for _ in range(129)]
    ar = Arena(sizes, 3, False, rng, PAD, 0, 200)
    got = hist_of(zj, ctx, torch, ar)
    for i in range(129):
        assert np.array_equal(got[i], tm.histogram(ar.image(i))), i


# ---- 2. the table build ----------------------------------------------------------------------------------------------------
def luts_of(ctx, torch, ops, channels, hist):
    n = len(ops)
    d_hist = cuda(torch, np.asarray(hist, np.uint32).reshape(n, channels, 256).view(np.int32)) if hist is not None else None
    luts = torch.full((n, channels, 256), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.tone_luts_device(ops, channels, d_hist.data_ptr() if d_hist is not None else None, luts.data_ptr())
    ctx.sync()
    return luts.cpu().numpy()


def test_every_lo_hi_pair_of_autocontrast_equals_the_python_doubles(ctx, torch):
    """all 32 640 pairs as two-bin histograms: the product and the sum rounded separately, on the device"""
    pairs = tm.autocontrast_pairs()
    assert len(pairs) == 32640
    hist = np.zeros((len(pairs), 256), np.uint32)
    for k, (lo, hi) in enumerate(pairs):
        hist[k, lo], hist[k, hi] = 3, 5
    got = luts_of(ctx, torch, [(tm.AUTOCONTRAST, 0)] * len(pairs), 1, hist)
    i = np.arange(256)
    bad = []
    for k, (lo, hi) in enumerate(pairs):
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        want = [min(255, max(0, int(j * scale + offset))) for j in i]
        if not np.array_equal(got[k, 0], want):
            bad.append((lo, hi))
    assert not bad, f"{len(bad)} pairs differ, first {bad[:5]}"


def test_the_equalize_cases_and_the_64_bit_sum(ctx, torch):
    cases = tm.equalize_cases()
    names = sorted(cases)
    # three channels: case k in channel 0, its neighbours in channels 1 and 2 (every channel its own bins)
    hist = np.array([[cases[names[(k + c) % len(names)]] for c in range(3)] for k in range(len(names))], np.uint64)
    assert hist.max() < 2 ** 32
    got = luts_of(ctx, torch, [(tm.EQUALIZE, 0)] * len(names), 3, hist.astype(np.uint32))
    for k, name in enumerate(names):
        for c in range(3):
            other = names[(k + c) % len(names)]
            assert np.array_equal(got[k, c], tm.table(tm.EQUALIZE, 0, cases[other])), (name, c, other)
    # ... and autocontrast over the same bins
    got = luts_of(ctx, torch, [(tm.AUTOCONTRAST, 0)] * len(names), 3, hist.astype(np.uint32))
    for k, name in enumerate(names):
        assert np.array_equal(got[k, 0], tm.table(tm.AUTOCONTRAST, 0, cases[name])), name


def test_ops_without_a_histogram_take_none(zj, ctx, torch):
    ops = [(tm.IDENTITY, 0), (tm.INVERT, 0)] + [(tm.POSTERIZE, b) for b in range(1, 9)] + [(tm.SOLARIZE, t) for t in (0, 1, 128, 255, 256)]
    ops = ops * 18                     # 270 ops: a second launch
    for channels in (1, 3):
        got = luts_of(ctx, torch, ops, channels, None)
        for k, (op, param) in enumerate(ops):
            assert np.array_equal(got[k], tm.tables(op, param, None, channels)), (k, op, param)
    luts = torch.full((2, 1, 256), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(zj.ZjError) as e:   # an op that needs the bins, and none given: refused before anything is launched
        ctx.tone_luts_device([(tm.INVERT, 0), (tm.EQUALIZE, 0)], 1, None, luts.data_ptr())
    assert e.value.status == ERR_ARG
    for bad in [(6, 0), (-1, 0), (tm.POSTERIZE, 0), (tm.POSTERIZE, 9), (tm.SOLARIZE, 257), (tm.SOLARIZE, -1), (tm.INVERT, 1), (tm.EQUALIZE, 2)]:
        with pytest.raises(zj.ZjError) as e:
            ctx.tone_luts_device([(tm.INVERT, 0), bad], 1, None, luts.data_ptr())
        assert e.value.status == ERR_ARG, bad
    ctx.sync()
    assert bool((luts == POISON).all())


# ---- 3. the lookup ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("channels,chw", [(3, False), (3, True), (1, False)], ids=["HWC", "CHW", "L"])
def test_lookup_under_permutation_tables(zj, ctx, torch, channels, chw, in_place):
    rng = np.random.default_rng(21 + channels + 2 * chw + 4 * in_place)
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(300, 20)]
    src = Arena(sizes, channels, chw, rng, POISON)
    dst = src if in_place else Arena(sizes, channels, chw, rng, POISON, pads=(13, 0, 1, 5), data=False)
    luts = permutations(rng, len(sizes), channels)
    # (the table at an odd address as well: its bytes are then loaded singly)
    for shift in (0, 1):
        d_src = cuda(torch, src.buf)
        d_dst = d_src if in_place else cuda(torch, dst.buf)
        d_luts = torch.zeros(luts.size + 1, dtype=torch.uint8, device="cuda")
        d_luts[shift:shift + luts.size] = cuda(torch, luts.reshape(-1))
        torch.cuda.synchronize()
        ctx.lut_device([d_src.data_ptr() + o for o in src.off], sizes, channels, layout_of(zj, chw), d_luts.data_ptr() + shift,
                       [d_dst.data_ptr() + o for o in dst.off], src.pitch, dst.pitch)
        ctx.sync()
        got = d_dst.cpu().numpy()
        for i in range(len(sizes)):
            assert np.array_equal(dst.image(i, got), tm.apply_luts(src.image(i), luts[i], chw)), (i, sizes[i], shift)
        assert (got[~dst.inside] == POISON).all(), "a padding or guard byte was written"
        if not in_place:
            assert np.array_equal(d_src.cpu().numpy(), src.buf), "an input was written"


def test_stage_argument_errors_launch_nothing(zj, ctx, torch):
    a = torch.full((256,), 200, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), POISON, dtype=torch.uint8, device="cuda")
    luts = cuda(torch, np.tile(np.arange(256, dtype=np.uint8)[::-1], 6))
    hist = torch.full((2, 3, 256), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = zj.lib()
    arr = lambda v: (C.c_void_p * len(v))(*v) if v is not None else None
    u = lambda v: (C.c_uint * len(v))(*v) if v is not None else None
    ops = lambda v: (C.c_int32 * len(v))(*v) if v is not None else None
    pa, po, pl, ph = a.data_ptr(), dst.data_ptr(), luts.data_ptr(), hist.data_ptr()
    tone = lambda n, ins, wh, ip, ch, lay, op, outs, opit, h=ctx.handle: L.zj_tone_device(h, n, arr(ins), u(wh), u(ip), ch, lay, ops(op), arr(outs), u(opit), None)
    lut = lambda n, ins, wh, ip, ch, lay, t, outs, opit, h=ctx.handle: L.zj_lut_device(h, n, arr(ins), u(wh), u(ip), ch, lay, t, arr(outs), u(opit), None)
    hst = lambda n, ins, wh, ip, ch, lay, t, h=ctx.handle: L.zj_histogram_device(h, n, arr(ins), u(wh), u(ip), ch, lay, t, None)
    inv = [tm.INVERT, 0]
    assert tone(1, [pa], [4, 4], None, 3, 0, inv, [po], None, h=None) == ERR_ARG
    assert tone(1, None, [4, 4], None, 3, 0, inv, [po], None) == ERR_ARG
    assert tone(1, [pa], None, None, 3, 0, inv, [po], None) == ERR_ARG
    assert tone(1, [pa], [4, 4], None, 3, 0, None, [po], None) == ERR_ARG
    assert tone(1, [pa], [4, 4], None, 3, 0, inv, None, None) == ERR_ARG
    assert tone(0, [pa], [4, 4], None, 3, 0, inv, [po], None) == ERR_ARG
    assert tone(1, [pa], [4, 4], None, 2, 0, inv, [po], None) == ERR_ARG                     # channels
    assert tone(1, [pa], [4, 4], None, 3, 2, inv, [po], None) == ERR_ARG                     # layout
    assert tone(2, [pa, pa], [4, 4, 0, 4], None, 3, 0, inv * 2, [po, po + 64], None) == ERR_ARG
    assert tone(1, [pa], [65536, 1], None, 1, 0, inv, [po], None) == ERR_ARG
    assert tone(1, [pa], [4, 4], [11], 3, 0, inv, [po], None) == ERR_ARG                     # a pitch below a row
    assert tone(1, [pa], [4, 4], None, 3, 1, inv, [po], [3]) == ERR_ARG
    assert tone(1, [pa], [4, 4], [(1 << 24) + 1], 1, 0, inv, [po], None) == ERR_ARG
    assert tone(2, [pa, pa], [4, 4, 4, 4], None, 3, 0, inv + [tm.POSTERIZE, 9], [po, po + 64], None) == ERR_ARG   # the second op
    assert tone(2, [pa, pa], [4, 4, 4, 4], None, 3, 0, inv + [7, 0], [po, po + 64], None) == ERR_ARG
    assert lut(1, [pa], [4, 4], None, 3, 0, None, [po], None) == ERR_ARG
    assert lut(1, [pa], [4, 4], None, 3, 0, pl, [None], None) == ERR_ARG
    assert lut(1, [pa], [4, 4], None, 4, 0, pl, [po], None) == ERR_ARG
    assert lut(1, [pa], [4, 4], None, 3, 0, pl, [po], None, h=None) == ERR_ARG
    assert hst(1, [pa], [4, 4], None, 3, 0, None) == ERR_ARG
    assert hst(1, [pa], [4, 4], None, 3, 0, ph + 2) == ERR_ARG                                # not a uint32 address
    assert hst(1, [pa], [4, 0], None, 3, 0, ph) == ERR_ARG
    assert hst(1, [None], [4, 4], None, 3, 0, ph) == ERR_ARG
    ctx.sync()
    assert bool((dst == POISON).all()) and bool((hist == 7).all())
    assert tone(1, [pa], [4, 4], None, 3, 0, inv, [po], None) == 0
    ctx.sync()
    assert bool((dst[:48] == 55).all()) and bool((dst[48:] == POISON).all())


# ---- 4. the whole stage ----------------------------------------------------------------------------------------------------
def tone_call(zj, ctx, torch, rng, sizes, ops, channels, chw, in_place):
    src = Arena(sizes, channels, chw, rng, POISON, 30, 220)
    dst = src if in_place else Arena(sizes, channels, chw, rng, POISON, pads=(5, 0, 13, 1), data=False)
    d_src = cuda(torch, src.buf)
    d_dst = d_src if in_place else cuda(torch, dst.buf)
    torch.cuda.synchronize()
    ctx.tone_device([d_src.data_ptr() + o for o in src.off], sizes, channels, layout_of(zj, chw), ops,
                    [d_dst.data_ptr() + o for o in dst.off], src.pitch, dst.pitch)
    ctx.sync()
    got = d_dst.cpu().numpy()
    for i, (op, param) in enumerate(ops):
        assert np.array_equal(dst.image(i, got), tm.apply(op, param, src.image(i), chw)), (i, sizes[i], op, param)
    assert (got[~dst.inside] == POISON).all(), "a padding or guard byte was written"


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("channels,chw", [(3, False), (3, True), (1, False)], ids=["HWC", "CHW", "L"])
def test_tone_device_equals_the_model_for_every_op(zj, ctx, torch, channels, chw, in_place):
    """every op on 37 x 3, 130 x 5 and 300 x 200, IDENTITY among them; then the same context again with other sizes and
    fewer images: the context's tables and histograms are reused"""
    rng = np.random.default_rng(60 + channels + 2 * chw + 4 * in_place)
    ops = [op for op in ALL_OPS for _ in range(3)]
    sizes = [(37, 3), (130, 5), (300, 200)] * len(ALL_OPS)
    tone_call(zj, ctx, torch, rng, sizes, ops, channels, chw, in_place)
    tone_call(zj, ctx, torch, rng, [(130, 5), (17, 9), (300, 200), (64, 64)],
              [(tm.EQUALIZE, 0), (tm.AUTOCONTRAST, 0), (tm.AUTOCONTRAST, 0), (tm.EQUALIZE, 0)], channels, chw, in_place)


def test_identity_images_in_place_are_left_alone_and_apart_are_copied(zj, ctx, torch):
    rng = np.random.default_rng(5)
    sizes = [(37, 3), (130, 5)]
    tone_call(zj, ctx, torch, rng, sizes, [(tm.IDENTITY, 0)] * 2, 3, False, True)
    tone_call(zj, ctx, torch, rng, sizes, [(tm.IDENTITY, 0)] * 2, 3, False, False)


# ---- 5. rows past 2^31 and 2^32 bytes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_far_rows_in_the_histogram_and_the_lookup(zj, ctx, torch, chw):
    """one image whose rows lie STAGE_PITCHES[1] bytes apart: the last row (HWC) or plane (CHW) starts past 2^32.  Every row
    has its own value range, so a row read from a wrapped offset shows in the counts; the lookup goes far to far in place"""
    from test_gpu_far_offsets import DevFar, need
    pitch, w = fc.STAGE_PITCHES[1], fc.STAGE_WIDTHS[1]
    npl, h, rb = (3, fc.STAGE_H_CHW, w) if chw else (1, fc.STAGE_H_HWC, 3 * w)
    assert fc.crosses(pitch, h, npl) and fc.crosses(pitch, h, npl, fc.LINE31)
    need(torch, npl * h * pitch)
    rng = np.random.default_rng(17 + chw)
    rows = rng.integers(0, 64, (npl, h, rb), dtype=np.uint8) + (np.arange(npl * h, dtype=np.uint8).reshape(npl, h, 1) % 4) * 64
    far = DevFar(torch, npl, h, rb, pitch).put(rows)
    img = rows.reshape(3, h, w) if chw else rows.reshape(h, w, 3)
    hist = torch.empty((1, 3, 256), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.histogram_device([far.ptr], [(w, h)], 3, layout_of(zj, chw), hist.data_ptr(), [pitch])
    ctx.sync()
    assert np.array_equal(hist.cpu().numpy()[0], tm.histogram(img, chw))
    luts = permutations(rng, 1, 3)
    d_luts = cuda(torch, luts)
    ctx.lut_device([far.ptr], [(w, h)], 3, layout_of(zj, chw), d_luts.data_ptr(), [far.ptr], [pitch], [pitch])
    ctx.sync()
    got = far.get()
    want = tm.apply_luts(img, luts[0], chw).reshape(npl, h, rb)
    for r in fc.lines(pitch, h, npl):
        assert np.array_equal(got.reshape(-1, rb)[r], want.reshape(-1, rb)[r]), f"row {r} (offset {r * pitch:#x}) differs"
    assert np.array_equal(got, want) and far.padding_untouched()


def test_far_tables_in_the_table_build(ctx, torch):
    """700 000 images of three channels: the last images' bins lie past 2^31 bytes (a call takes 2^20 images at most, so no
    table of this stage starts past 2^32)"""
    n = 700_000
    assert (n - 1) * 3 * 1024 >= fc.LINE31
    hist = torch.zeros((n, 3, 256), dtype=torch.int32, device="cuda")
    luts = torch.full((n, 3, 256), POISON, dtype=torch.uint8, device="cuda")
    picks = [0, 1, n // 2, fc.LINE31 // 3072 - 1, fc.LINE31 // 3072, fc.LINE31 // 3072 + 1, n - 2, n - 1]
    cases = tm.equalize_cases()
    names = ["random", "sparse", "quotient_509"]
    for j, k in enumerate(picks):
        for c in range(3):
            hist[k, c] = cuda(torch, np.asarray(cases[names[(j + c) % 3]], np.uint32).view(np.int32))
    ops = (C.c_int32 * (2 * n))()
    ops[0::2] = [tm.EQUALIZE] * n
    torch.cuda.synchronize()
    rc = importlib.import_module("zune-jpeg_amd").lib().zj_tone_luts_device(ctx.handle, n, 3, ops, hist.data_ptr(), luts.data_ptr(), None)
    assert rc == 0
    ctx.sync()
    for j, k in enumerate(picks):
        got = luts[k].cpu().numpy()
        for c in range(3):
            assert np.array_equal(got[c], tm.table(tm.EQUALIZE, 0, cases[names[(j + c) % 3]])), (k, c)
    ident = torch.arange(256, dtype=torch.uint8, device="cuda")
    assert bool((luts[picks[3] - 7] == ident).all()) and bool((luts[n - 3] == ident).all())   # (empty bins: the identity)


# ---- 6. the plane call and the file-batch call against their stages ------------------------------------------------------------
def frame_ops(n):
    return [ALL_OPS[i % len(ALL_OPS)] for i in range(n)]


@pytest.mark.parametrize("config", [("bilinear", "bf16", "NCHW", 0), ("aa", "u8", "NHWC", 1)], ids=lambda c: "-".join(map(str, c)))
def test_plane_call_equals_its_stages(zj, tz, ctx, torch, synth, config):
    """decode -> zj_color_device -> zj_tone_device -> zj_resize_filtered_device, frame by frame: 4:4:4 .. 4:2:0 frames, a gray
    one shown as RGB, a turned and a prescaled one, every op, with and without a colour matrix in front"""
    import color_model as cm
    import scaled_model as sm
    from test_gpu_color import plane_frames, plane_matrices, resize_u8, u8_image
    from test_gpu_mixed import filled, tdtype
    filt, dtype, layout, crop_layout = config
    chw = bool(crop_layout)
    frames, wins, oris = plane_frames(zj, torch, synth, crop_layout)
    n, size, maxlog = len(frames), (48, 30), 1
    ops = frame_ops(n)
    ms = plane_matrices(tz, n) if crop_layout else None
    flips = [i % 3 == 1 for i in range(n)]
    dt = tdtype(torch, dtype)
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    ks = [sm.prescale_log2(w[2], w[3], size[0], size[1], maxlog) for w in wins]
    assert set(ks) == {0, 1} and 6 in oris and frames[-1].desc.in_components == 1
    raw, out = filled(torch, n, 3, size, dt, layout)
    torch.cuda.synchronize()
    ctx.decode_crops_resized_mixed_device([f.desc for f in frames], [f.ptr(0) for f in frames], [f.ptr(1) for f in frames],
                                          [f.ptr(2) for f in frames], wins, size[0], size[1], tz._resize_dtype(dt),
                                          zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, out.data_ptr(), scale, bias, flips,
                                          None, filt == "aa", 1 << maxlog, oris, "bilinear", colors=ms, tones=ops)
    ctx.sync()
    changed = 0
    for i, f in enumerate(frames):
        img = u8_image(zj, ctx, torch, f, wins[i], oris[i], ks[i], chw)
        if ms is not None:   # the colour stage on the device, as the definition has it
            d = cuda(torch, img)
            h, w = (img.shape[1], img.shape[2]) if chw else (img.shape[0], img.shape[1])
            ctx.color_device([d.data_ptr()], [(w, h)], layout_of(zj, chw), [ms[i]], [d.data_ptr()])
            ctx.sync()
            img = d.cpu().numpy()
        d = cuda(torch, img)
        h, w = (img.shape[1], img.shape[2]) if chw else (img.shape[0], img.shape[1])
        ctx.tone_device([d.data_ptr()], [(w, h)], 3, layout_of(zj, chw), [ops[i]], [d.data_ptr()])
        ctx.sync()
        toned = d.cpu().numpy()
        assert np.array_equal(toned, tm.apply(ops[i][0], ops[i][1], img, chw)), f"frame {i}: zj_tone_device differs from the model"
        want = resize_u8(zj, tz, ctx, torch, toned, chw, size, dt, layout, scale, bias, flips[i], filt == "aa")
        assert torch.equal(out[i].view(torch.uint8), want.view(torch.uint8)), f"frame {i}: differs from resize(tone(colour(u8 image)))"
        changed += not np.array_equal(toned, img)
    assert changed >= 4, "the ops changed too few images"


def test_plane_call_without_tone_is_the_coloured_call_and_gray_outputs_take_an_op(zj, tz, ctx, torch, synth):
    import color_model as cm
    from test_gpu_color import plane_frames, plane_matrices
    from test_gpu_mixed import Frame, filled
    frames, wins, oris = plane_frames(zj, torch, synth, 0)
    n, size = len(frames), (48, 30)
    ms = plane_matrices(tz, n)
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    args = ([f.desc for f in frames], [f.ptr(0) for f in frames], [f.ptr(1) for f in frames], [f.ptr(2) for f in frames], wins,
            size[0], size[1], zj.DTYPE_BF16, zj.TENSOR_NCHW)
    outs = []
    for tones in ("null", None, [None] * n, [(tm.IDENTITY, 0)] * n):
        raw, out = filled(torch, n, 3, size, torch.bfloat16, "NCHW")
        torch.cuda.synchronize()
        if tones == "null":   # the toned entry point itself with a NULL `tone`
            arr = lambda c: (C.c_void_p * n)(*[f.ptr(c) for f in frames])
            colors = (C.c_double * (12 * n))(*[float(v) for m in ms for v in (cm.IDENTITY if m is None else m).reshape(-1)])
            rc = zj.lib().zj_decode_crops_resized_mixed_toned_device(
                ctx.handle, (zj.FrameDesc * n)(*args[0]), n, arr(0), arr(1), arr(2), (C.c_uint * (4 * n))(*[v for w in wins for v in w]),
                size[0], size[1], zj.DTYPE_BF16, zj.TENSOR_NCHW, (C.c_float * 3)(*scale), (C.c_float * 3)(*bias), None,
                zj.RESIZE_BILINEAR, 1, (C.c_uint8 * n)(*oris), colors, None, out.data_ptr(), None)
            assert rc == 0
        else:
            ctx.decode_crops_resized_mixed_device(*args, out.data_ptr(), scale, bias, None, None, False, 2, oris, "bilinear", colors=ms,
                                                  tones=tones)
        ctx.sync()
        outs.append(raw.clone())
    assert not bool((outs[1] == POISON).all())
    for o in outs[:1] + outs[2:]:
        assert torch.equal(o, outs[1])
    # a refused op: nothing is written
    raw, out = filled(torch, n, 3, size, torch.bfloat16, "NCHW")
    torch.cuda.synchronize()
    with pytest.raises(zj.ZjError) as e:
        ctx.decode_crops_resized_mixed_device(*args, out.data_ptr(), scale, bias, None, None, False, 2, oris, "bilinear",
                                              tones=[(tm.INVERT, 0)] * (n - 1) + [(tm.POSTERIZE, 0)])
    assert e.value.status == ERR_ARG
    ctx.sync()
    assert bool((raw == 0xA5).all())
    # GRAYSCALE outputs: one channel under an op; a colour matrix stays unsupported there
    g = zj.ColorSpace.GRAYSCALE
    gf = [Frame(zj, torch, synth, 96, 80, "420", cs=g, seed=41), Frame(zj, torch, synth, 64, 40, "444", cs=g, in_comp=1, seed=40)]
    gw = [(0, 0, 96, 80), (0, 0, 64, 40)]
    res = []
    for tones in (None, [(tm.EQUALIZE, 0), (tm.INVERT, 0)]):
        raw, out = filled(torch, 2, 1, (96, 80), torch.uint8, "NCHW")
        torch.cuda.synchronize()
        ctx.decode_crops_resized_mixed_device([f.desc for f in gf], [f.ptr(0) for f in gf], [f.ptr(1) for f in gf], [f.ptr(2) for f in gf],
                                              gw, 96, 80, zj.DTYPE_U8, zj.TENSOR_NCHW, out.data_ptr(), None, None,
                                              None, None, False, 1, None, "bilinear", tones=tones)
        ctx.sync()
        res.append(out.cpu().numpy())
    plain0 = res[0][0, 0]                                   # (96 x 80 at its own size: the resize is the identity)
    assert np.array_equal(res[1][0, 0], tm.apply(tm.EQUALIZE, 0, plain0))
    with pytest.raises(zj.ZjError) as e:
        ctx.decode_crops_resized_mixed_device([f.desc for f in gf], [f.ptr(0) for f in gf], [f.ptr(1) for f in gf], [f.ptr(2) for f in gf],
                                              gw, 96, 80, zj.DTYPE_U8, zj.TENSOR_NCHW, out.data_ptr(), None, None, None, None, False, 1,
                                              None, "bilinear", colors=[cm.GRAY, cm.IDENTITY], tones=[(tm.INVERT, 0)] * 2)
    assert e.value.status == ERR_UNSUPPORTED


def batch_files(synth, je):
    """(name, blob, even window in displayed pixels, op): a 4:2:0 colour, a gray, a CMYK, a damaged, a 4:1:1 and a turned file
    (test_gpu_color's), four more colour files and one with a refused op.  Every op is on a file that decodes under both
    entropy settings; the windows are even on both axes so that the reduced window of a prescaled file is exactly half of it"""
    from test_gpu_color import colour_files
    from test_gpu_to_tensor import colour_file
    base = dict(colour_files(synth, je))
    return [("colour", base["colour"], (2, 2, 92, 56), (tm.EQUALIZE, 0)),            # 97 x 61: prescaled
            ("gray", base["gray"], (4, 2, 112, 46), (tm.INVERT, 0)),                  # 120 x 50: prescaled
            ("cmyk", base["cmyk"], (2, 2, 96, 70), (tm.EQUALIZE, 0)),                 # 100 x 75: alone, prescaled
            ("damaged", base["damaged"], (0, 0, 8, 8), (tm.SOLARIZE, 128)),
            ("411", base["411"], (2, 2, 96, 70), (tm.SOLARIZE, 128)),                 # alone, never prescaled
            ("turned", base["turned"], (2, 2, 44, 60), (tm.IDENTITY, 0)),             # shown 48 x 64: not prescaled
            ("colour2", colour_file(je, synth, 160, 120, 2, 2, 7), (0, 0, 160, 120), (tm.AUTOCONTRAST, 0)),   # prescaled
            ("colour3", colour_file(je, synth, 80, 64, 1, 2, 8), (2, 2, 40, 30), (tm.POSTERIZE, 2)),          # not prescaled
            ("colour4", colour_file(je, synth, 112, 96, 2, 1, 9), (6, 4, 100, 88), (tm.SOLARIZE, 100)),       # prescaled
            ("colour5", colour_file(je, synth, 64, 48, 2, 2, 10), (0, 0, 64, 48), (tm.IDENTITY, 0)),          # prescaled
            ("refused", base["refused"], (2, 2, 70, 56), (tm.POSTERIZE, 9))]


def file_u8(zj, ctx, torch, blob, opt, win, k):
    """the u8 image the batch call resizes for this file at prescale 2^k: the single-file resized-crop call with the output
    as large as the (reduced) window, where the bilinear resize is the identity"""
    from test_gpu_crop_tensor import GUARD, body, guarded
    x, y, w, h = win
    ow, oh = w >> k, h >> k
    per = 3 * ow * oh
    buf = guarded(torch, per)
    dec = zj.Decoder(opt, ctx)
    try:
        dec.prepare(blob)
        assert dec.finish_pixels_resized_crop_device(x, y, w, h, ow, oh, zj.DTYPE_U8, zj.TENSOR_NHWC, buf.data_ptr() + GUARD, per, None,
                                                     None, False, False, 1 << k, True) == per
    finally:
        dec.close()
    return body(torch, buf, per), ow, oh


@pytest.mark.parametrize("entropy", ["ENTROPY_CPU", "ENTROPY_GPU_ALWAYS"])
def test_batch_of_every_kind(zj, tz, ctx, torch, synth, je, entropy):
    """max_prescale 2 and windows that make six files prescale (the CMYK file, which goes alone, among them): each file's
    image equals resize(zj_tone_device(zj_color_device(its u8 image at the scale the call picks))), every op -- IDENTITY and
    INVERT included -- on a file that decodes, with and without a colour matrix in front"""
    import color_model as cm
    import scaled_model as sm
    from test_gpu_color import resize_u8
    from test_gpu_crop_tensor import layout_code
    from test_gpu_mixed import filled, tdtype
    from test_gpu_to_tensor import options
    files = batch_files(synth, je)
    names = [f[0] for f in files]
    wins, ops = [f[2] for f in files], [f[3] for f in files]
    n, size, maxlog = len(files), (24, 20), 1
    ks = [0 if nm == "411" else sm.prescale_log2(w[2], w[3], size[0], size[1], maxlog) for nm, _, w, _ in files]
    assert [ks[names.index(nm)] for nm in ("colour", "gray", "cmyk", "turned", "colour2", "colour3", "colour4", "colour5")] == [1, 1, 1, 0, 1, 0, 1, 1]
    always = [op for (nm, _, _, op) in files if nm in ("colour", "gray", "turned", "colour2", "colour3", "colour4", "colour5")]
    assert {op[0] for op in always} == {tm.IDENTITY, tm.INVERT, tm.POSTERIZE, tm.SOLARIZE, tm.AUTOCONTRAST, tm.EQUALIZE}
    opt = options(zj, entropy)
    ms = [tz.color_matrix(contrast=0.8, saturation=0.7), None, cm.BGR, None, None, tz.color_matrix(brightness=0.6), None,
          tz.color_matrix(1.2, 1.1, 0.5), None, cm.NEGATIVE, None]
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    alone_ok = entropy == "ENTROPY_CPU"
    for dtype, layout, filt in (("bf16", "NCHW", "bilinear"), ("u8", "NHWC", "aa")):
        dt = tdtype(torch, dtype)
        decs, prepared = [], []
        for nm, b, _, _ in files:
            dec = zj.Decoder(opt, ctx)
            try:
                dec.prepare(b)
                prepared.append(True)
            except zj.ZjError:
                assert nm == "damaged" or (not alone_ok and nm in ("cmyk", "411")), (nm, entropy)
                prepared.append(False)
            decs.append(dec)
        flips = [k % 2 == 1 for k in range(n)]
        raw, out = filled(torch, n, 3, size, dt, layout)
        torch.cuda.synchronize()
        try:
            rcs = zj.finish_pixels_resized_crop_batch(decs, ctx, wins, size[0], size[1], tz._resize_dtype(dt), layout_code(zj, layout),
                                                      out.data_ptr(), raw.numel(), scale, bias, flips, filt == "aa", 1 << maxlog, True,
                                                      "bilinear", colors=ms, tones=ops)
            texts = [zj.lib().zj_decoder_error(d._d).decode(errors="replace") for d in decs]
        finally:
            for d in decs:
                d.close()
        ctx.sync()
        img_bytes = raw.numel() // n
        checked = []
        for k, (nm, b, w, op) in enumerate(files):
            slot = raw[k * img_bytes:(k + 1) * img_bytes]
            if nm == "refused":
                assert rcs[k] == ERR_ARG and "tone" in texts[k] and bool((slot == 0xA5).all())
                continue
            if not prepared[k]:
                assert rcs[k] != 0 and bool((slot == 0xA5).all()), (nm, rcs)
                continue
            assert rcs[k] == 0, (nm, rcs[k], texts[k])
            u8, uw, uh = file_u8(zj, ctx, torch, b, opt, w, ks[k])
            d = u8.reshape(-1).clone()
            if ms[k] is not None:
                ctx.color_device([d.data_ptr()], [(uw, uh)], zj.LAYOUT_HWC, [ms[k]], [d.data_ptr()])
            ctx.tone_device([d.data_ptr()], [(uw, uh)], 3, zj.LAYOUT_HWC, [op], [d.data_ptr()])
            ctx.sync()
            toned = d.cpu().numpy().reshape(uh, uw, 3)
            plain = cm.apply(cm.IDENTITY if ms[k] is None else ms[k], u8.cpu().numpy().reshape(uh, uw, 3))
            assert np.array_equal(toned, tm.apply(op[0], op[1], plain)), nm
            want = resize_u8(zj, tz, ctx, torch, toned, False, size, dt, layout, scale, bias, flips[k], filt == "aa")
            assert torch.equal(out[k].view(torch.uint8).reshape(-1), want.view(torch.uint8).reshape(-1)), (nm, dtype, layout, ks[k])
            checked.append(nm)
        assert set(checked) >= {"colour", "gray", "turned", "colour2", "colour3", "colour4", "colour5"}
        if alone_ok:
            assert [rc == 0 for rc in rcs] == [True, True, True, False, True, True, True, True, True, True, False], rcs
            assert "cmyk" in checked and "411" in checked


def test_batch_without_tone_is_the_coloured_batch_call(zj, tz, ctx, torch, synth, je):
    from test_gpu_mixed import filled
    from test_gpu_to_tensor import options
    files = [f for f in batch_files(synth, je) if f[0] not in ("damaged", "refused")]
    blobs = [f[1] for f in files]
    n = len(blobs)
    ms = [tz.color_matrix(contrast=0.8, saturation=0.7)] * n
    kw = dict(dtype=torch.bfloat16, layout="NHWC", mean=MEAN, std=STD, apply_orientation=True, options=options(zj), max_prescale=2)
    plain = tz.decode_files_resized_to_tensor(ctx, blobs, None, (24, 16), color=ms, **kw)
    ident = tz.decode_files_resized_to_tensor(ctx, blobs, None, (24, 16), color=ms, tone=[None] * n, **kw)
    toned = tz.decode_files_resized_to_tensor(ctx, blobs, None, (24, 16), color=ms, tone=[tz.tone_op("invert")] * n, **kw)
    torch.cuda.synchronize()
    assert torch.equal(plain.view(torch.uint8), ident.view(torch.uint8))
    assert not torch.equal(plain.view(torch.uint8), toned.view(torch.uint8))
    # the toned entry point itself with a NULL `tone`, called through ctypes: the coloured batch call's bytes and statuses
    wins = [f[2] for f in files]
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    colors = (C.c_double * (12 * n))(*[float(v) for m in ms for v in np.asarray(m).reshape(-1)])
    res = []
    for entry in ("zj_decoder_finish_pixels_resized_crop_batch_toned_device", "zj_decoder_finish_pixels_resized_crop_batch_colored_device"):
        decs = [zj.Decoder(options(zj), ctx) for _ in blobs]
        raw, out = filled(torch, n, 3, (24, 20), torch.bfloat16, "NCHW")
        torch.cuda.synchronize()
        try:
            for d, b in zip(decs, blobs):
                d.prepare(b)
            rcs = (C.c_int * n)(*([7] * n))
            args = [(C.c_void_p * n)(*[d._d for d in decs]), n, ctx.handle, (C.c_uint * (4 * n))(*[v for w in wins for v in w]), 24, 20,
                    zj.DTYPE_BF16, zj.TENSOR_NCHW, (C.c_float * 3)(*scale), (C.c_float * 3)(*bias), None, zj.RESIZE_BILINEAR, 1, 1, colors]
            if "toned" in entry:
                args.append(None)
            assert getattr(zj.lib(), entry)(*args, out.data_ptr(), raw.numel(), rcs) == 0
        finally:
            for d in decs:
                d.close()
        ctx.sync()
        res.append((list(rcs), raw.clone()))
    assert res[0][0] == res[1][0] == [0] * n
    assert torch.equal(res[0][1], res[1][1]) and not bool((res[0][1] == 0xA5).all())


# ---- 7. the wrappers -----------------------------------------------------------------------------------------------------------
def test_the_stage_wrappers(zj, tz, ctx, torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    rnd = lambda *shape: torch.randint(20, 230, shape, dtype=torch.uint8, device="cuda", generator=g)
    ops = [tz.tone_op("equalize"), None, tz.tone_op("posterize", 3), tz.tone_op("autocontrast")]
    pairs = [(tm.IDENTITY, 0) if o is None else o for o in ops]
    for layout in ("HWC", "CHW"):
        chw = layout == "CHW"
        sizes = ((17, 9), (130, 3), (1, 1))
        imgs = [rnd(3, h, w) if chw else rnd(h, w, 3) for w, h in sizes]
        wide = rnd(3, 9, 40) if chw else rnd(9, 40, 3)      # (the last image's rows at a pitch of 40 pixels)
        imgs.append(wide[:, :, 3:36] if chw else wide[:, 3:36])
        before = [im.cpu().numpy() for im in imgs]
        hist = tz.histogram_tensor(ctx, imgs, layout)
        outs = tz.tone_tensor(ctx, imgs, ops, layout)
        lut = tz.lut_tensor(ctx, imgs, tz.gamma_lut(2.2), layout)
        torch.cuda.synchronize()
        gl = tz.gamma_lut(2.2)
        assert gl.shape == (3, 256) and gl.dtype == np.uint8 and gl[0, 0] == 0 and gl[0, 255] == 255
        assert list(gl[1, :4]) == [min(255, int(255 * (i / 255) ** 2.2 + 0.5)) for i in range(4)]
        for i, (a, (op, param)) in enumerate(zip(before, pairs)):
            assert np.array_equal(hist[i].cpu().numpy(), tm.histogram(a, chw))
            assert outs[i].is_contiguous() and np.array_equal(outs[i].cpu().numpy(), tm.apply(op, param, a, chw))
            assert np.array_equal(lut[i].cpu().numpy(), tm.apply_luts(a, gl, chw))
        same = tz.tone_tensor(ctx, imgs, ops, layout, inplace=True)
        torch.cuda.synchronize()
        for a, (op, param), o, im in zip(before, pairs, same, imgs):
            assert o is im and np.array_equal(im.cpu().numpy(), tm.apply(op, param, a, chw))
    gray = rnd(21, 33)
    out = tz.tone_tensor(ctx, [gray], [tz.tone_op("equalize")])
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy().reshape(21, 33), tm.apply(tm.EQUALIZE, 0, gray.cpu().numpy()))
    with pytest.raises(ValueError):
        tz.tone_op("posterize", 9)
    with pytest.raises(ValueError):
        tz.tone_tensor(ctx, [gray], [])


def test_tone_on_both_resized_crop_wrappers_equals_the_stages(zj, tz, ctx, torch, synth, je):
    """tone= on decode_files_resized_to_tensor and decode_resized_crops_to_tensor equals the wrapper without it at the crop's
    own size in u8, followed by tone_tensor and resize_to_tensor"""
    from test_gpu_mixed import Frame
    from test_gpu_to_tensor import colour_file, gray_file, options
    ops = [tz.tone_op("equalize"), tz.tone_op("autocontrast"), tz.tone_op("solarize", 77)]
    blobs = [gray_file(je, synth), colour_file(je, synth, 97, 61, 2, 2, 4), colour_file(je, synth, 64, 48, 2, 2, 5, orientation=6)]
    kw = dict(layout="NHWC", apply_orientation=True, options=options(zj))
    got = tz.decode_files_resized_to_tensor(ctx, blobs, None, (33, 21), dtype=torch.bfloat16, mean=MEAN, std=STD, tone=ops, **kw)
    torch.cuda.synchronize()
    for i, b in enumerate(blobs):
        info = zj.Decoder(options(zj), ctx)
        try:
            hdr = info.prepare(b)[1]
            turned = info.orientation in (5, 6, 7, 8)
        finally:
            info.close()
        w, h = (int(hdr.height), int(hdr.width)) if turned else (int(hdr.width), int(hdr.height))
        u8 = tz.decode_files_resized_to_tensor(ctx, [b], None, (w, h), dtype=torch.uint8, **kw)[0]
        toned = tz.tone_tensor(ctx, [u8], [ops[i]])
        want = tz.resize_to_tensor(ctx, toned, (33, 21), dtype=torch.bfloat16, layout="NHWC", mean=MEAN, std=STD)
        torch.cuda.synchronize()
        assert torch.equal(got[i].view(torch.uint8), want[0].view(torch.uint8)), i
    # frames of one geometry
    f = [Frame(zj, torch, synth, 96, 80, "420", seed=50 + i, quality=80) for i in range(3)]
    frames = [tuple(x.planes) for x in f]
    wins = [(3, 5, 70, 50), (0, 0, 96, 80), (11, 2, 85, 77)]
    got = tz.decode_resized_crops_to_tensor(ctx, f[0].desc, frames, wins, (33, 21), dtype=torch.bfloat16, layout="NHWC", mean=MEAN, std=STD,
                                            tone=ops)
    torch.cuda.synchronize()
    for i in range(3):
        u8 = tz.decode_resized_crops_to_tensor(ctx, f[0].desc, frames[i:i + 1], wins[i:i + 1], (wins[i][2], wins[i][3]), dtype=torch.uint8,
                                               layout="NHWC")[0]
        toned = tz.tone_tensor(ctx, [u8], [ops[i]])
        want = tz.resize_to_tensor(ctx, toned, (33, 21), dtype=torch.bfloat16, layout="NHWC", mean=MEAN, std=STD)
        torch.cuda.synchronize()
        assert torch.equal(got[i].view(torch.uint8), want[0].view(torch.uint8)), i
    with pytest.raises(ValueError):
        tz.decode_resized_crops_to_tensor(ctx, f[0].desc, frames, wins, (33, 21), tone=ops[:2])
