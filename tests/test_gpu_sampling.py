"""GPU: three-component JPEGs of odd samplings and stored-RGB files as RGB resized crops on an MI355X
(ZJ_FLAG_ANY_SAMPLING).
1. zj_planes_to_rgb_device against numpy (box replication, the oracle's colour arithmetic) over the size / pitch / alignment /
   ratio matrix of tests/planes_cases.py, sentinels around every output, guard bytes behind every plane; argument errors
   launch nothing.
2. Files: the single-file call equals the MODEL bit for bit -- the planes zj_decoder_plane gives through clamped IDCT,
   replication and colour in numpy (tests/sampling_cases.py), then zj_orient_device and zj_resize_filtered_device.
3. A Pillow keep_rgb=True file against Pillow's RGB.
4. The batch call with such files between standard, gray and CMYK files.
5. The status codes.
Every comparison but 3 is torch.equal / np.array_equal on bytes."""
import ctypes as C
import importlib
import io

import numpy as np
import pytest

import cmyk_cases as cc
import orient_model as om
import planes_cases as pc
import sampling_cases as sc

pytestmark = pytest.mark.gpu
FILL = 0xA5
ERR_ARG, ERR_UNSUPPORTED, ERR_FORMAT = -1, -2, -20
FILTERS = {"bilinear": (False, "bilinear"), "aa": (True, "bilinear"), "bicubic": (True, "bicubic")}
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


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


def test_the_status_values(zj):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zjhip.h")).read()
    st = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ZJ_ERR_\w+)\s*=\s*(-?\d+)", hdr)}
    assert (st["ZJ_ERR_ARG"], st["ZJ_ERR_UNSUPPORTED"], st["ZJ_ERR_FORMAT"]) == (ERR_ARG, ERR_UNSUPPORTED, ERR_FORMAT)


# ---- 1. the stage by itself -------------------------------------------------------------------------------------------
def aligned_cuda(torch, n):
    """n bytes of device memory that start on a 16-byte boundary"""
    t = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    off = (-t.data_ptr()) % 16
    return t[off:off + n]


def stage_call(zj, ctx, torch, rng, cases, chw, stored_rgb):
    lay = pc.Layout(rng, cases, chw, stored_rgb)
    src = aligned_cuda(torch, lay.src.size)
    src.copy_(torch.from_numpy(lay.src))
    arena = aligned_cuda(torch, lay.arena_len)
    arena.fill_(pc.SENTINEL)
    torch.cuda.synchronize()
    base = src.data_ptr()
    ctx.planes_to_rgb_device([base + o[0] for o in lay.p_off], [base + o[1] for o in lay.p_off], [base + o[2] for o in lay.p_off],
                             lay.sizes, [tuple((g[0], g[1]) for g in geo) for geo in lay.geos],
                             zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, [arena.data_ptr() + o for o in lay.out_off], stored_rgb,
                             lay.p_pitch, lay.out_pitch)
    ctx.sync()
    got = arena.cpu().numpy()
    assert np.array_equal(got[lay.inside], lay.want[lay.inside]), "an image differs from the replicated, converted planes"
    assert (got[~lay.inside] == pc.SENTINEL).all(), "a padding or guard byte was written"
    assert np.array_equal(src.cpu().numpy(), lay.src), "an input was written"


@pytest.mark.parametrize("stored_rgb", [False, True], ids=["ycbcr", "stored_rgb"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_over_the_size_pitch_alignment_and_ratio_matrix(zj, ctx, torch, chw, stored_rgb):
    """1152 images in one call (16 launches): every width, height, pitch and base of the matrix, every ratio pair in every
    component (the public stage starts every plane at phase 0; the phases run in the emulation and in the file tests)"""
    stage_call(zj, ctx, torch, np.random.default_rng(43 + chw + 2 * stored_rgb), pc.matrix(phases=False), chw, stored_rgb)


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_129_images_of_mixed_sizes(zj, ctx, torch, chw):
    rng = np.random.default_rng(89 + chw)
    stage_call(zj, ctx, torch, rng, pc.mixed_129(rng, phases=False), chw, bool(chw))


def test_stage_tight_pitches_by_default_and_the_tensor_wrapper(zj, tz, ctx, torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    sizes = ((17, 9), (130, 3), (1, 1), (33, 9))
    ratios = (((1, 1), (4, 1), (4, 1)), ((1, 1), (2, 2), (2, 2)), ((4, 4), (1, 1), (2, 1)), ((1, 1), (4, 2), (1, 4)))
    planes = []
    for (w, h), rs in zip(sizes, ratios):
        planes.append([rnd(-(-h // ry), -(-w // rx)) for rx, ry in rs])
    planes[3][0] = rnd(9, 40)[:, 3:36]  # (the last image's first plane: rows at a pitch of 40)
    for layout in ("HWC", "CHW"):
        for stored in (False, True):
            outs = tz.planes_to_rgb_tensor(ctx, planes, sizes, ratios, layout, stored)
            torch.cuda.synchronize()
            for trio, (w, h), rs, o in zip(planes, sizes, ratios, outs):
                want = pc.combine([p.cpu().numpy() for p in trio], [(rx, ry, 0, 0) for rx, ry in rs], w, h, stored)
                got = o.cpu().numpy()
                assert o.is_contiguous() and np.array_equal(got.transpose(1, 2, 0) if layout == "CHW" else got, want)


def test_stage_argument_errors_launch_nothing(zj, ctx, torch):
    p = torch.full((256,), 128, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = zj.lib()

    def call(n, p0, p1, p2, wh, ratios, pitches, stored, layout, outs, op):
        arr = lambda v: (C.c_void_p * len(v))(*v) if v is not None else None
        u = lambda v: (C.c_uint * len(v))(*v) if v is not None else None
        b = (C.c_uint8 * len(ratios))(*ratios) if ratios is not None else None
        return L.zj_planes_to_rgb_device(ctx.handle, n, arr(p0), arr(p1), arr(p2), u(wh), b, u(pitches), stored, layout, arr(outs), u(op), None)

    a, o = p.data_ptr(), dst.data_ptr()
    ones = [1] * 6
    assert call(1, [a], [a], [a], [4, 4], [3, 1, 1, 1, 1, 1], None, 0, 0, [o], None) == ERR_ARG    # a ratio of 3
    assert call(1, [a], [a], [a], [4, 4], [1, 1, 1, 8, 1, 1], None, 0, 0, [o], None) == ERR_ARG    # ... of 8
    assert call(1, [a], [a], [a], [4, 4], [1, 1, 1, 1, 1, 0], None, 0, 0, [o], None) == ERR_ARG    # ... of 0
    assert call(2, [a, a], [a, a], [a, a], [4, 4, 0, 4], ones * 2, None, 0, 0, [o, o + 64], None) == ERR_ARG  # an empty image
    assert call(1, [a], [a], [a], [4, 4], ones, [4, 3, 4], 0, 0, [o], None) == ERR_ARG             # a pitch below a row
    assert call(1, [a], [a], [a], [8, 4], [1, 1, 4, 1, 4, 1], [8, 1, 2], 0, 0, [o], None) == ERR_ARG  # ... below ceil(8 / 4)
    assert call(1, [a], [a], [a], [4, 4], ones, None, 0, 0, [o], [11]) == ERR_ARG
    assert call(1, [a], [a], [a], [4, 4], ones, None, 0, 1, [o], [3]) == ERR_ARG
    assert call(1, [a], [a], [a], [4, 4], ones, None, 0, 2, [o], None) == ERR_ARG                  # not a layout
    assert call(1, [a], [a], [a], [65536, 1], ones, None, 0, 0, [o], None) == ERR_ARG
    assert call(1, [a], [None], [a], [4, 4], ones, None, 0, 0, [o], None) == ERR_ARG
    assert call(1, [a], [a], [a], [4, 4], None, None, 0, 0, [o], None) == ERR_ARG
    assert call(0, [a], [a], [a], [4, 4], ones, None, 0, 0, [o], None) == ERR_ARG
    ctx.sync()
    assert bool((dst == FILL).all())
    assert call(1, [a], [a], [a], [4, 4], [4, 4, 2, 1, 1, 2], None, 0, 0, [o], None) == 0  # gray 128 stays gray
    ctx.sync()
    assert bool((dst[:48] == 128).all()) and bool((dst[48:] == FILL).all())


# ---- 2. files against the model -----------------------------------------------------------------------------------------
def options(zj, flags=None, layout=0, entropy="ENTROPY_CPU", cs=None):
    o = zj.ZuneJpegOptions()
    o.flags = zj.FLAG_ANY_SAMPLING if flags is None else flags
    o.out_layout = layout
    o.entropy = getattr(zj, entropy)
    if cs is not None:
        o.out_colorspace = cs
    return o


def tdtype(torch, name):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}[name]


def odd_file(synth, w, h, samp, seed, progressive=False, restart=0, orientation=None, **kw):
    planes = sc.small_planes(w, h, samp, seed=seed, amp=12, dc=120)
    data = sc.encode(planes, synth.quant_tables(60 + seed % 30), w, h, samp, progressive=progressive, restart=restart, **kw)
    return om.splice(data, om.exif_segment(orientation)) if orientation else data


def single_file(zj, tz, ctx, torch, blob, opt, win, size, dt, layout, flip=False, filt="bilinear", max_prescale=1, mean=MEAN, std=STD):
    dec = zj.Decoder(opt, ctx)
    _, info = dec.prepare(blob)
    if win is None:
        win = (0, 0) + tuple(zj.oriented_size(dec.orientation, int(info.width), int(info.height)))
    ow, oh = size
    raw = torch.full((3 * oh * ow * torch.empty((), dtype=dt).element_size(),), FILL, dtype=torch.uint8, device="cuda")
    one = raw.view(dt).view((3, oh, ow) if layout == "NCHW" else (oh, ow, 3))
    scale, bias = tz.normalize_factors(3, mean, std)
    torch.cuda.synchronize()
    try:
        n = dec.finish_pixels_resized_crop_device(win[0], win[1], win[2], win[3], ow, oh, tz._resize_dtype(dt),
                                                  zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, one.data_ptr(),
                                                  raw.numel(), scale, bias, flip, FILTERS[filt][0], max_prescale, True, FILTERS[filt][1])
    finally:
        dec.close()
    assert n == raw.numel(), "*out_len is not the slot's size"
    return one


def model_e(zj, blob, win):
    """E of the definition in numpy, over the stored window of the displayed window `win` (None: all): (E, orientation)"""
    # (ZJ_FLAG_FULL_AC_VALUES: a standard file's coefficients as coded too; the serial walk of the others never cuts them)
    dec = zj.Decoder(options(zj, zj.FLAG_ANY_SAMPLING | zj.FLAG_FULL_AC_VALUES))
    _, info = dec.prepare(blob)
    assert info.components == 3
    w, h, o = int(info.width), int(info.height), dec.orientation
    samp = tuple(dec.component_sampling(c) for c in range(3))
    kept = [dec.plane(c) for c in range(3)]
    for c in range(3):
        cw, ch = sc.comp_size(w, h, samp, c)
        assert kept[c].shape[:2] == (-(-ch // 8), -(-cw // 8))
    stored = dec.stored_rgb
    dec.close()
    qt, tqs = cc.file_tables(blob)
    if win is None:
        win = (0, 0) + tuple(om.oriented_size(o, w, h))
    st = om.stored_window(o, w, h, win)
    return sc.model_image(kept, [qt[t] for t in tqs], samp, st[0], st[1], st[2], st[3], stored), o


def model(zj, tz, ctx, torch, blob, win, size, dt, layout, flip, filt, chw=False):
    e, o = model_e(zj, blob, win)
    h, w = e.shape[:2]
    lay = zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC
    src = torch.from_numpy(np.ascontiguousarray(e.transpose(2, 0, 1) if chw else e)).cuda()
    dw, dh = om.oriented_size(o, w, h)
    shown = torch.empty((3, dh, dw) if chw else (dh, dw, 3), dtype=torch.uint8, device="cuda")
    ow, oh = size
    one = torch.full((3, oh, ow) if layout == "NCHW" else (oh, ow, 3), 0, dtype=dt, device="cuda")
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    torch.cuda.synchronize()
    ctx.orient_device([src.data_ptr()], [(w, h)], 3, lay, [o], [shown.data_ptr()])
    ctx.resize_device([shown.data_ptr()], [(dw, dh)], 3, lay, ow, oh, tz._resize_dtype(dt),
                      zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, one.data_ptr(), scale, bias, [flip], None, None,
                      FILTERS[filt][0], FILTERS[filt][1])
    ctx.sync()
    return one


# the four sizes x the sampling list; the other choices turn with the case's number so that every value of each meets every
# sampling and every size: progressive, filter, dtype, tensor layout, orientation, flip, crop layout, window
def file_cases():
    cases = []
    for i, samp in enumerate(sc.SAMPLINGS):
        for j, (w, h) in enumerate(sc.SIZES):
            n = 4 * i + j
            o = (1, 2, 6)[(i + j) % 3]
            dw, dh = om.oriented_size(o, w, h)
            win = None if n % 2 == 0 else (1 + n % 3, n % 4, dw - 4 - n % 5, dh - 3 - n % 3)
            cases.append((samp, (w, h), bool((i + j) % 2), ("bilinear", "aa", "bicubic")[(i + 2 * j) % 3], ("u8", "bf16", "f32")[(2 * i + j) % 3],
                          ("NCHW", "NHWC")[(i // 2 + j) % 2], o, bool((i + j // 2) % 2), (i + j // 2 + 1) % 2, win, ((12, 9), (7, 5))[n % 2]))
    return cases


@pytest.mark.parametrize("case", file_cases(), ids=lambda c: f"{sc.name(c[0])}-{c[1][0]}x{c[1][1]}-{'p' if c[2] else 'b'}-{c[3]}-{c[4]}-{c[5]}-o{c[6]}")
def test_single_file_call_equals_the_model(zj, tz, ctx, torch, synth, case):
    samp, (w, h), prog, filt, dtype, layout, o, flip, crop_layout, win, size = case
    blob = odd_file(synth, w, h, samp, seed=w + 3 * o + samp[0][0], progressive=prog, restart=0 if (w + o) % 2 else 3,
                    orientation=o if o != 1 else None, ids=(1, 2, 3) if w % 2 else (9, 8, 7))
    dt = tdtype(torch, dtype)
    want = model(zj, tz, ctx, torch, blob, win, size, dt, layout, flip, filt, bool(crop_layout))
    for max_prescale in (1, 8):  # (such a file is never prescaled: the same bytes)
        got = single_file(zj, tz, ctx, torch, blob, options(zj, layout=crop_layout), win, size, dt, layout, flip, filt, max_prescale)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), f"max_prescale {max_prescale}"
    # the device entropy options leave such a file to the CPU walk: the same bytes
    for entropy in ("ENTROPY_GPU", "ENTROPY_GPU_ALWAYS"):
        dev = single_file(zj, tz, ctx, torch, blob, options(zj, layout=crop_layout, entropy=entropy), win, size, dt, layout, flip, filt, 8)
        assert torch.equal(dev.view(torch.uint8), want.view(torch.uint8)), entropy


def test_what_the_cases_reach():
    cs = file_cases()
    assert len(cs) == 28
    for k, values in ((2, {False, True}), (3, set(FILTERS)), (4, {"u8", "bf16", "f32"}), (5, {"NCHW", "NHWC"}), (6, {1, 2, 6}),
                      (7, {False, True}), (8, {0, 1})):
        assert {c[k] for c in cs} == values, k
        for samp in sc.SAMPLINGS:
            assert len({c[k] for c in cs if c[0] == samp}) >= 2, (k, samp)


@pytest.mark.parametrize("samp", [sc.SAMPLINGS[0], sc.SAMPLINGS[1], sc.SAMPLINGS[2], sc.SAMPLINGS[6]], ids=sc.name)
def test_windows_that_start_at_every_phase(zj, tz, ctx, torch, synth, samp):
    """16 windows of one file: x and y 0..3 past a multiple of 4, widths and heights that end at every phase too"""
    w, h = 48, 40
    blob = odd_file(synth, w, h, samp, seed=11, progressive=samp[0] == (4, 2))
    for x in range(4):
        for y in range(4):
            win = (4 + x, 8 + y, 17 + (x + y) % 4, 9 + (2 * x + y) % 4)
            want = model(zj, tz, ctx, torch, blob, win, (9, 6), torch.uint8, "NHWC", False, "bilinear")
            got = single_file(zj, tz, ctx, torch, blob, options(zj), win, (9, 6), torch.uint8, "NHWC")
            assert torch.equal(got, want), win


@pytest.mark.parametrize("kind", ["ids", "stored_rgb", "stored_rgb_420"])
def test_standard_samplings_that_are_non_standard_files(zj, tz, ctx, torch, synth, kind):
    """ids outside 1..3 on a 4:2:0 file; stored RGB (Adobe transform 0) at 4:4:4 and, odd as it is, at 4:2:0"""
    samp = sc.STANDARD[0] if kind == "stored_rgb" else sc.STANDARD[3]
    kw = dict(ids=(4, 5, 6)) if kind == "ids" else dict(adobe=0, ids=tuple(b"RGB"), jfif=False)
    blob = odd_file(synth, 100, 75, samp, seed=2, restart=2, **kw)
    for chw in (0, 1):
        want = model(zj, tz, ctx, torch, blob, (3, 2, 90, 70), (12, 9), torch.float32, "NCHW", True, "aa", bool(chw))
        got = single_file(zj, tz, ctx, torch, blob, options(zj, layout=chw), (3, 2, 90, 70), (12, 9), torch.float32, "NCHW", True, "aa", 8)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def test_a_standard_file_keeps_its_bytes_under_the_flag(zj, tz, ctx, torch, synth):
    for samp in sc.STANDARD:
        blob = odd_file(synth, 100, 75, samp, seed=3, adobe=1 if samp == sc.STANDARD[1] else None)
        for entropy in ("ENTROPY_CPU", "ENTROPY_GPU_ALWAYS"):
            a = single_file(zj, tz, ctx, torch, blob, options(zj, 0, entropy=entropy), None, (16, 12), torch.uint8, "NHWC", max_prescale=4)
            b = single_file(zj, tz, ctx, torch, blob, options(zj, entropy=entropy), None, (16, 12), torch.uint8, "NHWC", max_prescale=4)
            assert torch.equal(a, b), (samp, entropy)


# ---- 3. Pillow's stored-RGB files against Pillow --------------------------------------------------------------------------
def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 3 + yy * 2 + seed * 17) % 256, (xx * yy // 7 + 40 * seed) % 256, (255 - xx - 2 * yy) % 256], -1)
    return (img + rng.integers(0, 24, img.shape)).clip(0, 255).astype(np.uint8)


def pillow_file(w, h, seed, gray=False, progressive=False, orientation=None, quality=85, **save):
    from PIL import Image
    img = picture(w, h, seed)
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if gray else img).save(buf, "JPEG", quality=quality, progressive=progressive, **save)
    data = buf.getvalue()
    return om.splice(data, om.exif_segment(orientation)) if orientation else data


@pytest.mark.parametrize("quality,progressive,wh", [(75, False, (64, 48)), (95, True, (100, 75)), (90, False, (33, 17))])
def test_a_pillow_stored_rgb_file_against_pillow(zj, tz, ctx, torch, quality, progressive, wh):
    """|ours - Pillow| <= the largest difference between the MODEL of the ordinary 4:4:4 file of the same picture and Pillow's
    decode of that file, measured here, plus 1 (tests/test_sampling_model.py has the reasoning)"""
    from PIL import Image
    w, h = wh
    plain = pillow_file(w, h, quality, progressive=progressive, quality=quality, subsampling="4:4:4")
    e, _ = model_e(zj, plain, None)
    bound = int(np.abs(e.astype(np.int32) - np.asarray(Image.open(io.BytesIO(plain)).convert("RGB")).astype(np.int32)).max()) + 1
    blob = pillow_file(w, h, quality, progressive=progressive, quality=quality, keep_rgb=True)
    rgb = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB")).astype(np.int32)
    ours = single_file(zj, tz, ctx, torch, blob, options(zj), None, (w, h), torch.uint8, "NHWC", mean=None, std=None)
    worst = int(np.abs(ours.cpu().numpy().astype(np.int32) - rgb).max())
    print(f"pillow keep_rgb q{quality} {'progressive' if progressive else 'baseline'} {w}x{h}: bound {bound} largest |ours - Pillow| {worst}")
    assert worst <= bound


# ---- 4. the batch call ------------------------------------------------------------------------------------------------------
def pillow_cmyk(w, h, seed, **save):
    from PIL import Image
    img = np.concatenate([picture(w, h, seed), picture(w, h, seed + 1)[..., :1] // 2], axis=2)
    buf = io.BytesIO()
    Image.fromarray(img, "CMYK").save(buf, "JPEG", **save)
    return buf.getvalue()


def mixed_files(synth):
    """(blob, non-standard): odd-sampled and stored-RGB files between colour, gray and CMYK files"""
    return [(pillow_file(96, 72, 1), False), (odd_file(synth, 100, 75, sc.SAMPLINGS[0], 21), True),
            (pillow_file(80, 56, 2, gray=True), False), (pillow_cmyk(64, 48, 3, quality=85), False),
            (odd_file(synth, 48, 40, sc.SAMPLINGS[3], 22, progressive=True, orientation=6), True),
            (pillow_file(97, 61, 3, subsampling="4:4:4", orientation=6), False),
            (pillow_file(80, 64, 4, keep_rgb=True), True), (odd_file(synth, 33, 17, sc.SAMPLINGS[1], 23, restart=2), True),
            (pillow_file(64, 48, 6, progressive=True), False)]


@pytest.mark.parametrize("workers", [1, 4])
def test_odd_files_between_standard_gray_and_cmyk_files(zj, tz, ctx, torch, synth, workers):
    files = mixed_files(synth)
    blobs = [b for b, _ in files]
    rest_flags = zj.FLAG_GRAY_TO_RGB | zj.FLAG_CMYK_TO_RGB
    size = (16, 12)
    wins = [None, (3, 5, 40, 30), None, None, (2, 1, 30, 40), None, (1, 1, 70, 60), None, None]
    flips = [k % 3 == 1 for k in range(len(blobs))]
    for dt, layout, filt, max_prescale in ((torch.uint8, "NHWC", "bilinear", 1), (torch.float32, "NCHW", "aa", 4)):
        kw = dict(dtype=dt, layout=layout, antialias=FILTERS[filt][0], max_prescale=max_prescale, apply_orientation=True,
                  workers=workers, mean=MEAN, std=STD)
        out = tz.decode_files_resized_to_tensor(ctx, blobs, wins, size, flips=flips, options=options(zj, rest_flags | zj.FLAG_ANY_SAMPLING), **kw)
        torch.cuda.synchronize()
        for k, (blob, odd) in enumerate(files):
            if odd:
                want = model(zj, tz, ctx, torch, blob, wins[k], size, dt, layout, flips[k], filt)
                assert torch.equal(out[k].view(torch.uint8), want.view(torch.uint8)), f"file {k} differs from the model"
        # the other files: what the same call gives without the odd files, and without their flag
        rest = [k for k, (_, odd) in enumerate(files) if not odd]
        pick = lambda v: [v[k] for k in rest]
        alone = tz.decode_files_resized_to_tensor(ctx, pick(blobs), pick(wins), size, flips=pick(flips), options=options(zj, rest_flags), **kw)
        torch.cuda.synchronize()
        assert torch.equal(out[rest].view(torch.uint8), alone.view(torch.uint8)), "a file changed beside odd-sampled files"


def test_without_the_flag_the_batch_names_the_file(zj, tz, ctx, torch, synth):
    blobs = [b for b, _ in mixed_files(synth)[:3]]
    with pytest.raises(zj.DecodeError) as e:
        tz.decode_files_resized_to_tensor(ctx, blobs, None, (8, 8), dtype=torch.uint8, options=options(zj, zj.FLAG_GRAY_TO_RGB))
    assert e.value.status == ERR_FORMAT and e.value.text == "file 1: Unknown down-sampling method, cannot continue"


# ---- 5. status codes ----------------------------------------------------------------------------------------------------------
def test_status_codes(zj, tz, ctx, torch, synth):
    blob = odd_file(synth, 48, 40, sc.SAMPLINGS[1], 5)
    raw = torch.full((3 * 48 * 40 * 4,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    resized = lambda dec, win=(0, 0, 48, 40), cap=3 * 64 * 4: dec.finish_pixels_resized_crop_device(
        win[0], win[1], win[2], win[3], 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, raw.data_ptr(), cap)
    # a decoder that asks for GRAYSCALE or YCbCr
    for cs in (zj.ColorSpace.GRAYSCALE, zj.ColorSpace.YCbCr):
        dec = zj.Decoder(options(zj, cs=cs), ctx)
        dec.prepare(blob)
        with pytest.raises(zj.DecodeError) as e:
            resized(dec)
        assert e.value.status == ERR_UNSUPPORTED and "ZJ_CS_RGB" in e.value.text
        dec.close()
    # every finish call outside the resized-crop family
    calls = [lambda d: d.finish_pixels(), lambda d: d.finish_pixels_device(raw.data_ptr(), raw.numel()),
             lambda d: d.finish_pixels_device(raw.data_ptr(), raw.numel(), True),
             lambda d: d.finish_pixels_crop_device(0, 0, 16, 16, raw.data_ptr(), raw.numel()),
             lambda d: d.finish_pixels_scaled_device(2, raw.data_ptr(), raw.numel())]
    for call in calls:
        dec = zj.Decoder(options(zj), ctx)
        dec.prepare(blob)
        with pytest.raises(zj.DecodeError) as e:
            call(dec)
        assert e.value.status == ERR_UNSUPPORTED and "resized-crop calls only" in e.value.text
        dec.close()
    dec = zj.Decoder(options(zj), ctx)
    with pytest.raises(zj.DecodeError) as e:
        dec.decode_buffer(blob)
    assert e.value.status == ERR_UNSUPPORTED
    dec.close()
    # the oriented full-frame call for a file that is to be turned (the call's own path, not finish_pixels_device's)
    turned = odd_file(synth, 48, 40, sc.SAMPLINGS[1], 5, orientation=6)
    dec = zj.Decoder(options(zj), ctx)
    dec.prepare(turned)
    assert dec.orientation == 6
    with pytest.raises(zj.DecodeError) as e:
        dec.finish_pixels_device(raw.data_ptr(), raw.numel(), True)
    assert e.value.status == ERR_UNSUPPORTED and "resized-crop calls only" in e.value.text
    dec.close()
    # the pool: the file's own status, its standard neighbour decoded
    plain = odd_file(synth, 48, 40, sc.STANDARD[3], 5)
    with zj.Pool(threads=1, options=options(zj)) as pool:
        for blobs, want in (([blob], [ERR_UNSUPPORTED]), ([plain, blob], [0, ERR_UNSUPPORTED])):
            half = raw.numel() // 2
            lens, _, sts = pool.decode_files_device(blobs, [raw.data_ptr() + half * k for k in range(len(blobs))], [half] * len(blobs), False)
            assert list(sts) == want, sts
    ctx.sync()
    torch.cuda.synchronize()
    assert lens[0] == 48 * 40 * 3 and not bool((raw[:lens[0]] == FILL).all())
    raw.fill_(FILL)
    torch.cuda.synchronize()
    # a window that leaves the image; an output buffer below three channels
    for win, cap in (((1, 0, 48, 40), 3 * 64 * 4), ((0, 0, 48, 41), 3 * 64 * 4), ((0, 0, 0, 4), 3 * 64 * 4), ((0, 0, 48, 40), 2 * 64 * 4)):
        dec = zj.Decoder(options(zj), ctx)
        dec.prepare(blob)
        with pytest.raises(zj.DecodeError) as e:
            resized(dec, win, cap)
        assert e.value.status == ERR_ARG
        dec.close()
    # without the flag the file is refused when it is prepared, as ever
    dec = zj.Decoder(options(zj, 0), ctx)
    with pytest.raises(zj.DecodeError) as e:
        dec.prepare(blob)
    assert e.value.status == ERR_FORMAT
    dec.close()
    ctx.sync()
    assert bool((raw == FILL).all()), "a refused call wrote to the output"
    # ... and the good call
    dec = zj.Decoder(options(zj), ctx)
    dec.prepare(blob)
    assert resized(dec) == 3 * 64 * 4
    dec.close()
    assert not bool((raw[:3 * 64 * 4] == FILL).all()) and bool((raw[3 * 64 * 4:] == FILL).all())
