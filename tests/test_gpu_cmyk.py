"""GPU: four-component (Adobe CMYK / YCCK) JPEGs as RGB resized crops on an MI355X (ZJ_FLAG_CMYK_TO_RGB).
1. zj_cmyk_to_rgb_device against (a * k + 127) // 255 in numpy over the size / pitch / alignment matrix of
   tests/cmyk_stage_cases.py, in place and apart, padding and guard bytes untouched; argument errors launch nothing.
2. Files: the single-file call equals the definition, run stage by stage through calls the library already had -- the crop or
   reduced decode of components 1-3 and of component 4 from the planes zj_decoder_plane gives, zj_orient_device,
   zj_cmyk_to_rgb_device, zj_resize_filtered_device.
3. The batch call and tensors.decode_files_resized_to_tensor with four-component files between colour and gray files; the
   device entropy options; nothing changes without the flag.
4. Pillow-written CMYK files against Pillow's convert("RGB"), within the error of the stages the parent already had.
5. The status codes.
Every comparison but 4 is torch.equal / np.array_equal on bytes."""
import ctypes as C
import importlib
import io

import numpy as np
import pytest

import cmyk_cases as cc
import cmyk_stage_cases as sc
import orient_model as om
import scaled_model as sm

pytestmark = pytest.mark.gpu
FILL = 0xA5
ERR_ARG, ERR_UNSUPPORTED, ERR_PANIC, ERR_SOF = -1, -2, -5, -26
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


# ---- 1. the stage by itself -------------------------------------------------------------------------------------------
def aligned_cuda(torch, n):
    """n bytes of device memory that start on a 16-byte boundary"""
    t = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    off = (-t.data_ptr()) % 16
    return t[off:off + n]


def stage_call(zj, ctx, torch, rng, cases, chw, in_place):
    lay = sc.Layout(rng, cases, chw, in_place)
    src = aligned_cuda(torch, lay.src.size)
    src.copy_(torch.from_numpy(lay.src))
    arena = aligned_cuda(torch, lay.arena_len)
    arena.copy_(torch.from_numpy(lay.arena0))
    torch.cuda.synchronize()
    a_base = arena.data_ptr() if in_place else src.data_ptr()
    ctx.cmyk_to_rgb_device([a_base + o for o in lay.a_off], [src.data_ptr() + o for o in lay.k_off], lay.sizes,
                           zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, [arena.data_ptr() + o for o in lay.out_off], lay.inverted,
                           lay.a_pitch, lay.k_pitch, lay.out_pitch)
    ctx.sync()
    got = arena.cpu().numpy()
    assert np.array_equal(got[lay.inside], lay.want[lay.inside]), "an image differs from (a * k + 127) // 255"
    assert (got[~lay.inside] == sc.SENTINEL).all(), "a padding or guard byte was written"
    assert np.array_equal(src.cpu().numpy(), lay.src), "an input was written"


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_over_the_size_pitch_and_alignment_matrix(zj, ctx, torch, chw, in_place):
    """1152 image pairs in one call: every width, height, pitch and base of the matrix, both values of `inverted`"""
    stage_call(zj, ctx, torch, np.random.default_rng(41 + chw + 2 * in_place), sc.matrix(), chw, in_place)


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_129_images_of_mixed_sizes(zj, ctx, torch, chw):
    rng = np.random.default_rng(87 + chw)
    stage_call(zj, ctx, torch, rng, sc.mixed_129(rng), chw, bool(chw))


def test_stage_tight_pitches_by_default_and_the_tensor_wrapper(zj, tz, ctx, torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    sizes = ((17, 9), (130, 3), (1, 1), (33, 9))
    for layout in ("HWC", "CHW"):
        imgs = [rnd(3, h, w) if layout == "CHW" else rnd(h, w, 3) for w, h in sizes]
        ks = [rnd(h, w) for w, h in sizes[:3]] + [rnd(9, 40)[:, 3:36]]  # (the last plane's rows at a pitch of 40)
        inv = [True, False, True, False]
        outs = tz.cmyk_to_rgb_tensor(ctx, imgs, ks, layout, inv)
        torch.cuda.synchronize()
        for a, k, i, o in zip(imgs, ks, inv, outs):
            kk = k.cpu().numpy()
            want = sc.combine(a.cpu().numpy(), kk[None] if layout == "CHW" else kk[:, :, None], i)
            assert o.is_contiguous() and np.array_equal(o.cpu().numpy(), want)


def test_stage_argument_errors_launch_nothing(zj, ctx, torch):
    a = torch.full((256,), 200, dtype=torch.uint8, device="cuda")
    k = torch.full((64,), 255, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = zj.lib()

    def call(n, aa, kk, wh, ap, kp, layout, inv, outs, op):
        arr = lambda v: (C.c_void_p * len(v))(*v) if v is not None else None
        u = lambda v: (C.c_uint * len(v))(*v) if v is not None else None
        b = (C.c_uint8 * len(inv))(*inv) if inv is not None else None
        return L.zj_cmyk_to_rgb_device(ctx.handle, n, arr(aa), arr(kk), u(wh), u(ap), u(kp), layout, b, arr(outs), u(op), None)

    pa, pk, po = a.data_ptr(), k.data_ptr(), dst.data_ptr()
    assert call(2, [pa, pa], [pk, pk], [4, 4, 0, 4], None, None, 0, None, [po, po + 64], None) == ERR_ARG  # an empty image behind a good one
    assert call(1, [pa], [pk], [4, 4], [11], None, 0, None, [po], None) == ERR_ARG                        # a pitch below a row
    assert call(1, [pa], [pk], [4, 4], None, [3], 0, None, [po], None) == ERR_ARG
    assert call(1, [pa], [pk], [4, 4], None, None, 0, None, [po], [11]) == ERR_ARG
    assert call(1, [pa], [pk], [4, 4], None, None, 1, None, [po], [3]) == ERR_ARG
    assert call(1, [pa], [pk], [4, 4], None, None, 2, None, [po], None) == ERR_ARG                        # not a layout
    assert call(1, [pa], [pk], [65536, 1], None, None, 0, None, [po], None) == ERR_ARG
    assert call(2, [pa, pa], [pk, None], [4, 4, 4, 4], None, None, 0, None, [po, po + 64], None) == ERR_ARG
    assert call(0, [pa], [pk], [4, 4], None, None, 0, None, [po], None) == ERR_ARG
    ctx.sync()
    assert bool((dst == FILL).all())
    assert call(1, [pa], [pk], [4, 4], None, None, 0, [1], [po], None) == 0  # inverted: 200 * 255 / 255
    ctx.sync()
    assert bool((dst[:48] == 200).all()) and bool((dst[48:] == FILL).all())
    assert call(1, [pa], [pk], [4, 4], None, None, 0, None, [po], None) == 0  # inverted NULL: complemented, (55 * 0 + 127) / 255
    ctx.sync()
    assert bool((dst[:48] == 0).all()) and bool((dst[48:] == FILL).all())


# ---- 2. files against the definition -------------------------------------------------------------------------------------
def options(zj, flags=None, layout=0, entropy="ENTROPY_CPU", cs=None):
    o = zj.ZuneJpegOptions()
    o.flags = zj.FLAG_CMYK_TO_RGB if flags is None else flags
    o.out_layout = layout
    o.entropy = getattr(zj, entropy)
    if cs is not None:
        o.out_colorspace = cs
    return o


def tdtype(torch, name):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}[name]


def four_file(synth, w, h, mode, seed, progressive=False, adobe=0, restart=0, orientation=None):
    hs, vs = cc.MODES[mode]
    planes = cc.small_planes(w, h, hs, vs, seed=seed, amp=12, dc=120)
    enc = cc.encode_progressive if progressive else cc.encode_baseline
    data = enc(planes, synth.quant_tables(60 + seed % 30), w, h, hs, vs, restart=restart, adobe=adobe)
    return om.splice(data, om.exif_segment(orientation)) if orientation else data


def single_file(zj, tz, ctx, torch, blob, opt, win, size, dt, layout, flip=False, filt="bilinear", max_prescale=1, mean=MEAN, std=STD,
                channels=3):
    dec = zj.Decoder(opt, ctx)
    _, info = dec.prepare(blob)
    if win is None:
        win = (0, 0) + tuple(zj.oriented_size(dec.orientation, int(info.width), int(info.height)))
    ow, oh = size
    raw = torch.full((channels * oh * ow * torch.empty((), dtype=dt).element_size(),), FILL, dtype=torch.uint8, device="cuda")
    one = raw.view(dt).view((channels, oh, ow) if layout == "NCHW" else (oh, ow, channels))
    scale, bias = tz.normalize_factors(channels, mean, std)
    torch.cuda.synchronize()
    try:
        n = dec.finish_pixels_resized_crop_device(win[0], win[1], win[2], win[3], ow, oh, tz._resize_dtype(dt),
                                                  zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, one.data_ptr(),
                                                  raw.numel(), scale, bias, flip, FILTERS[filt][0], max_prescale, True, FILTERS[filt][1])
    finally:
        dec.close()
    assert n == raw.numel(), "*out_len is not the slot's size"
    return one


def stages(zj, ctx, torch, blob, flags, crop_layout, win, size, max_prescale):
    """A and K of the definition through calls the library had before: the file's planes (zj_decoder_plane) as a three-component
    frame (RGB when the Adobe transform is 2, else YCbCr: the stored samples) and as a one-component GRAYSCALE frame, cut to
    the stored window (at the scale the call picks: the reduced window), turned to their displayed form.  Returns (a, k, w, h,
    layout of a, inverted, scale)."""
    dec = zj.Decoder(options(zj, zj.FLAG_CMYK_TO_RGB | flags), ctx)
    desc, info = dec.prepare(blob)
    assert info.components == 4
    w, h, o = int(info.width), int(info.height), dec.orientation
    transform = dec.adobe_transform
    planes = [torch.from_numpy(dec.plane(c).reshape(-1)).cuda() for c in range(4)]
    dec.close()
    qt, tqs = cc.file_tables(blob)
    ycck = transform == 2
    chw = bool(crop_layout) and ycck
    fa = zj.FrameDesc.make(w, h, int(info.h_max), int(info.v_max), 3, zj.ColorSpace.RGB if ycck else zj.ColorSpace.YCbCr,
                           [qt[t] for t in tqs[:3]], flags=flags, out_layout=zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC)
    fk = zj.FrameDesc.make(w, h, 1, 1, 1, zj.ColorSpace.GRAYSCALE, [qt[tqs[3]]], flags=flags)
    if win is None:
        win = (0, 0) + tuple(om.oriented_size(o, w, h))
    st = om.stored_window(o, w, h, win)
    k = sm.prescale_log2(win[2], win[3], size[0], size[1], {1: 0, 2: 1, 4: 2, 8: 3}[max_prescale])
    if k:
        st = sm.reduced_window(st[0], st[1], st[2], st[3], k, w, h)
    cw, chh = st[2], st[3]
    a = torch.full((3, chh, cw) if chw else (chh, cw, 3), FILL, dtype=torch.uint8, device="cuda")
    kk = torch.full((chh, cw), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in planes]
    if k:
        ctx.decode_crops_scaled_device(fa, [p[0]], [p[1]], [p[2]], 1 << k, [a.data_ptr()], [st])
        ctx.decode_crops_scaled_device(fk, [p[3]], None, None, 1 << k, [kk.data_ptr()], [st])
    else:
        ctx.decode_crops_device(fa, [p[0]], [p[1]], [p[2]], [(st[0], st[1])], cw, chh, [a.data_ptr()])
        ctx.decode_crops_device(fk, [p[3]], None, None, [(st[0], st[1])], cw, chh, [kk.data_ptr()])
    dw, dh = om.oriented_size(o, cw, chh)
    a2 = torch.empty((3, dh, dw) if chw else (dh, dw, 3), dtype=torch.uint8, device="cuda")
    k2 = torch.empty((dh, dw), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.orient_device([a.data_ptr()], [(cw, chh)], 3, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, [o], [a2.data_ptr()])
    ctx.orient_device([kk.data_ptr()], [(cw, chh)], 1, zj.LAYOUT_HWC, [o], [k2.data_ptr()])
    ctx.sync()
    return a2, k2, dw, dh, chw, transform >= 0, k


def definition(zj, tz, ctx, torch, blob, flags, crop_layout, win, size, dt, layout, flip, filt, max_prescale):
    a, k, dw, dh, chw, inverted, scale_k = stages(zj, ctx, torch, blob, flags, crop_layout, win, size, max_prescale)
    lay = zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC
    ctx.cmyk_to_rgb_device([a.data_ptr()], [k.data_ptr()], [(dw, dh)], lay, [a.data_ptr()], [inverted])  # in place
    ow, oh = size
    one = torch.full((3, oh, ow) if layout == "NCHW" else (oh, ow, 3), 0, dtype=dt, device="cuda")
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    torch.cuda.synchronize()
    ctx.resize_device([a.data_ptr()], [(dw, dh)], 3, lay, ow, oh, tz._resize_dtype(dt),
                      zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, one.data_ptr(), scale, bias, [flip], None, None,
                      FILTERS[filt][0], FILTERS[filt][1])
    ctx.sync()
    return scale_k, one


# (w, h), mode, progressive, adobe transform, orientation, displayed window (None: all), flip, filter, dtype, tensor layout,
# crop layout, max_prescale, flags(corrected?), output size
FILE_CASES = [
    ((48, 40), "none", False, 0, 1, None, False, "bilinear", "u8", "NHWC", 0, 1, False, (12, 9)),
    ((48, 40), "h", True, 2, 6, None, True, "aa", "bf16", "NCHW", 1, 1, True, (12, 9)),
    ((48, 40), "v", False, None, 2, (5, 7, 31, 30), False, "bicubic", "f32", "NCHW", 0, 8, False, (12, 9)),
    ((48, 40), "hv", True, 0, 1, (0, 30, 48, 10), True, "aa", "u8", "NCHW", 1, 8, True, (12, 9)),     # rows below rows_covered
    ((100, 75), "none", True, 2, 6, None, False, "bicubic", "bf16", "NHWC", 1, 8, False, (9, 12)),   # 1/8: 75 x 100 shown
    ((100, 75), "h", False, None, 1, (3, 2, 90, 70), True, "bilinear", "f32", "NHWC", 0, 8, True, (12, 9)),
    ((100, 75), "v", True, 0, 2, None, False, "aa", "u8", "NHWC", 0, 1, True, (12, 9)),
    ((100, 75), "hv", False, 2, 6, (5, 9, 30, 80), True, "bilinear", "f32", "NCHW", 1, 1, False, (12, 9)),
    ((16, 16), "none", False, None, 6, None, True, "bicubic", "u8", "NCHW", 1, 1, True, (12, 9)),
    ((16, 16), "h", True, 0, 1, (1, 0, 15, 16), False, "bilinear", "bf16", "NCHW", 0, 8, False, (7, 5)),
    ((16, 16), "v", False, 2, 2, (4, 4, 1, 1), False, "aa", "f32", "NHWC", 1, 1, False, (3, 3)),
    ((16, 16), "hv", True, 2, 1, None, True, "bicubic", "u8", "NHWC", 1, 8, True, (4, 4)),
    # 33 pixels wide: component 4's GRAYSCALE decode at full resolution is ZJ_ERR_PANIC like any one-component frame of that
    # width (zj_plan.h: make_plan), so these take a reduced decode, which has no strips
    ((33, 17), "none", False, 0, 1, None, False, "bilinear", "u8", "NHWC", 0, 8, False, (8, 4)),
    ((33, 17), "h", True, None, 6, None, True, "aa", "f32", "NCHW", 0, 8, True, (4, 8)),
    ((33, 17), "v", False, 2, 2, None, False, "bicubic", "bf16", "NHWC", 1, 8, False, (16, 8)),
    ((33, 17), "hv", True, 2, 1, (1, 1, 32, 16), True, "bilinear", "u8", "NCHW", 1, 8, True, (8, 4)),
]


@pytest.mark.parametrize("case", FILE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}-{'p' if c[2] else 'b'}-t{c[3]}-o{c[4]}-{c[7]}-{c[8]}")
def test_single_file_call_equals_its_stages(zj, tz, ctx, torch, synth, case):
    (w, h), mode, prog, adobe, o, win, flip, filt, dtype, layout, crop_layout, max_prescale, corrected, size = case
    blob = four_file(synth, w, h, mode, seed=w + 3 * o + len(mode), progressive=prog, adobe=adobe, restart=0 if prog else 3,
                     orientation=o if o != 1 else None)
    flags = zj.FLAG_CORRECTED if corrected else 0
    dt = tdtype(torch, dtype)
    k, want = definition(zj, tz, ctx, torch, blob, flags, crop_layout, win, size, dt, layout, flip, filt, max_prescale)
    got = single_file(zj, tz, ctx, torch, blob, options(zj, zj.FLAG_CMYK_TO_RGB | flags, crop_layout), win, size, dt, layout, flip,
                      filt, max_prescale)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), f"scale {k}"
    if w == 33:
        assert k >= 1
    # the device entropy options leave such a file to the CPU walk: the same bytes
    for entropy in ("ENTROPY_GPU", "ENTROPY_GPU_ALWAYS"):
        dev = single_file(zj, tz, ctx, torch, blob, options(zj, zj.FLAG_CMYK_TO_RGB | flags, crop_layout, entropy), win, size, dt,
                          layout, flip, filt, max_prescale)
        assert torch.equal(dev.view(torch.uint8), want.view(torch.uint8)), entropy


def test_the_scales_the_cases_reach():
    ks = set()
    for (w, h), _, _, _, o, win, _, _, _, _, _, mp, _, size in FILE_CASES:
        ww, hh = (win[2], win[3]) if win else om.oriented_size(o, w, h)
        ks.add(sm.prescale_log2(ww, hh, size[0], size[1], {1: 0, 8: 3}[mp]))
    assert ks >= {0, 1, 2, 3}


# ---- 3. the batch call ------------------------------------------------------------------------------------------------------
def pillow_file(w, h, seed, gray, progressive=False, orientation=None, subsampling="4:2:0", quality=85):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 3 + yy * 2 + seed * 17) % 256, (xx * yy // 7 + 40 * seed) % 256, (255 - xx - 2 * yy) % 256], -1)
    img = (img + rng.integers(0, 24, img.shape)).clip(0, 255).astype(np.uint8)
    buf = io.BytesIO()
    if gray:
        Image.fromarray(img[..., 0]).save(buf, "JPEG", quality=quality, progressive=progressive)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=subsampling, progressive=progressive)
    data = buf.getvalue()
    return om.splice(data, om.exif_segment(orientation)) if orientation else data


def pillow_cmyk(w, h, seed, **save):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 // (w - 1)), (yy * 255 // (h - 1)), ((xx + yy) * 3) % 256, (xx * yy // 9) % 160], axis=2)
    img = np.clip(img + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img, "CMYK").save(buf, "JPEG", **save)
    return buf.getvalue()


def mixed_files(synth):
    """(blob, has four components): four-component files of both kinds between colour and gray files"""
    return [(pillow_file(96, 72, 1, False), False), (four_file(synth, 100, 75, "hv", 21, adobe=2), True),
            (pillow_file(80, 56, 2, True), False), (pillow_cmyk(64, 48, 3, quality=85), True),
            (pillow_file(97, 61, 3, False, subsampling="4:4:4", orientation=6), False),
            (four_file(synth, 48, 40, "h", 22, progressive=True, adobe=None, orientation=6), True),
            (pillow_cmyk(80, 64, 4, quality=75, progressive=True), True), (pillow_file(64, 48, 6, False, progressive=True), False)]


@pytest.mark.parametrize("workers", [1, 4])
def test_four_component_files_between_colour_and_gray_files(zj, tz, ctx, torch, synth, workers):
    files = mixed_files(synth)
    blobs = [b for b, _ in files]
    both = zj.FLAG_GRAY_TO_RGB | zj.FLAG_CMYK_TO_RGB
    size = (16, 12)
    wins = [None, None, (3, 5, 40, 30), None, None, (2, 1, 30, 40), (1, 1, 70, 60), None]
    flips = [k % 3 == 1 for k in range(len(blobs))]
    for dt, layout, filt, max_prescale in ((torch.uint8, "NHWC", "bilinear", 1), (torch.float32, "NCHW", "aa", 4)):
        kw = dict(dtype=dt, layout=layout, antialias=FILTERS[filt][0], max_prescale=max_prescale, apply_orientation=True,
                  workers=workers, mean=MEAN, std=STD)
        out = tz.decode_files_resized_to_tensor(ctx, blobs, wins, size, flips=flips, options=options(zj, both), **kw)
        torch.cuda.synchronize()
        for k, (blob, four) in enumerate(files):
            one = single_file(zj, tz, ctx, torch, blob, options(zj, both), wins[k], size, dt, layout, flips[k], filt, max_prescale)
            assert torch.equal(out[k].view(torch.uint8), one.view(torch.uint8)), f"file {k} differs from the single-file call"
            if four:
                _, want = definition(zj, tz, ctx, torch, blob, 0, 0, wins[k], size, dt, layout, flips[k], filt, max_prescale)
                assert torch.equal(out[k].view(torch.uint8), want.view(torch.uint8)), f"file {k} differs from its stages"
        # the colour and gray files: what the same call gives without the four-component files, and without their flag
        rest = [k for k, (_, four) in enumerate(files) if not four]
        pick = lambda v: [v[k] for k in rest]
        alone = tz.decode_files_resized_to_tensor(ctx, pick(blobs), pick(wins), size, flips=pick(flips),
                                                  options=options(zj, zj.FLAG_GRAY_TO_RGB), **kw)
        torch.cuda.synchronize()
        assert torch.equal(out[rest].view(torch.uint8), alone.view(torch.uint8)), "a file changed beside four-component files"


def test_without_the_flag_the_batch_names_the_file(zj, tz, ctx, torch, synth):
    files = mixed_files(synth)[:3]
    blobs = [b for b, _ in files]
    with pytest.raises(zj.DecodeError) as e:
        tz.decode_files_resized_to_tensor(ctx, blobs, None, (8, 8), dtype=torch.uint8, options=options(zj, zj.FLAG_GRAY_TO_RGB))
    assert e.value.status == ERR_SOF and e.value.text == "file 1: Invalid components. Found 4, expected either 1 or 3"


def test_with_the_flag_the_batch_gives_a_tensor(zj, tz, ctx, torch, synth):
    files = mixed_files(synth)[:3]
    out = tz.decode_files_resized_to_tensor(ctx, [b for b, _ in files], None, (8, 8), dtype=torch.uint8, layout="NHWC",
                                            options=options(zj, zj.FLAG_GRAY_TO_RGB | zj.FLAG_CMYK_TO_RGB))
    torch.cuda.synchronize()
    assert out.shape == (3, 8, 8, 3) and out.dtype == torch.uint8
    one = single_file(zj, tz, ctx, torch, files[1][0], options(zj), None, (8, 8), torch.uint8, "NHWC", mean=None, std=None)
    assert torch.equal(out[1], one)
    assert int(out[1].max()) > int(out[1].min()), "a flat image"


# ---- 4. Pillow's files against Pillow ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality,progressive,wh", [(75, False, (64, 48)), (95, True, (96, 32)), (90, False, (48, 64))])
def test_pillow_cmyk_files_against_pillow(zj, tz, ctx, torch, quality, progressive, wh):
    """|ours - convert("RGB")| <= eA + eK + 1: eA, eK the largest differences between the stages the library had before (the
    stored samples of components 1-3 and of component 4, ZJ_FLAG_CORRECTED) and Pillow's own CMYK samples of this file,
    measured here; 1 for the stage's rounding.  With c = a * k / 255: |c - c'| <= |a - a'| k / 255 + a' |k - k'| / 255."""
    from PIL import Image
    w, h = wh  # multiples of 16, an even number of MCU rows
    blob = pillow_cmyk(w, h, quality, quality=quality, progressive=progressive)
    im = Image.open(io.BytesIO(blob))
    assert im.mode == "CMYK"
    stored = 255 - np.asarray(im).astype(np.int32)  # (Pillow complements what an Adobe file stores)
    rgb = np.asarray(im.convert("RGB")).astype(np.int32)
    a, k, dw, dh, chw, inverted, _ = stages(zj, ctx, torch, blob, zj.FLAG_CORRECTED, 0, None, (w, h), 1)
    assert (dw, dh) == (w, h) and inverted and not chw
    eA = int(np.abs(a.cpu().numpy().astype(np.int32) - stored[..., :3]).max())
    eK = int(np.abs(k.cpu().numpy().astype(np.int32) - stored[..., 3]).max())
    ours = single_file(zj, tz, ctx, torch, blob, options(zj, zj.FLAG_CMYK_TO_RGB | zj.FLAG_CORRECTED), None, (w, h), torch.uint8,
                       "NHWC", mean=None, std=None)
    worst = int(np.abs(ours.cpu().numpy().astype(np.int32) - rgb).max())
    print(f"pillow cmyk q{quality} {'progressive' if progressive else 'baseline'} {w}x{h}: eA {eA} eK {eK} largest |ours - Pillow| {worst}")
    assert worst <= eA + eK + 1


# ---- 5. status codes ----------------------------------------------------------------------------------------------------------
def test_status_codes(zj, tz, ctx, torch, synth):
    blob = four_file(synth, 48, 40, "hv", 5, adobe=2)
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
    # a window that leaves the image; an output buffer below three channels
    for win, cap in (((1, 0, 48, 40), 3 * 64 * 4), ((0, 0, 48, 41), 3 * 64 * 4), ((0, 0, 0, 4), 3 * 64 * 4), ((0, 0, 48, 40), 2 * 64 * 4)):
        dec = zj.Decoder(options(zj), ctx)
        dec.prepare(blob)
        with pytest.raises(zj.DecodeError) as e:
            resized(dec, win, cap)
        assert e.value.status == ERR_ARG
        dec.close()
    # a file 33 pixels wide at full resolution: the status its component 4 has as a one-component GRAYSCALE frame
    dec = zj.Decoder(options(zj), ctx)
    dec.prepare(four_file(synth, 33, 17, "none", 6))
    with pytest.raises(zj.DecodeError) as e:
        resized(dec, (0, 0, 33, 17))
    assert e.value.status == ERR_PANIC
    dec.close()
    ctx.sync()
    assert bool((raw == FILL).all()), "a refused call wrote to the output"
    # the flag on a frame descriptor: an unknown bit
    planes, qts = synth.make_frame(48, 40, 2, 2, 3, seed=1, quality=70)
    dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]
    d = zj.FrameDesc.make(48, 40, 2, 2, 3, zj.ColorSpace.RGB, qts, flags=zj.FLAG_CMYK_TO_RGB)
    for call in (lambda: ctx.decode_crops_resized_device(d, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()],
                                                         [(0, 0, 48, 40)], 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, raw.data_ptr()),
                 lambda: ctx.decode_crops_device(d, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], [(0, 0)], 16, 16,
                                                 [raw.data_ptr()])):
        with pytest.raises(zj.ZjError) as e:
            call()
        assert e.value.status == ERR_ARG
    ctx.sync()
    assert bool((raw == FILL).all())
    # ... and the good call
    dec = zj.Decoder(options(zj), ctx)
    dec.prepare(blob)
    assert resized(dec) == 3 * 64 * 4
    dec.close()
    assert not bool((raw[:3 * 64 * 4] == FILL).all()) and bool((raw[3 * 64 * 4:] == FILL).all())
