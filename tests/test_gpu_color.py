"""GPU: per-image colour matrices on an MI355X.
1. zj_color_device against the definition in numpy (tests/color_model.py) byte for byte: images 1 x 1, 17 x 3, 53 x 37 and
   258 x 3, both layouts, in place and apart, odd pitches and addresses, 49 images in one call; padding and guard bytes
   untouched; argument errors launch nothing.
2. zj_decode_crops_resized_mixed_colored_device image by image against the definition run through calls the library already
   had: the crop or reduced decode, zj_orient_device, zj_gray_to_rgb_device, the model on the host, zj_resize_filtered_device.
   NULL and all-identity matrices are the uncoloured call; a GRAYSCALE output is refused.
3. zj_decoder_finish_pixels_resized_crop_batch_colored_device over a colour, a gray, a CMYK, a 4:1:1, a turned and a damaged
   file and one with a refused matrix, under the CPU walker and under device entropy, against each file's uncoloured u8 image
   through the model and zj_resize_filtered_device.
4. The tensors wrappers against the uncoloured float32 result with the matrix applied in float64 afterwards.
Every comparison but 4 is on bytes."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import color_cases as cc
import color_model as cm
import orient_model as om
import resize_model as rm
import scaled_model as sm
from test_gpu_crop_tensor import ESZ, GUARD, body, guarded, layout_code
from test_gpu_mixed import Frame, filled, tdtype

pytestmark = pytest.mark.gpu
FILL = 0xA5
ERR_ARG, ERR_UNSUPPORTED = -1, -2
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


@pytest.fixture(scope="module")
def je():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import jpeg_enc
    return jpeg_enc


# ---- 1. the stage by itself -------------------------------------------------------------------------------------------
def aligned_cuda(torch, n):
    """n bytes of device memory that start on a 16-byte boundary"""
    t = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    off = (-t.data_ptr()) % 16
    return t[off:off + n]


def stage_call(zj, ctx, torch, rng, cases, chw, in_place, matrices=cc.MATRICES):
    lay = cc.Layout(rng, cases, chw, in_place, matrices=matrices)
    arena = aligned_cuda(torch, lay.arena_len)
    arena.copy_(torch.from_numpy(lay.arena0))
    if in_place:
        src = arena
    else:
        src = aligned_cuda(torch, lay.src.size)
        src.copy_(torch.from_numpy(lay.src))
    torch.cuda.synchronize()
    ctx.color_device([src.data_ptr() + o for o in lay.in_off], lay.sizes, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, lay.m,
                     [arena.data_ptr() + o for o in lay.out_off], lay.in_pitch, lay.out_pitch)
    ctx.sync()
    got = arena.cpu().numpy()
    assert np.array_equal(got[lay.inside], lay.want[lay.inside]), "an image differs from the definition"
    assert (got[~lay.inside] == cc.SENTINEL).all(), "a padding or guard byte was written"
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), lay.src), "an input was written"


def stage_cases():
    """1 x 1, 17 x 3, 53 x 37 and 258 x 3 at every pad pair and at odd and even offsets from a 16-byte boundary"""
    out = []
    for i, (w, h) in enumerate([(1, 1), (17, 3), (53, 37), (258, 3)]):
        for j, (ip, op) in enumerate([(0, 0), (1, 13), (13, 1), (0, 1)]):
            for base in (0, 1, 4, 15):
                out.append((w, h, ip, op, (base + 3 * j + i) % 16, base))
    return out


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_equals_the_model(zj, ctx, torch, chw, in_place):
    cases = stage_cases()
    assert len(cases) == 64  # (two launches)
    stage_call(zj, ctx, torch, np.random.default_rng(41 + chw + 2 * in_place), cases, chw, in_place)


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_operand_extremes_equal_the_model(zj, ctx, torch, chw, in_place):
    """color_cases.EXTREMES (+-16 / +-4096 in every entry; mixed signs beside entries of 1/65536): color_mad is __mul24 on the
    device and a plain product in the emulation, so only this run shows the instruction at the ends of its operands.  Widths 1,
    15, 16, 17, 33, every width under each of the three matrices, against color_model.apply_fixed."""
    cases = [(w, 3, 1, 13, (3 * i + k) % 16, (5 * i + 7 * k) % 16) for i, w in enumerate(cc.EXTREME_WIDTHS) for k in range(3)]
    assert len(cases) == 15 and [c[0] for c in cases[::3]] == list(cc.EXTREME_WIDTHS)   # case 3i + k: width i under matrix k
    stage_call(zj, ctx, torch, np.random.default_rng(112 + chw + 2 * in_place), cases, chw, in_place, matrices=cc.EXTREMES)


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_49_images_in_one_call(zj, ctx, torch, chw):
    rng = np.random.default_rng(87 + chw)
    stage_call(zj, ctx, torch, rng, cc.mixed_49(rng), chw, bool(chw))


def test_stage_tight_pitches_by_default_and_the_tensor_wrapper(zj, tz, ctx, torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    sizes = ((17, 9), (130, 3), (1, 1), (33, 9))
    ms = [tz.color_matrix(1.8, 1.6, 2.0, 0.2), None, tz.color_matrix(bgr=True), tz.color_matrix(grayscale=True)]
    for layout in ("HWC", "CHW"):
        chw = layout == "CHW"
        imgs = [rnd(3, h, w) if chw else rnd(h, w, 3) for w, h in sizes[:3]]
        wide = rnd(3, 9, 40) if chw else rnd(9, 40, 3)      # (the last image's rows at a pitch of 40 pixels)
        imgs.append(wide[:, :, 3:36] if chw else wide[:, 3:36])
        before = [im.cpu().numpy() for im in imgs]
        outs = tz.color_twist_tensor(ctx, imgs, ms, layout)
        torch.cuda.synchronize()
        for a, m, o in zip(before, ms, outs):
            assert o.is_contiguous() and np.array_equal(o.cpu().numpy(), cm.apply(cm.IDENTITY if m is None else m, a, chw))
        same = tz.color_twist_tensor(ctx, imgs, ms, layout, inplace=True)
        torch.cuda.synchronize()
        for a, m, o, im in zip(before, ms, same, imgs):
            assert o is im and np.array_equal(im.cpu().numpy(), cm.apply(cm.IDENTITY if m is None else m, a, chw))


def test_stage_argument_errors_launch_nothing(zj, ctx, torch):
    a = torch.full((256,), 200, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = zj.lib()
    ident = list(cm.IDENTITY.reshape(-1))

    def call(n, ins, wh, ip, layout, ms, outs, op, handle=ctx.handle):
        arr = lambda v: (C.c_void_p * len(v))(*v) if v is not None else None
        u = lambda v: (C.c_uint * len(v))(*v) if v is not None else None
        m = (C.c_double * len(ms))(*ms) if ms is not None else None
        return L.zj_color_device(handle, n, arr(ins), u(wh), u(ip), layout, m, arr(outs), u(op), None)

    pa, po = a.data_ptr(), dst.data_ptr()
    assert call(1, [pa], [4, 4], None, 0, ident, [po], None, handle=None) == ERR_ARG                   # NULL pointers
    assert call(1, None, [4, 4], None, 0, ident, [po], None) == ERR_ARG
    assert call(1, [pa], None, None, 0, ident, [po], None) == ERR_ARG
    assert call(1, [pa], [4, 4], None, 0, None, [po], None) == ERR_ARG
    assert call(1, [pa], [4, 4], None, 0, ident, None, None) == ERR_ARG
    assert call(2, [pa, None], [4, 4, 4, 4], None, 0, ident * 2, [po, po + 64], None) == ERR_ARG
    assert call(2, [pa, pa], [4, 4, 4, 4], None, 0, ident * 2, [po, None], None) == ERR_ARG
    assert call(0, [pa], [4, 4], None, 0, ident, [po], None) == ERR_ARG
    assert call(2, [pa, pa], [4, 4, 0, 4], None, 0, ident * 2, [po, po + 64], None) == ERR_ARG          # an empty image behind a good one
    assert call(1, [pa], [65536, 1], None, 0, ident, [po], None) == ERR_ARG
    assert call(1, [pa], [4, 4], [11], 0, ident, [po], None) == ERR_ARG                                # a pitch below a row
    assert call(1, [pa], [4, 4], None, 0, ident, [po], [11]) == ERR_ARG
    assert call(1, [pa], [4, 4], None, 1, ident, [po], [3]) == ERR_ARG
    assert call(1, [pa], [4, 4], None, 2, ident, [po], None) == ERR_ARG                                # not a layout
    for bad in (float("nan"), float("inf"), 16.001):
        ms = ident * 2
        ms[12 + 5] = bad                                                                               # the second image's matrix
        assert call(2, [pa, pa], [4, 4, 4, 4], None, 0, ms, [po, po + 64], None) == ERR_ARG
    ctx.sync()
    assert bool((dst == FILL).all())
    assert call(1, [pa], [4, 4], None, 0, list(cm.NEGATIVE.reshape(-1)), [po], None) == 0
    ctx.sync()
    assert bool((dst[:48] == 55).all()) and bool((dst[48:] == FILL).all())


# ---- 2. the planes call against its stages ---------------------------------------------------------------------------------
def u8_image(zj, ctx, torch, f, win, o, k, chw):
    """The u8 image the uncoloured call resizes, through calls the library had before: the stored window's crop (at scale k:
    the reduced window's), turned to its displayed form, a one-component frame copied into three channels.  On the host,
    [dh, dw, 3] or (chw) [3, dh, dw]."""
    gray = f.desc.in_components == 1
    d = copy.copy(f.desc)
    d.flags &= ~zj.FLAG_GRAY_TO_RGB
    if gray:
        d.out_colorspace = int(zj.ColorSpace.GRAYSCALE)
    ch = 1 if gray else 3
    planes = chw and not gray
    st = om.stored_window(o, f.w, f.h, win)
    if k:
        st = sm.reduced_window(st[0], st[1], st[2], st[3], k, f.w, f.h)
    cw, chh = st[2], st[3]
    crop = torch.full((ch * cw * chh,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cb, cr = ([f.ptr(1)], [f.ptr(2)]) if not gray else (None, None)
    if k:
        ctx.decode_crops_scaled_device(d, [f.ptr(0)], cb, cr, 1 << k, [crop.data_ptr()], [st])
    else:
        ctx.decode_crops_device(d, [f.ptr(0)], cb, cr, [(st[0], st[1])], cw, chh, [crop.data_ptr()])
    dw, dh = om.oriented_size(o, cw, chh)
    shown = torch.empty_like(crop)
    ctx.orient_device([crop.data_ptr()], [(cw, chh)], ch, zj.LAYOUT_CHW if planes else zj.LAYOUT_HWC, [o], [shown.data_ptr()])
    if gray:
        rgb = torch.empty((3 * dw * dh,), dtype=torch.uint8, device="cuda")
        ctx.gray_to_rgb_device([shown.data_ptr()], [(dw, dh)], zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, [rgb.data_ptr()])
        shown = rgb
    ctx.sync()
    return shown.cpu().numpy().reshape((3, dh, dw) if chw else (dh, dw, 3))


def resize_u8(zj, tz, ctx, torch, img, chw, size, dt, layout, scale, bias, flip, antialias, interpolation="bilinear"):
    """zj_resize_filtered_device over one u8 image on the host: the output image"""
    dh, dw = (img.shape[1], img.shape[2]) if chw else (img.shape[0], img.shape[1])
    dev = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    _, one = filled(torch, 1, 3, size, dt, layout)
    torch.cuda.synchronize()
    ctx.resize_device([dev.data_ptr()], [(dw, dh)], 3, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, size[0], size[1], tz._resize_dtype(dt),
                      zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, one.data_ptr(), scale, bias, [flip], None, None, antialias,
                      interpolation)
    ctx.sync()
    return one[0]


def plane_frames(zj, torch, synth, crop_layout):
    """96 x 80 and 517 x 40 in the four sampling modes, and one one-component frame shown as RGB"""
    modes = ["444", "422", "440", "420"]
    frames = [Frame(zj, torch, synth, 96, 80, m, layout=crop_layout, seed=10 + i, quality=60 + 8 * i) for i, m in enumerate(modes)]
    frames += [Frame(zj, torch, synth, 517, 40, m, layout=crop_layout, seed=20 + i, quality=85 - 6 * i,
                     flags=zj.FLAG_CORRECTED if i % 2 else 0) for i, m in enumerate(modes)]
    frames.append(Frame(zj, torch, synth, 96, 80, "444", layout=crop_layout, flags=zj.FLAG_GRAY_TO_RGB, seed=30, in_comp=1))
    # windows that are not tile-aligned, in displayed pixels; frame 2 is shown under orientation 6 (80 x 96)
    wins = [(0, 0, 96, 80), (3, 5, 70, 50), (7, 9, 61, 83), (1, 2, 95, 77), (5, 3, 301, 36), (257, 1, 259, 38), (0, 0, 517, 40),
            (11, 7, 100, 30), (3, 5, 90, 71)]
    oris = [1, 1, 6, 1, 1, 1, 1, 1, 1]
    return frames, wins, oris


def plane_matrices(tz, n):
    ms = [tz.color_matrix(1.8, 1.6, 2.0, 0.2), tz.color_matrix(grayscale=True), tz.color_matrix(bgr=True), cm.NEGATIVE,
          tz.color_matrix(contrast=0.8, saturation=0.7), None, tz.color_matrix(brightness=0.5, hue=-0.3), cm.IDENTITY]
    return [ms[i % len(ms)] for i in range(n)]


@pytest.mark.parametrize("config", [("bilinear", "bf16", "NCHW", 0), ("aa", "u8", "NHWC", 1)], ids=lambda c: "-".join(map(str, c)))
def test_plane_call_equals_its_stages(zj, tz, ctx, torch, synth, config):
    filt, dtype, layout, crop_layout = config
    chw = bool(crop_layout)
    frames, wins, oris = plane_frames(zj, torch, synth, crop_layout)
    n, size, maxlog = len(frames), (48, 30), 1
    ms = plane_matrices(tz, n)
    flips = [i % 3 == 1 for i in range(n)]
    dt = tdtype(torch, dtype)
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    ks = [sm.prescale_log2(w[2], w[3], size[0], size[1], maxlog) for w in wins]
    assert set(ks) == {0, 1} and ks[0] == 1
    raw, out = filled(torch, n, 3, size, dt, layout)
    torch.cuda.synchronize()
    ctx.decode_crops_resized_mixed_device([f.desc for f in frames], [f.ptr(0) for f in frames], [f.ptr(1) for f in frames],
                                          [f.ptr(2) for f in frames], wins, size[0], size[1], tz._resize_dtype(dt),
                                          zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, out.data_ptr(), scale, bias, flips,
                                          None, filt == "aa", 1 << maxlog, oris, "bilinear", colors=ms)
    ctx.sync()
    for i, f in enumerate(frames):
        img = u8_image(zj, ctx, torch, f, wins[i], oris[i], ks[i], chw)
        coloured = cm.apply(cm.IDENTITY if ms[i] is None else ms[i], img, chw)
        want = resize_u8(zj, tz, ctx, torch, coloured, chw, size, dt, layout, scale, bias, flips[i], filt == "aa")
        assert torch.equal(out[i].view(torch.uint8), want.view(torch.uint8)), f"frame {i}: differs from resize(colour(u8 image))"
        if ms[i] is not None and not np.array_equal(ms[i], cm.IDENTITY):
            plain = resize_u8(zj, tz, ctx, torch, img, chw, size, dt, layout, scale, bias, flips[i], filt == "aa")
            assert not torch.equal(plain.view(torch.uint8), want.view(torch.uint8)), f"frame {i}: the matrix changes nothing"


def test_plane_call_without_colour_is_the_mixed_call(zj, tz, ctx, torch, synth):
    frames, wins, oris = plane_frames(zj, torch, synth, 0)
    n, size = len(frames), (48, 30)
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    args = ([f.desc for f in frames], [f.ptr(0) for f in frames], [f.ptr(1) for f in frames], [f.ptr(2) for f in frames], wins,
            size[0], size[1], zj.DTYPE_BF16, zj.TENSOR_NCHW)
    outs = []
    for colors in ("null", None, [None] * n, [cm.IDENTITY] * n):
        raw, out = filled(torch, n, 3, size, torch.bfloat16, "NCHW")
        torch.cuda.synchronize()
        if colors == "null":   # the coloured entry point itself with a NULL `color`
            arr = lambda c: (C.c_void_p * n)(*[f.ptr(c) for f in frames])
            rc = zj.lib().zj_decode_crops_resized_mixed_colored_device(
                ctx.handle, (zj.FrameDesc * n)(*args[0]), n, arr(0), arr(1), arr(2), (C.c_uint * (4 * n))(*[v for w in wins for v in w]),
                size[0], size[1], zj.DTYPE_BF16, zj.TENSOR_NCHW, (C.c_float * 3)(*scale), (C.c_float * 3)(*bias), None,
                zj.RESIZE_BILINEAR, 1, (C.c_uint8 * n)(*oris), None, out.data_ptr(), None)
            assert rc == 0
        else:
            ctx.decode_crops_resized_mixed_device(*args, out.data_ptr(), scale, bias, None, None, False, 2, oris, "bilinear", colors=colors)
        ctx.sync()
        outs.append(raw.clone())
    assert not bool((outs[1] == FILL).all())
    for o in outs[:1] + outs[2:]:
        assert torch.equal(o, outs[1])


def test_plane_call_refusals_write_nothing(zj, tz, ctx, torch, synth):
    g = zj.ColorSpace.GRAYSCALE
    frames = [Frame(zj, torch, synth, 96, 80, "420", cs=g, seed=41), Frame(zj, torch, synth, 64, 40, "444", cs=g, in_comp=1, seed=40)]
    wins = [(0, 0, 96, 80), (0, 0, 64, 40)]
    raw, out = filled(torch, 2, 1, (16, 12), torch.float32, "NCHW")
    torch.cuda.synchronize()
    call = lambda fr, colors: ctx.decode_crops_resized_mixed_device(
        [f.desc for f in fr], [f.ptr(0) for f in fr], [f.ptr(1) for f in fr], [f.ptr(2) for f in fr], wins, 16, 12, zj.DTYPE_F32,
        zj.TENSOR_NCHW, out.data_ptr(), None, None, None, None, False, 1, None, "bilinear", colors=colors)
    with pytest.raises(zj.ZjError) as e:
        call(frames, [cm.GRAY, cm.IDENTITY])
    assert e.value.status == ERR_UNSUPPORTED
    rgb = [Frame(zj, torch, synth, 96, 80, "420", seed=41), Frame(zj, torch, synth, 64, 40, "444", seed=40)]
    bad = cm.IDENTITY.copy()
    bad[2, 3] = 4097.0
    with pytest.raises(zj.ZjError) as e:
        call(rgb, [cm.GRAY, bad])
    assert e.value.status == ERR_ARG
    ctx.sync()
    assert bool((raw == FILL).all()), "a refused call wrote to the output"
    call(frames, None)
    ctx.sync()
    assert not bool((raw == FILL).all())


# ---- 3. the batch file call -------------------------------------------------------------------------------------------------
def colour_files(synth, je):
    """(name, blob): a 4:2:0 colour, a gray, a CMYK, a 4:1:1 and a turned file (the warp tests' five), one damaged in the middle
    and one more colour file, for the refused matrix"""
    from test_gpu_to_tensor import colour_file
    from test_gpu_warp import file_cases
    five = [(name, blob) for name, blob, _, _, _ in file_cases(synth, je)]
    return five[:3] + [("damaged", five[0][1][:300])] + five[3:] + [("refused", colour_file(je, synth, 80, 64, 1, 2, 6))]


@pytest.mark.parametrize("entropy", ["ENTROPY_CPU", "ENTROPY_GPU_ALWAYS"])
def test_batch_of_every_kind(zj, tz, ctx, torch, synth, je, entropy):
    from test_gpu_to_tensor import options, resized_call
    files = colour_files(synth, je)
    names = [nm for nm, _ in files]
    n, size = len(files), (40, 28)
    assert names == ["colour", "gray", "cmyk", "damaged", "411", "turned", "refused"]
    opt = options(zj, entropy)
    ms = [tz.color_matrix(1.8, 1.6, 2.0, 0.2), tz.color_matrix(contrast=0.8, saturation=0.7), cm.NEGATIVE, cm.BGR,
          tz.color_matrix(grayscale=True), tz.color_matrix(brightness=0.6, hue=0.25, bgr=True), cm.IDENTITY.copy()]
    ms[6][0, 1] = 16.5                                       # not a matrix the stage takes
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    for dtype, layout, filt in (("bf16", "NCHW", "bilinear"), ("u8", "NHWC", "aa")):
        dt = tdtype(torch, dtype)
        decs, wins, prepared = [], [], []
        for k, (nm, b) in enumerate(files):
            dec = zj.Decoder(opt, ctx)
            try:
                info = dec.prepare(b)[1]
                dw, dh = om.oriented_size(dec.orientation, int(info.width), int(info.height))
                wins.append((3, 2, dw - 7, dh - 5))          # not tile-aligned, in displayed pixels
                prepared.append(True)
            except zj.ZjError:
                assert nm == "damaged" or (entropy != "ENTROPY_CPU" and nm in ("cmyk", "411")), (nm, entropy)
                wins.append((0, 0, 8, 8))
                prepared.append(False)
            decs.append(dec)
        flips = [k % 2 == 1 for k in range(n)]
        raw, out = filled(torch, n, 3, size, dt, layout)
        torch.cuda.synchronize()
        try:
            rcs = zj.finish_pixels_resized_crop_batch(decs, ctx, wins, size[0], size[1], tz._resize_dtype(dt), layout_code(zj, layout),
                                                      out.data_ptr(), raw.numel(), scale, bias, flips, filt == "aa", 1, True,
                                                      "bilinear", colors=ms)
            texts = [zj.lib().zj_decoder_error(d._d).decode(errors="replace") for d in decs]
        finally:
            for d in decs:
                d.close()
        ctx.sync()
        img_bytes = raw.numel() // n
        for k, (nm, b) in enumerate(files):
            slot = raw[k * img_bytes:(k + 1) * img_bytes]
            if nm == "refused":
                assert rcs[k] == ERR_ARG and "colour" in texts[k] and bool((slot == FILL).all())
                continue
            try:   # the uncoloured u8 image of the window: the resized-crop file call at out == window
                w = wins[k]
                assert prepared[k]
                u8 = resized_call(zj, ctx, torch, b, opt, w, rm.U8, "NHWC", None, None, False, oriented=True)
            except (zj.ZjError, AssertionError):
                # a file the uncoloured call does not finish either: its status, its image untouched
                assert nm == "damaged" or (entropy != "ENTROPY_CPU" and nm in ("cmyk", "411")), (nm, entropy)
                assert rcs[k] != 0 and bool((slot == FILL).all()), (nm, rcs)
                continue
            assert rcs[k] == 0, (nm, rcs[k], texts[k])
            img = u8.cpu().numpy().reshape(w[3], w[2], 3)
            want = resize_u8(zj, tz, ctx, torch, cm.apply(ms[k], img), False, size, dt, layout, scale, bias, flips[k], filt == "aa")
            assert torch.equal(out[k].view(torch.uint8).reshape(-1), want.view(torch.uint8).reshape(-1)), (nm, dtype, layout)
        assert rcs[names.index("damaged")] != 0 and rcs[names.index("colour")] == 0 and rcs[names.index("turned")] == 0
        if entropy == "ENTROPY_CPU":
            assert [rc == 0 for rc in rcs] == [True, True, True, False, True, True, False], rcs


def test_batch_without_colour_is_the_batch_call(zj, tz, ctx, torch, synth, je):
    from test_gpu_to_tensor import options
    files = [f for f in colour_files(synth, je) if f[0] not in ("damaged", "refused")]
    blobs = [b for _, b in files]
    opt = options(zj)
    kw = dict(dtype=torch.bfloat16, layout="NHWC", mean=MEAN, std=STD, apply_orientation=True, options=opt, max_prescale=2)
    plain = tz.decode_files_resized_to_tensor(ctx, blobs, None, (24, 16), **kw)
    ident = tz.decode_files_resized_to_tensor(ctx, blobs, None, (24, 16), color=[None] * len(blobs), **kw)
    torch.cuda.synchronize()
    assert torch.equal(plain.view(torch.uint8), ident.view(torch.uint8))
    # a decoder that asks for GRAYSCALE: a matrix is refused for that file
    g = options(zj)
    g.out_colorspace = zj.ColorSpace.GRAYSCALE
    with pytest.raises(zj.DecodeError) as e:
        tz.decode_files_resized_to_tensor(ctx, blobs[:1], None, (8, 8), options=g, color=[cm.GRAY])
    assert e.value.status == ERR_UNSUPPORTED and "file 0" in str(e.value)


# ---- 4. the wrappers -----------------------------------------------------------------------------------------------------------
def wrapper_matrices(tz):
    """matrices whose real outputs stay inside [0, 255] for every input: nothing clamps, so colour and the bilinear taps
    commute up to the stage's rounding"""
    ms = [tz.color_matrix(contrast=0.8, saturation=0.7), tz.color_matrix(grayscale=True), tz.color_matrix(bgr=True)]
    for m in ms:
        lo = np.minimum(m[:, :3], 0).sum(1) * 255 + m[:, 3]
        hi = np.maximum(m[:, :3], 0).sum(1) * 255 + m[:, 3]
        assert (lo >= 0).all() and (hi <= 255).all()
    return ms


def check_commutes(torch, plain, got, ms, scale, bias, dt, layout):
    """|got - (M x + t) scale + bias| <= 0.51 grey levels x scale + the dtype's rounding, x the uncoloured float32 result in
    grey levels.  0.51: the stage rounds once (1/2) and its integers are within 2^-17 of the matrix (3 x 255 x 2^-17 + 2^-17 <
    0.006); the resize is a convex combination of such values."""
    s, b = np.asarray(scale, np.float64), np.asarray(bias, np.float64)
    half_ulp = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dt]  # of |value|: 8 and 11 bits
    for i, m in enumerate(ms):
        x = plain[i].double().cpu().numpy()
        y = got[i].double().cpu().numpy()
        if layout == "NCHW":
            x, y = x.transpose(1, 2, 0), y.transpose(1, 2, 0)
        grey = (x - b) / s
        want = (grey @ m[:, :3].T + m[:, 3]) * s + b
        err = np.abs(y - want)
        tol = 0.51 * s + np.abs(want) * half_ulp
        print(f"image {i}: largest |got - want| / scale = {(err / s).max():.4f} grey levels")
        assert (err <= tol).all(), (i, float((err / s).max()))
        assert np.abs(y - x).max() > 4 * s.max(), "the matrix changed nothing"


@pytest.mark.parametrize("dtype,layout", [("f32", "NCHW"), ("bf16", "NHWC")])
def test_the_wrappers_commute_with_the_matrix(zj, tz, ctx, torch, synth, je, dtype, layout):
    from test_gpu_to_tensor import colour_file, gray_file, options
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]
    ms = wrapper_matrices(tz)
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    # files: a gray, a colour and a turned one (the gray one under the contrast matrix: saturation does nothing to it)
    blobs = [gray_file(je, synth), colour_file(je, synth, 97, 61, 2, 2, 4), colour_file(je, synth, 64, 48, 2, 2, 5, orientation=6)]
    kw = dict(layout=layout, mean=MEAN, std=STD, apply_orientation=True, options=options(zj))
    plain = tz.decode_files_resized_to_tensor(ctx, blobs, None, (33, 21), dtype=torch.float32, **kw)
    got = tz.decode_files_resized_to_tensor(ctx, blobs, None, (33, 21), dtype=dt, color=ms, **kw)
    torch.cuda.synchronize()
    assert got.dtype == dt and got.shape == plain.shape
    check_commutes(torch, plain, got, ms, scale, bias, dt, layout)
    # frames of one geometry
    f = [Frame(zj, torch, synth, 96, 80, "420", seed=50 + i, quality=80) for i in range(3)]
    frames = [tuple(x.planes) for x in f]
    wins = [(3, 5, 70, 50), (0, 0, 96, 80), (11, 2, 85, 77)]
    kw = dict(layout=layout, mean=MEAN, std=STD, flips=[False, True, False])
    plain = tz.decode_resized_crops_to_tensor(ctx, f[0].desc, frames, wins, (33, 21), dtype=torch.float32, **kw)
    got = tz.decode_resized_crops_to_tensor(ctx, f[0].desc, frames, wins, (33, 21), dtype=dt, color=ms, **kw)
    torch.cuda.synchronize()
    check_commutes(torch, plain, got, ms, scale, bias, dt, layout)
    with pytest.raises(ValueError):
        tz.decode_resized_crops_to_tensor(ctx, f[0].desc, frames, wins, (33, 21), color=ms[:2])
