"""GPU: one-component JPEGs as RGB resized crops on an MI355X (ZJ_FLAG_GRAY_TO_RGB).
1. zj_gray_to_rgb_device against numpy's repeat over the size / pitch / alignment matrix of tests/expand_cases.py, padding and
   guard bytes untouched.
2. The mixed and the one-geometry frame calls: a gray frame's image equals the stages the library already has, run one by
   one -- the GRAYSCALE crop (zj_decode_crops_device / zj_decode_crops_scaled_device), zj_orient_device, a torch expand to
   three channels, zj_resize_filtered_device -- and the colour frames keep the bytes they have without the gray frames.
3. Files: Pillow-written gray files among colour ones through tensors.decode_files_resized_to_tensor against the single-file
   call and against a GRAYSCALE decoder.
4. Nothing changes without the flag; the status codes.
Every comparison is torch.equal / np.array_equal on bytes: there are no tolerances."""
import copy
import ctypes as C
import importlib
import io

import numpy as np
import pytest

import expand_cases as ec
import orient_model as om
import scaled_model as sm

pytestmark = pytest.mark.gpu
MODES = {"444": (1, 1), "422": (2, 1), "440": (1, 2), "420": (2, 2)}
FILL = 0xA5
ERR_ARG, ERR_UNSUPPORTED, ERR_PANIC = -1, -2, -5


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


def stage_call(zj, ctx, torch, rng, cases, chw):
    lay = ec.Layout(rng, cases, chw)
    src = aligned_cuda(torch, lay.src.size)
    src.copy_(torch.from_numpy(lay.src))
    arena = aligned_cuda(torch, lay.arena_len)
    arena.fill_(ec.SENTINEL)
    torch.cuda.synchronize()
    ctx.gray_to_rgb_device([src.data_ptr() + o for o in lay.in_off], lay.sizes, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC,
                           [arena.data_ptr() + o for o in lay.out_off], lay.in_pitch, lay.out_pitch)
    ctx.sync()
    got = arena.cpu().numpy()
    assert np.array_equal(got[lay.inside], lay.want[lay.inside]), "an image differs from numpy's repeat"
    assert (got[~lay.inside] == ec.SENTINEL).all(), "a padding or guard byte was written"


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_over_the_size_pitch_and_alignment_matrix(zj, ctx, torch, chw):
    """1152 images in one call (nine launches): every width, height, pitch and base of the matrix"""
    stage_call(zj, ctx, torch, np.random.default_rng(31 + chw), ec.matrix(), chw)


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_stage_129_images_of_mixed_sizes(zj, ctx, torch, chw):
    rng = np.random.default_rng(77 + chw)
    stage_call(zj, ctx, torch, rng, ec.mixed_129(rng), chw)


def test_stage_tight_pitches_by_default_and_the_tensor_wrapper(zj, tz, ctx, torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    planes = [torch.randint(0, 256, (h, w), dtype=torch.uint8, device="cuda", generator=g) for w, h in ((17, 9), (130, 3), (1, 1))]
    strided = torch.randint(0, 256, (9, 40), dtype=torch.uint8, device="cuda", generator=g)[:, 3:36]  # rows at a pitch of 40
    planes.append(strided)
    for layout in ("HWC", "CHW"):
        outs = tz.gray_to_rgb_tensor(ctx, planes, layout)
        torch.cuda.synchronize()
        for p, o in zip(planes, outs):
            want = p[None].expand(3, -1, -1) if layout == "CHW" else p[..., None].expand(-1, -1, 3)
            assert o.is_contiguous() and torch.equal(o, want)


def test_stage_argument_errors_launch_nothing(zj, ctx, torch):
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = zj.lib()

    def call(n, ins, wh, ip, layout, outs, op):
        arr = lambda v: (C.c_void_p * len(v))(*v) if v is not None else None
        u = lambda v: (C.c_uint * len(v))(*v) if v is not None else None
        return L.zj_gray_to_rgb_device(ctx.handle, n, arr(ins), u(wh), u(ip), layout, arr(outs), u(op), None)

    i, o = src.data_ptr(), dst.data_ptr()
    assert call(2, [i, i], [4, 4, 0, 4], None, 0, [o, o + 64], None) == ERR_ARG      # an empty image behind a good one
    assert call(1, [i], [4, 4], [3], 0, [o], None) == ERR_ARG                        # a pitch below a row
    assert call(1, [i], [4, 4], None, 0, [o], [11]) == ERR_ARG
    assert call(1, [i], [4, 4], None, 1, [o], [3]) == ERR_ARG
    assert call(1, [i], [4, 4], None, 2, [o], None) == ERR_ARG                       # not a layout
    assert call(1, [i], [65536, 1], None, 0, [o], None) == ERR_ARG
    assert call(2, [i, None], [4, 4, 4, 4], None, 0, [o, o + 64], None) == ERR_ARG
    assert call(0, [i], [4, 4], None, 0, [o], None) == ERR_ARG
    ctx.sync()
    assert bool((dst == FILL).all())
    assert call(1, [i], [4, 4], None, 0, [o], None) == 0
    ctx.sync()
    assert bool((dst[:48] == 0).all()) and bool((dst[48:] == FILL).all())


# ---- 2. frames --------------------------------------------------------------------------------------------------------
class Frame:
    """one frame: its descriptor and its planes in device memory; gray: one component, asked for RGB with the flag"""

    def __init__(self, zj, torch, synth, w, h, mode, layout, seed, gray=False, flags=0, cs=None):
        hs, vs = (1, 1) if gray else MODES[mode]
        ncomp = 1 if gray else 3
        planes, qts = synth.make_frame(w, h, hs, vs, ncomp, seed=seed, quality=40 + 5 * (seed % 10))
        self.desc = zj.FrameDesc.make(w, h, hs, vs, ncomp, zj.ColorSpace.RGB if cs is None else cs, qts,
                                      flags=flags | (zj.FLAG_GRAY_TO_RGB if gray else 0), out_layout=layout)
        self.planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]
        self.w, self.h, self.gray = w, h, gray

    def ptr(self, c):
        return self.planes[c].data_ptr() if c < len(self.planes) else None


def tdtype(torch, name):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}[name]


def filled(torch, n, size, dtype, layout):
    ow, oh = size
    shape = (n, 3, oh, ow) if layout == "NCHW" else (n, oh, ow, 3)
    numel = int(np.prod(shape))
    raw = torch.full((numel * torch.empty((), dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device="cuda")
    return raw, raw.view(dtype).view(shape)


FILTERS = {"bilinear": (False, "bilinear"), "aa": (True, "bilinear"), "bicubic": (True, "bicubic")}
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def gray_chain(zj, tz, ctx, torch, f, win, o, flip, size, dt, layout, filt, max_prescale):
    """frame f's image from the stages the library had before: GRAYSCALE crop -> orient -> three channels -> resize"""
    d = copy.copy(f.desc)
    d.out_colorspace = int(zj.ColorSpace.GRAYSCALE)
    d.flags = f.desc.flags & ~zj.FLAG_GRAY_TO_RGB
    st = om.stored_window(o, f.w, f.h, win)
    k = sm.prescale_log2(win[2], win[3], size[0], size[1], {1: 0, 2: 1, 4: 2, 8: 3}[max_prescale])
    if k:
        rw = sm.reduced_window(st[0], st[1], st[2], st[3], k, f.w, f.h)
        crop = torch.full((rw[3], rw[2]), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.decode_crops_scaled_device(d, [f.ptr(0)], None, None, 1 << k, [crop.data_ptr()], [rw])
    else:
        crop = torch.full((st[3], st[2]), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.decode_crops_device(d, [f.ptr(0)], None, None, [(st[0], st[1])], st[2], st[3], [crop.data_ptr()])
    ch, cw = crop.shape
    dw, dh = om.oriented_size(o, cw, ch)
    shown = torch.empty((dh, dw), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.orient_device([crop.data_ptr()], [(cw, ch)], 1, zj.LAYOUT_HWC, [o], [shown.data_ptr()])
    ctx.sync()
    chw = f.desc.out_layout == zj.LAYOUT_CHW
    e = (shown[None].expand(3, -1, -1) if chw else shown[..., None].expand(-1, -1, 3)).contiguous()
    _, one = filled(torch, 1, size, dt, layout)
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    torch.cuda.synchronize()
    ctx.resize_device([e.data_ptr()], [(dw, dh)], 3, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, size[0], size[1],
                      tz._resize_dtype(dt), zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, one.data_ptr(), scale, bias,
                      [flip], None, None, FILTERS[filt][0], FILTERS[filt][1])
    ctx.sync()
    return k, one[0]


def mixed_call(zj, tz, ctx, torch, frames, wins, oris, flips, size, dt, layout, filt, max_prescale):
    n = len(frames)
    raw, out = filled(torch, n, size, dt, layout)
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    torch.cuda.synchronize()
    ctx.decode_crops_resized_mixed_device([f.desc for f in frames], [f.ptr(0) for f in frames], [f.ptr(1) for f in frames],
                                          [f.ptr(2) for f in frames], wins, size[0], size[1], tz._resize_dtype(dt),
                                          zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, out.data_ptr(), scale, bias,
                                          flips, None, FILTERS[filt][0], max_prescale, oris, FILTERS[filt][1])
    ctx.sync()
    return out


def interleaved_frames(zj, torch, synth, layout):
    """gray frames with the flag between colour frames of all four sampling modes; sizes 48 x 40, 33 x 17, 100 x 75, 16 x 16.
    (33 pixels is no width of a gray frame: its GRAYSCALE decode is ZJ_ERR_PANIC, see the status tests.)
    Per frame: (frame, orientation, displayed window, flip)."""
    F = lambda *a, **k: Frame(zj, torch, synth, *a, **k)
    return [
        (F(48, 40, None, layout, 1, gray=True), 1, (0, 0, 48, 40), False),
        (F(100, 75, "420", layout, 2), 1, (3, 2, 90, 70), True),
        (F(100, 75, None, layout, 3, gray=True, flags=zj.FLAG_CLAMP_DC), 6, (0, 0, 75, 100), False),   # prescale_pick 2 at 8
        (F(16, 16, "444", layout, 4), 2, (0, 0, 16, 16), False),
        (F(16, 16, None, layout, 5, gray=True), 2, (1, 0, 15, 16), True),
        (F(48, 40, "420", layout, 6), 1, (0, 30, 48, 10), False),                                        # rows below rows_covered
        (F(48, 40, None, layout, 7, gray=True), 6, (5, 7, 31, 37), True),
        (F(33, 17, "422", layout, 8), 6, (0, 0, 17, 33), False),
        (F(100, 75, None, layout, 9, gray=True), 1, (0, 0, 100, 75), False),                             # prescale_pick 3 at 8
        (F(33, 17, "440", layout, 10, flags=zj.FLAG_CORRECTED), 1, (2, 1, 30, 15), True),
        (F(16, 16, None, layout, 11, gray=True), 1, (4, 4, 1, 1), False),
    ]


@pytest.mark.parametrize("crop_layout", [0, 1], ids=["HWC", "CHW"])
@pytest.mark.parametrize("filt", ["bilinear", "aa", "bicubic"])
def test_mixed_call_gray_frames_between_colour_frames(zj, tz, ctx, torch, synth, filt, crop_layout):
    spec = interleaved_frames(zj, torch, synth, crop_layout)
    frames, oris, wins, flips = [list(v) for v in zip(*spec)]
    colour = [i for i, f in enumerate(frames) if not f.gray]
    size = (12, 9)
    seen_k = set()
    for dtype, layout, max_prescale in (("u8", "NCHW", 1), ("bf16", "NHWC", 8), ("f32", "NCHW", 8), ("u8", "NHWC", 8)):
        dt = tdtype(torch, dtype)
        out = mixed_call(zj, tz, ctx, torch, frames, wins, oris, flips, size, dt, layout, filt, max_prescale)
        for i, f in enumerate(frames):
            if not f.gray:
                continue
            k, want = gray_chain(zj, tz, ctx, torch, f, wins[i], oris[i], flips[i], size, dt, layout, filt, max_prescale)
            seen_k.add(k)
            assert torch.equal(out[i].view(torch.uint8), want.view(torch.uint8)), \
                f"gray frame {i} ({f.w}x{f.h}, o {oris[i]}, window {wins[i]}, scale {k}) differs from its stages run one by one"
            if dtype == "u8":
                px = out[i] if layout == "NHWC" else out[i].permute(1, 2, 0)
                assert torch.equal(px[..., 0], px[..., 1]) and torch.equal(px[..., 0], px[..., 2])
        # the colour frames: the same call without the gray frames
        pick = lambda v: [v[i] for i in colour]
        alone = mixed_call(zj, tz, ctx, torch, pick(frames), pick(wins), pick(oris), pick(flips), size, dt, layout, filt, max_prescale)
        assert torch.equal(out[colour].view(torch.uint8), alone.view(torch.uint8)), "a colour frame changed beside gray frames"
    assert seen_k == {0, 1, 2, 3}


@pytest.mark.parametrize("crop_layout", [0, 1], ids=["HWC", "CHW"])
def test_one_geometry_call_with_an_all_gray_descriptor(zj, tz, ctx, torch, synth, crop_layout):
    """six frames of ONE gray descriptor with the flag through zj_decode_crops_resized_oriented_device"""
    w, h, size = 100, 75, (12, 9)
    base = Frame(zj, torch, synth, w, h, None, crop_layout, 20, gray=True)
    frames = [base]
    for s in range(21, 26):
        f = Frame(zj, torch, synth, w, h, None, crop_layout, s, gray=True)
        f.desc = base.desc  # (one descriptor: the first frame's tables)
        frames.append(f)
    oris = [1, 6, 2, 1, 6, 2]
    wins = [(0, 0, 100, 75), (0, 0, 75, 100), (7, 3, 50, 40), (99, 74, 1, 1), (5, 9, 30, 80), (0, 0, 100, 75)]
    flips = [False, True, False, True, False, True]
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    for filt, dtype, layout, max_prescale in (("bilinear", "f32", "NCHW", 1), ("aa", "u8", "NHWC", 8), ("bicubic", "bf16", "NCHW", 8)):
        dt = tdtype(torch, dtype)
        raw, out = filled(torch, len(frames), size, dt, layout)
        torch.cuda.synchronize()
        ctx.decode_crops_resized_device(base.desc, [f.ptr(0) for f in frames], None, None, wins, size[0], size[1],
                                        tz._resize_dtype(dt), zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC,
                                        out.data_ptr(), scale, bias, flips, None, FILTERS[filt][0], max_prescale, oris,
                                        FILTERS[filt][1])
        ctx.sync()
        for i, f in enumerate(frames):
            k, want = gray_chain(zj, tz, ctx, torch, f, wins[i], oris[i], flips[i], size, dt, layout, filt, max_prescale)
            assert torch.equal(out[i].view(torch.uint8), want.view(torch.uint8)), (filt, dtype, layout, max_prescale, i, k)
    # ... and through the tensor wrapper without orientations (the prescaled entry point)
    t = tz.decode_resized_crops_to_tensor(ctx, base.desc, [(f.planes[0], None, None) for f in frames[:2]],
                                          [(0, 0, 100, 75), (7, 3, 50, 40)], size, dtype=torch.uint8, layout="NHWC")
    torch.cuda.synchronize()
    assert t.shape == (2, 9, 12, 3) and torch.equal(t[..., 0], t[..., 1]) and torch.equal(t[..., 0], t[..., 2])


# ---- 3. files ---------------------------------------------------------------------------------------------------------
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


def mixed_files():
    """(blob, is gray): gray baseline, gray progressive and a gray file with EXIF orientation 6 among colour files"""
    return [(pillow_file(96, 72, 1, False), False), (pillow_file(80, 56, 2, True), True),
            (pillow_file(97, 61, 3, False, subsampling="4:4:4", orientation=6), False),
            (pillow_file(104, 88, 4, True, progressive=True), True), (pillow_file(72, 120, 5, True, orientation=6), True),
            (pillow_file(64, 48, 6, False, progressive=True, subsampling="4:2:2"), False), (pillow_file(45, 31, 7, True), True)]


def options(zj, entropy="ENTROPY_CPU", cs=None, flag=True):
    o = zj.ZuneJpegOptions()
    o.entropy = getattr(zj, entropy)
    o.flags = zj.FLAG_GRAY_TO_RGB if flag else 0
    if cs is not None:
        o.out_colorspace = cs
    return o


def single_file(zj, tz, ctx, torch, blob, opt, win, size, dt, layout, channels, flip=False, antialias=False, max_prescale=1):
    dec = zj.Decoder(opt, ctx)
    _, info = dec.prepare(blob)
    if win is None:
        win = (0, 0) + tuple(zj.oriented_size(dec.orientation, int(info.width), int(info.height)))
    ow, oh = size
    one = torch.full((channels, oh, ow) if layout == "NCHW" else (oh, ow, channels), 0, dtype=dt, device="cuda")
    scale, bias = tz.normalize_factors(channels, None, None)
    torch.cuda.synchronize()
    n = dec.finish_pixels_resized_crop_device(win[0], win[1], win[2], win[3], ow, oh, tz._resize_dtype(dt),
                                              zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC, one.data_ptr(),
                                              one.numel() * one.element_size(), scale, bias, flip, antialias, max_prescale, True)
    dec.close()
    assert n == one.numel() * one.element_size(), "*out_len is not the slot's size"
    return one


@pytest.mark.parametrize("workers", [1, 4])
def test_gray_files_among_colour_files(zj, tz, ctx, torch, workers):
    files = mixed_files()
    blobs = [b for b, _ in files]
    opt = options(zj)
    size = (16, 12)
    wins = [None, None, (3, 5, 40, 30), None, (2, 1, 100, 60), None, (1, 1, 40, 29)]
    flips = [k % 3 == 1 for k in range(len(blobs))]
    for dt, layout, antialias, max_prescale in ((torch.uint8, "NHWC", False, 1), (torch.float32, "NCHW", True, 4)):
        out = tz.decode_files_resized_to_tensor(ctx, blobs, wins, size, dtype=dt, layout=layout, flips=flips, antialias=antialias,
                                                max_prescale=max_prescale, apply_orientation=True, options=opt, workers=workers)
        torch.cuda.synchronize()
        for k, (blob, gray) in enumerate(files):
            one = single_file(zj, tz, ctx, torch, blob, opt, wins[k], size, dt, layout, 3, flips[k], antialias, max_prescale)
            assert torch.equal(out[k].view(torch.uint8), one.view(torch.uint8)), f"file {k} differs from the single-file call"
            if gray and dt == torch.uint8:
                assert torch.equal(out[k][..., 0], out[k][..., 1]) and torch.equal(out[k][..., 0], out[k][..., 2])
                g = single_file(zj, tz, ctx, torch, blob, options(zj, cs=zj.ColorSpace.GRAYSCALE, flag=False), wins[k], size, dt,
                                layout, 1, flips[k], antialias, max_prescale)
                assert torch.equal(out[k][..., 0], g[..., 0]), f"gray file {k} is not its GRAYSCALE decode in every channel"
        # the colour files: what a batch without the flag and without the gray files gives
        colour = [k for k, (_, gray) in enumerate(files) if not gray]
        pick = lambda v: [v[k] for k in colour]
        alone = tz.decode_files_resized_to_tensor(ctx, pick(blobs), pick(wins), size, dtype=dt, layout=layout, flips=pick(flips),
                                                  antialias=antialias, max_prescale=max_prescale, apply_orientation=True,
                                                  options=options(zj, flag=False), workers=workers)
        torch.cuda.synchronize()
        assert torch.equal(out[colour].view(torch.uint8), alone.view(torch.uint8))


def test_gray_files_with_the_scan_left_for_the_device(zj, tz, ctx, torch):
    """ENTROPY_GPU_ALWAYS: the baseline files keep their scan for the device and take the single-file call inside the batch"""
    files = mixed_files()
    blobs = [b for b, _ in files]
    size = (16, 12)
    kw = dict(dtype=torch.uint8, layout="NHWC", apply_orientation=True, max_prescale=2)
    cpu = tz.decode_files_resized_to_tensor(ctx, blobs, None, size, options=options(zj), **kw)
    opt = options(zj, "ENTROPY_GPU_ALWAYS")
    dev = tz.decode_files_resized_to_tensor(ctx, blobs, None, size, options=opt, **kw)
    torch.cuda.synchronize()
    assert torch.equal(cpu, dev)
    for k, (blob, gray) in enumerate(files):
        one = single_file(zj, tz, ctx, torch, blob, opt, None, size, torch.uint8, "NHWC", 3, max_prescale=2)
        assert torch.equal(dev[k], one), f"file {k}"


# ---- 4. unchanged without the flag; status codes --------------------------------------------------------------------------
def raw_mixed(zj, ctx, frames, descs, wins, out, oris=None, max_k=0):
    n = len(frames)
    arr = lambda c: (C.c_void_p * n)(*[f.ptr(c) for f in frames])
    rc = zj.lib().zj_decode_crops_resized_mixed_device(
        ctx.handle, (zj.FrameDesc * n)(*descs), n, arr(0), arr(1), arr(2), (C.c_uint * (4 * n))(*[v for w in wins for v in w]),
        8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, None, None, None, zj.RESIZE_BILINEAR, max_k,
        (C.c_uint8 * n)(*oris) if oris else None, out.data_ptr(), None)
    ctx.sync()
    return rc


def test_without_the_flag_nothing_changes(zj, tz, ctx, torch, synth):
    g = Frame(zj, torch, synth, 48, 40, None, 0, 30, gray=True)
    raw, out = filled(torch, 1, (8, 8), torch.float32, "NCHW")
    torch.cuda.synchronize()
    # a one-component descriptor that asks for RGB, no flag: the frame calls refuse it as they did (zj_plan.h: make_plan), in
    # both forms, and write nothing
    plain = copy.copy(g.desc)
    plain.flags = 0
    assert raw_mixed(zj, ctx, [g], [plain], [(0, 0, 48, 40)], out) == ERR_UNSUPPORTED
    with pytest.raises(zj.ZjError) as e:
        ctx.decode_crops_resized_device(plain, [g.ptr(0)], None, None, [(0, 0, 48, 40)], 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, out.data_ptr())
    assert e.value.status == ERR_UNSUPPORTED
    ctx.sync()
    assert bool((raw == FILL).all())
    assert zj.resized_out_len(plain, 8, 8, zj.DTYPE_F32) == 3 * 64 * 4  # (the all-zero output's length, as before)
    # the flag on every other entry point: an unknown bit, ZJ_ERR_ARG -- on the one-component RGB descriptor itself the
    # status such a descriptor has there with or without it (ZJ_ERR_UNSUPPORTED: the colour space is looked at first)
    crop = torch.full((3 * 16 * 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c = Frame(zj, torch, synth, 48, 40, "420", 0, 31, flags=zj.FLAG_GRAY_TO_RGB)
    gg = Frame(zj, torch, synth, 48, 40, None, 0, 30, gray=True, cs=zj.ColorSpace.GRAYSCALE)
    for f in (c, gg):
        cb, cr = ([f.ptr(1)], [f.ptr(2)]) if f.ptr(1) else (None, None)
        with pytest.raises(zj.ZjError) as e:
            ctx.decode_crops_device(f.desc, [f.ptr(0)], cb, cr, [(0, 0)], 16, 16, [crop.data_ptr()])
        assert e.value.status == ERR_ARG
        with pytest.raises(zj.ZjError) as e:
            ctx.decode_crops_scaled_device(f.desc, [f.ptr(0)], cb, cr, 2, [crop.data_ptr()], [(0, 0, 16, 16)])
        assert e.value.status == ERR_ARG
    for d in (g.desc, plain):
        with pytest.raises(zj.ZjError) as e:
            ctx.decode_crops_device(d, [g.ptr(0)], None, None, [(0, 0)], 16, 16, [crop.data_ptr()])
        assert e.value.status == ERR_UNSUPPORTED
    ctx.sync()
    assert bool((crop == FILL).all())
    # a three-component frame: the flag does nothing
    a = mixed_call(zj, tz, ctx, torch, [c], [(0, 0, 48, 40)], [1], [False], (8, 8), torch.float32, "NCHW", "aa", 2)
    c.desc.flags = 0
    b = mixed_call(zj, tz, ctx, torch, [c], [(0, 0, 48, 40)], [1], [False], (8, 8), torch.float32, "NCHW", "aa", 2)
    assert torch.equal(a, b)
    # a gray file without the flag: one channel in the first third of its slot, the rest of the slot not written
    blob = pillow_file(80, 56, 2, True)
    dec = zj.Decoder(options(zj, flag=False), ctx)
    dec.prepare(blob)
    slot = torch.full((3 * 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = dec.finish_pixels_resized_crop_device(0, 0, 80, 56, 8, 8, zj.DTYPE_U8, zj.TENSOR_NCHW, slot.data_ptr(), slot.numel())
    dec.close()
    assert n == 64 and bool((slot[64:] == FILL).all())


def test_status_codes(zj, tz, ctx, torch, synth):
    frames = [Frame(zj, torch, synth, 48, 40, "420", 0, 40), Frame(zj, torch, synth, 48, 40, None, 0, 41, gray=True),
              Frame(zj, torch, synth, 16, 16, "444", 0, 42)]
    descs = [f.desc for f in frames]
    wins = [(0, 0, 48, 40), (0, 0, 48, 40), (0, 0, 16, 16)]
    raw, out = filled(torch, 3, (8, 8), torch.float32, "NCHW")
    torch.cuda.synchronize()
    # a bad gray window in the middle: the single-frame status, nothing launched
    bad = list(wins)
    bad[1] = (1, 0, 48, 40)
    assert raw_mixed(zj, ctx, frames, descs, bad, out) == ERR_ARG
    assert raw_mixed(zj, ctx, frames, descs, wins, out, oris=[1, 9, 1]) == ERR_ARG
    # YCbCr with the flag and one component: not supported, in the mixed call (all descriptors YCbCr), the one-geometry call
    # and the decoder
    ycc = [copy.copy(d) for d in descs]
    for d in ycc:
        d.out_colorspace = int(zj.ColorSpace.YCbCr)
    assert raw_mixed(zj, ctx, frames, ycc, wins, out) == ERR_UNSUPPORTED
    with pytest.raises(zj.ZjError) as e:
        ctx.decode_crops_resized_device(ycc[1], [frames[1].ptr(0)], None, None, [wins[1]], 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW,
                                        out.data_ptr())
    assert e.value.status == ERR_UNSUPPORTED
    # a gray frame 33 pixels wide: its GRAYSCALE decode is ZJ_ERR_PANIC (zj_plan.h: make_plan), and so is the frame here --
    # unless every window is taken from a reduced decode, which has no strips
    narrow = Frame(zj, torch, synth, 33, 17, None, 0, 43, gray=True)
    gs = copy.copy(narrow.desc)
    gs.out_colorspace, gs.flags = int(zj.ColorSpace.GRAYSCALE), 0
    assert zj.crop_out_len(gs, 8, 8) == 0
    assert raw_mixed(zj, ctx, frames[:1] + [narrow], descs[:1] + [narrow.desc], [wins[0], (0, 0, 33, 17)], out) == ERR_PANIC
    ctx.sync()
    assert bool((raw == FILL).all()), "a refused call wrote to the output"
    dec = zj.Decoder(options(zj, cs=zj.ColorSpace.YCbCr), ctx)
    dec.prepare(pillow_file(80, 56, 2, True))
    with pytest.raises(zj.DecodeError) as e:
        dec.finish_pixels_resized_crop_device(0, 0, 80, 56, 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, out.data_ptr(), raw.numel())
    assert e.value.status == ERR_UNSUPPORTED
    dec.close()
    assert bool((raw == FILL).all())
    # the capacity check uses three channels
    dec = zj.Decoder(options(zj), ctx)
    dec.prepare(pillow_file(80, 56, 2, True))
    with pytest.raises(zj.DecodeError) as e:
        dec.finish_pixels_resized_crop_device(0, 0, 80, 56, 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, out.data_ptr(), 2 * 64 * 4)
    assert e.value.status == ERR_ARG
    dec.prepare(pillow_file(80, 56, 2, True))  # (a failed call leaves the decoder in its error state)
    assert dec.finish_pixels_resized_crop_device(0, 0, 80, 56, 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, out.data_ptr(), 3 * 64 * 4) == 3 * 64 * 4
    dec.close()
    assert raw_mixed(zj, ctx, frames, descs, wins, out) == 0 and not bool((raw[3 * 64 * 4:] == FILL).all())
