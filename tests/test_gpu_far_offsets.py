"""GPU: byte offsets past 2^31 and 2^32 in every device stage and decode path (far_cases.py; the CPU side of the same cases is
test_far_offsets_emu.py, which must pass on the same tree first).
a. the pitched u8 stages and the tensor stages' inputs at pitches up to 2^24: row x pitch, plane x pitch x height
b. the frame, crop and reduced decode at output pitches up to 2^20, with the rows each path zeroes
c. the strided batch: frame x stride
d. one launch whose last slot starts past 2^32: slot x image bytes, in the three resizes, to-tensor and warp
e. one image of 4.3 GB: element x size, in to-tensor and the crop-tensor decode
The buffers are device tensors full of a poison byte; only the images' own rows are read back, the padding is compared on
the device.  Every test asserts that the largest offset it makes a kernel form is past the line it is about."""
import ctypes as C
import functools
import importlib
import math

import numpy as np
import pytest

import far_cases as fc
import oracle_c as oc
import test_far_offsets_emu as fe

pytestmark = pytest.mark.gpu
POISON = 0xA5
ERR_ARG = -1
GB = 1 << 30

PITCHES = pytest.mark.parametrize("pitch", fc.STAGE_PITCHES, ids=["limit", "odd"])
LAYOUTS = pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
OUT_PITCH = pytest.mark.parametrize("which", [0, 1], ids=["limit", "below"])


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


@pytest.fixture(autouse=True)
def release(torch, request):
    """every test's gigabytes go back to the device before the next one asks for its own; its peak goes into the report
    (--junitxml) as the property peak_device_gb"""
    torch.cuda.reset_peak_memory_stats()
    yield
    request.node.user_properties.append(("peak_device_gb", round(torch.cuda.max_memory_allocated() / GB, 2)))
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def need(torch, nbytes):
    """skip only when the device has not the memory free that the test is about to take"""
    free, _ = torch.cuda.mem_get_info()
    assert nbytes < 20 * GB, "a test of this file stays under 20 GB"
    if free < nbytes + GB:
        pytest.skip(f"{free / GB:.1f} GB of device memory free, {nbytes / GB:.1f} GB + 1 GB needed")


class DevFar:
    """far_cases.Far on the device: `planes` planes of h rows of row_bytes bytes, pitch apart, in a tensor full of POISON"""

    def __init__(self, torch, planes, h, row_bytes, pitch, fill=POISON):
        self.torch, self.planes, self.h, self.row_bytes, self.pitch = torch, planes, h, row_bytes, pitch
        self.t = torch.full((planes * h * pitch,), fill, dtype=torch.uint8, device="cuda")
        self.rows = self.t.view(planes, h, pitch)[:, :, :row_bytes]

    @property
    def ptr(self):
        return self.t.data_ptr()

    def put(self, rows):
        self.rows.copy_(self.torch.from_numpy(np.ascontiguousarray(rows).reshape(self.planes, self.h, self.row_bytes)))
        return self

    def get(self):
        return self.rows.cpu().numpy()

    def padding(self):
        """per row (through the planes): is its padding all POISON, is it all zero -- compared on the device, 512 MB at a time"""
        flat = self.t.view(self.planes * self.h, self.pitch)
        step = max(1, (1 << 29) // self.pitch)
        kept, zeroed = [], []
        for r0 in range(0, flat.shape[0], step):
            pad = flat[r0:r0 + step, self.row_bytes:]
            kept.append((pad == POISON).all(dim=1))
            zeroed.append((pad == 0).all(dim=1))
        return self.torch.cat(kept).cpu().numpy(), self.torch.cat(zeroed).cpu().numpy()

    def padding_untouched(self):
        return bool(self.padding()[0].all())


def assert_rows(got, want, pitch, what):
    got = got.reshape(-1, got.shape[-1])
    want = np.asarray(want).reshape(got.shape)
    for r in fc.lines(pitch, got.shape[0]):
        assert np.array_equal(got[r], want[r]), f"{what}: row {r} (offset {r * pitch:#x}) differs"
    assert np.array_equal(got, want), what


def stage_far(torch, rng, chw, w, pitch):
    """a random far 3-channel image and its bytes: (DevFar, rows [planes, h, row bytes])"""
    npl, h, rb = fe.stage_shape(chw, w)
    rows = rng.integers(0, 256, (npl, h, rb), dtype=np.uint8)
    return DevFar(torch, npl, h, rb, pitch).put(rows), rows


def layout_of(zj, chw):
    return zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC


# ---- a. the pitched stages -----------------------------------------------------------------------------------------------

def test_a_pitch_above_the_limit_is_refused_and_nothing_written(zj, ctx, torch):
    """STAGE_PITCH_MAX + 1 in a stage call and OUT_PITCH_MAX + 16 in the frame call: argument errors (the accepted side of
    both limits is every other test of this file)"""
    buf = torch.full((4096,), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(zj.ZjError) as e:
        ctx.color_device([buf.data_ptr()], [(4, 1)], zj.LAYOUT_HWC, [np.eye(3, 4)], [buf.data_ptr() + 2048], [fc.STAGE_PITCH_MAX + 1], None)
    assert e.value.status == ERR_ARG
    with pytest.raises(zj.ZjError) as e:
        ctx.gray_to_rgb_device([buf.data_ptr()], [(4, 1)], zj.LAYOUT_HWC, [buf.data_ptr() + 2048], None, [fc.STAGE_PITCH_MAX + 1])
    assert e.value.status == ERR_ARG
    qts = [np.ones(64, np.uint16)] * 3
    d = zj.FrameDesc.make(48, 8, 1, 1, 3, zj.ColorSpace.RGB, qts, out_pitch=fc.OUT_PITCH_MAX + 16)
    with pytest.raises(zj.ZjError) as e:
        ctx.decode_planes_device(d, 1, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.status == ERR_ARG
    ctx.sync()
    assert bool((buf == POISON).all())


@pytest.mark.parametrize("o", range(1, 9))
@LAYOUTS
@PITCHES
def test_orient(zj, ctx, torch, pitch, chw, o):
    import orient_model as om
    H = fc.STAGE_H_CHW if chw else fc.STAGE_H_HWC
    bpp, npl = (1, 3) if chw else (3, 1)
    rng = np.random.default_rng(100 + o)
    for w, h in ((37, H), (H, 37)) if o >= 5 else ((37, H),):
        dw, dh = om.oriented_size(o, w, h)
        assert fc.crosses(pitch, max(h, dh), npl), "no offset of this case reaches 2^32"
        need(torch, npl * (h + dh) * pitch)
        rows = rng.integers(0, 256, (npl, h, w * bpp), dtype=np.uint8)
        src = DevFar(torch, npl, h, w * bpp, pitch).put(rows)
        dst = DevFar(torch, npl, dh, dw * bpp, pitch)
        torch.cuda.synchronize()
        ctx.orient_device([src.ptr], [(w, h)], 3, layout_of(zj, chw), [o], [dst.ptr], [pitch], [pitch])
        ctx.sync()
        img = rows if chw else rows[0].reshape(h, w, 3)
        want = om.orient_chw(img, o) if chw else om.orient(img, o)
        what = f"orient {o} stored {w}x{h} pitch {pitch}"
        assert_rows(dst.get(), fe.rows_of(want, chw), pitch, what)
        assert dst.padding_untouched() and src.padding_untouched(), f"{what}: a padding byte was written"
        assert np.array_equal(src.get(), rows), f"{what}: the input was written"
        del src, dst
        torch.cuda.empty_cache()


@PITCHES
@LAYOUTS
@pytest.mark.parametrize("w", fc.STAGE_WIDTHS)
def test_gray_to_rgb(zj, ctx, torch, w, chw, pitch):
    npl, h, rb = fe.stage_shape(chw, w)
    assert fc.crosses(pitch, h, npl) and (chw or fc.crosses(pitch, h))
    need(torch, (npl + 1) * h * pitch)
    g = np.random.default_rng(w).integers(0, 256, (1, h, w), dtype=np.uint8)
    src = DevFar(torch, 1, h, w, pitch).put(g)
    dst = DevFar(torch, npl, h, rb, pitch)
    torch.cuda.synchronize()
    ctx.gray_to_rgb_device([src.ptr], [(w, h)], layout_of(zj, chw), [dst.ptr], [pitch], [pitch])
    ctx.sync()
    want = np.stack([g[0]] * 3) if chw else np.repeat(g[0], 3, axis=1)
    assert_rows(dst.get(), want, pitch, "gray to RGB")
    assert dst.padding_untouched() and src.padding_untouched()


@PITCHES
@LAYOUTS
@pytest.mark.parametrize("w", fc.STAGE_WIDTHS)
def test_cmyk(zj, ctx, torch, w, chw, pitch):
    import cmyk_stage_cases as sc
    npl, h, rb = fe.stage_shape(chw, w)
    assert fc.crosses(pitch, h, npl)
    need(torch, (2 * npl + 1) * h * pitch)
    rng = np.random.default_rng(w + 1)
    a, arows = stage_far(torch, rng, chw, w, pitch)
    krows = rng.integers(0, 256, (1, h, w), dtype=np.uint8)
    k = DevFar(torch, 1, h, w, pitch).put(krows)
    dst = DevFar(torch, npl, h, rb, pitch)
    for inverted in (0, 1):
        torch.cuda.synchronize()
        ctx.cmyk_to_rgb_device([a.ptr], [k.ptr], [(w, h)], layout_of(zj, chw), [dst.ptr], [inverted], [pitch], [pitch], [pitch])
        ctx.sync()
        img = arows if chw else arows[0].reshape(h, w, 3)
        want = sc.combine(img, krows if chw else krows[0][:, :, None], inverted).astype(np.uint8)
        assert_rows(dst.get(), fe.rows_of(want, chw), pitch, f"cmyk inverted {inverted}")
        assert dst.padding_untouched()
    assert a.padding_untouched() and k.padding_untouched() and np.array_equal(a.get(), arows)


@PITCHES
@LAYOUTS
def test_planes(zj, ctx, torch, chw, pitch):
    import planes_cases as pc
    w = 37
    npl, h, rb = fe.stage_shape(chw, w)
    geo = ((1, 1, 0, 0), (2, 1, 0, 0), (4, 2, 0, 0))        # (the public call has no phases: the planes begin with the image)
    sizes = [pc.plane_size(w, h, g) for g in geo]
    assert fc.crosses(pitch, h, npl) and fc.crosses(pitch, sizes[1][1], 1, fc.LINE31)
    assert chw or fc.crosses(pitch, sizes[1][1])            # (the third plane, half as tall, ends around 2^31)
    need(torch, (sum(ph for _, ph in sizes) + npl * h) * pitch)
    rng = np.random.default_rng(9)
    host = [rng.integers(0, 256, (ph, pw), dtype=np.uint8) for pw, ph in sizes]
    dev = [DevFar(torch, 1, ph, pw, pitch).put(p) for (pw, ph), p in zip(sizes, host)]
    dst = DevFar(torch, npl, h, rb, pitch)
    ratios = tuple((g[0], g[1]) for g in geo)
    for stored_rgb in (False, True):
        torch.cuda.synchronize()
        ctx.planes_to_rgb_device([dev[0].ptr], [dev[1].ptr], [dev[2].ptr], [(w, h)], [ratios], layout_of(zj, chw), [dst.ptr],
                                 stored_rgb=stored_rgb, pitches=[(pitch,) * 3], out_pitches=[pitch])
        ctx.sync()
        e = pc.combine(host, geo, w, h, stored_rgb).reshape(h, w, 3)
        assert_rows(dst.get(), e.transpose(2, 0, 1) if chw else e.reshape(1, h, 3 * w), pitch, f"planes stored_rgb {stored_rgb}")
        assert dst.padding_untouched()
    assert all(d.padding_untouched() for d in dev)


@PITCHES
@LAYOUTS
@pytest.mark.parametrize("w", fc.STAGE_WIDTHS)
def test_color(zj, ctx, torch, w, chw, pitch):
    import color_cases as cc
    import color_model as cm
    npl, h, rb = fe.stage_shape(chw, w)
    assert fc.crosses(pitch, h, npl)
    need(torch, 2 * npl * h * pitch)
    src, rows = stage_far(torch, np.random.default_rng(w + 2), chw, w, pitch)
    dst = DevFar(torch, npl, h, rb, pitch)
    m = cc.jitter()
    want = fe.rows_of(cm.apply(m, rows if chw else rows[0].reshape(h, w, 3), chw), chw)
    torch.cuda.synchronize()
    ctx.color_device([src.ptr], [(w, h)], layout_of(zj, chw), [m], [dst.ptr], [pitch], [pitch])
    ctx.sync()
    assert_rows(dst.get(), want, pitch, "colour, apart")
    assert dst.padding_untouched() and src.padding_untouched() and np.array_equal(src.get(), rows)
    ctx.color_device([src.ptr], [(w, h)], layout_of(zj, chw), [m], [src.ptr], [pitch], [pitch])
    ctx.sync()
    assert_rows(src.get(), want, pitch, "colour, in place")
    assert src.padding_untouched()


def _norm(ch):
    return np.float32([0.02, 0.015, 0.01])[:ch], np.float32([-1.5, 0.25, 2.0])[:ch]


@PITCHES
@pytest.mark.parametrize("kind", ["bilinear", "antialiased", "bicubic"])
@LAYOUTS
def test_resize_inputs(zj, ctx, torch, chw, kind, pitch):
    """HWC at 258 rows.  A CHW input is taken up to 2^31 bytes in all (zj_resize_filtered_device's own rule), which at these
    pitches is 42 rows a plane: the third plane's last row ends just below that line, and one row more is refused.  (The
    emulation runs the kernels' headers over CHW planes of 130 rows: test_far_offsets_emu.py.)"""
    import resize_model as rm
    model = importlib.import_module({"bilinear": "resize_model", "antialiased": "resize_aa_model", "bicubic": "resize_bicubic_model"}[kind])
    w = 37
    npl, h, rb = fe.stage_shape(chw, w)
    if chw:
        h = fc.LINE31 // (3 * pitch)
        assert h == 42 and 3 * h * pitch <= fc.LINE31 < 3 * (h + 1) * pitch
    else:
        assert fc.crosses(pitch, h, npl)
    need(torch, npl * (h + 1) * pitch)
    rows = np.random.default_rng(5).integers(0, 256, (npl, h, rb), dtype=np.uint8)
    src = DevFar(torch, npl, h, rb, pitch).put(rows)
    img = rows if chw else rows[0].reshape(h, w, 3).transpose(2, 0, 1)
    scale, bias = _norm(3)
    kw = dict(scale=scale, bias=bias, pitches=[pitch], antialias=kind != "bilinear", interpolation="bicubic" if kind == "bicubic" else "bilinear")
    for ow, oh in ((29, h), (16, 9)):
        out = torch.full((3 * ow * oh * 4 + 128,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.resize_device([src.ptr], [(w, h)], 3, layout_of(zj, chw), ow, oh, zj.DTYPE_F32, zj.TENSOR_NHWC, out.data_ptr() + 64, **kw)
        ctx.sync()
        got = out.cpu().numpy()
        exp = np.ascontiguousarray(model.resize(img, ow, oh, rm.F32, scale, bias, False, "NHWC")).view(np.uint8).reshape(-1)
        assert np.array_equal(got[64:-64], exp), (kind, ow, oh)
        assert (got[:64] == POISON).all() and (got[-64:] == POISON).all()
    assert src.padding_untouched() and np.array_equal(src.get(), rows)
    if chw:
        taller = torch.empty((3 * (h + 1) * pitch,), dtype=torch.uint8, device="cuda")
        out = torch.empty((3 * 16 * 9 * 4,), dtype=torch.uint8, device="cuda")
        with pytest.raises(zj.ZjError) as e:
            ctx.resize_device([taller.data_ptr()], [(w, h + 1)], 3, zj.LAYOUT_CHW, 16, 9, zj.DTYPE_F32, zj.TENSOR_NHWC, out.data_ptr(), **kw)
        assert e.value.status == ERR_ARG


@PITCHES
@pytest.mark.parametrize("cin,cout", [(1, 3), (3, 3)])
@pytest.mark.parametrize("w", fc.STAGE_WIDTHS)
def test_to_tensor_inputs(zj, ctx, torch, w, cin, cout, pitch):
    import resize_model as rm
    h = fc.STAGE_H_HWC
    assert fc.crosses(pitch, h)
    need(torch, h * pitch)
    rows = np.random.default_rng(w + cin).integers(0, 256, (1, h, w * cin), dtype=np.uint8)
    src = DevFar(torch, 1, h, w * cin, pitch).put(rows)
    scale, bias = _norm(cout)
    chw_img = rows[0].reshape(h, w, cin).transpose(2, 0, 1)
    if cin != cout:
        chw_img = np.repeat(chw_img, cout, axis=0)
    for flip in (False, True):
        out = torch.full((cout * w * h * 4 + 128,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.to_tensor_device([src.ptr], w, h, cin, cout, zj.DTYPE_F32, zj.TENSOR_NHWC, out.data_ptr() + 64, scale=scale, bias=bias,
                             flips=[flip], pitches=[pitch])
        ctx.sync()
        got = out.cpu().numpy()
        exp = np.ascontiguousarray(rm.resize(chw_img, w, h, rm.F32, scale, bias, flip, "NHWC")).view(np.uint8).reshape(-1)
        assert np.array_equal(got[64:-64], exp), (w, cin, cout, flip)
        assert (got[:64] == POISON).all() and (got[-64:] == POISON).all()
    assert src.padding_untouched()


@PITCHES
@pytest.mark.parametrize("ch", [1, 3])
def test_warp_inputs(zj, ctx, torch, ch, pitch):
    import resize_model as rm
    import warp_model as wm
    w, h = 37, fc.STAGE_H_HWC
    assert fc.crosses(pitch, h)
    need(torch, h * pitch)
    rows = np.random.default_rng(ch).integers(0, 256, (1, h, w * ch), dtype=np.uint8)
    src = DevFar(torch, 1, h, w * ch, pitch).put(rows)
    scale, bias = _norm(ch)
    co, si = math.cos(math.radians(17)), math.sin(math.radians(17))
    cx, cy = w / 2, h / 2
    img = rows[0].reshape(h, w, ch)
    fill = (7, 130, 255)
    for m in (wm.orientation_matrix(1, w, h), wm.orientation_matrix(3, w, h), (co, -si, cx - co * cx + si * cy, si, co, cy - si * cx - co * cy)):
        q = wm.fixed(m)
        assert q is not None
        out = torch.full((ch * w * h * 4 + 128,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.warp_device([src.ptr], [(w, h)], ch, [m], w, h, zj.DTYPE_F32, zj.TENSOR_NHWC, out.data_ptr() + 64, scale=scale, bias=bias,
                        fill=fill[:ch], edge="fill", pitches=[pitch])
        ctx.sync()
        got = out.cpu().numpy()
        exp = np.ascontiguousarray(wm.warp(img, q, w, h, rm.F32, scale, bias, wm.FILL, fill, "NHWC")).view(np.uint8).reshape(-1)
        assert np.array_equal(got[64:-64], exp), m
        assert (got[:64] == POISON).all() and (got[-64:] == POISON).all()
    assert src.padding_untouched()


# ---- b. the decode paths at output pitches up to 1 MiB ---------------------------------------------------------------------

def upload(torch, planes):
    return [torch.from_numpy(np.ascontiguousarray(p, np.int16)).cuda() for p in planes]


def cs_of(zj, kind):
    return zj.ColorSpace.GRAYSCALE if kind == "gray" else zj.ColorSpace.RGB


def check_decode(far, want, pitch, zero_rows, whole, what):
    """the rows equal the oracle's; the rows below the last complete strip are zero and lie past 2^32; the padding is
    untouched -- but for those rows where the frame call zeroes them whole (Q6, test_gpu_pitch.py)"""
    got = far.get()
    assert_rows(got, want, pitch, what)
    kept, zeroed = far.padding()
    if zero_rows:
        flat = got.reshape(-1, got.shape[-1])
        assert not flat[zero_rows].any() and max(zero_rows) * pitch >= fc.LINE32, f"{what}: the zeroed rows"
    if whole:   # a row's padding is untouched, or zeroed with the row where that row is one the strips never reach
        assert (kept | zeroed).all() and np.delete(kept, zero_rows).all(), f"{what}: a padding byte was written"
    else:
        assert kept.all(), f"{what}: a padding byte was written"


@OUT_PITCH
@pytest.mark.parametrize("w", fc.OUT_WIDTHS)
@pytest.mark.parametrize("kind", fe.KINDS)
@pytest.mark.parametrize("mode", list(fe.MODES))
def test_frame_decode(zj, ctx, torch, synth, mode, kind, w, which):
    hs, vs = fe.MODES[mode]
    npl, h, rb = fe.out_shape(kind, w)
    pitch = fc.out_pitches(w)[which]
    planes, qts = synth.make_frame(w, h, hs, vs, 3, seed=w + h)
    d = zj.FrameDesc.make(w, h, hs, vs, 3, cs_of(zj, kind), qts, out_layout=1 if kind == "chw" else 0, out_pitch=pitch)
    assert fc.crosses(pitch, h, npl) and zj.lib().zj_out_len(C.byref(d)) == npl * h * pitch
    need(torch, npl * h * pitch)
    dev = upload(torch, planes)
    if fe.refused_by_the_reference(kind, w, h, hs, vs, qts, planes):
        far = DevFar(torch, npl, h, rb, pitch)
        with pytest.raises(zj.ZjError) as e:
            ctx.decode_planes_device(d, 1, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), far.ptr)
        assert e.value.status == -5
        return
    want = fe.oracle_rows(kind, w, h, hs, vs, qts, planes)
    zero_rows = fe.uncovered(kind, h, hs, vs)
    try:
        for variant in zj.variants_available() if which == 0 else [0]:
            ctx.set_variant(variant)
            far = DevFar(torch, npl, h, rb, pitch)
            torch.cuda.synchronize()
            ctx.decode_planes_device(d, 1, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), far.ptr)
            ctx.sync()
            check_decode(far, want, pitch, zero_rows, True, f"frame {mode} {kind} {w}x{h} pitch {pitch} variant {variant}")
            del far
    finally:
        ctx.set_variant(0)


@OUT_PITCH
@pytest.mark.parametrize("w", fc.OUT_WIDTHS)
@pytest.mark.parametrize("kind", fe.KINDS)
@pytest.mark.parametrize("mode", list(fe.MODES))
def test_crop_decode(zj, ctx, torch, synth, mode, kind, w, which):
    hs, vs = fe.MODES[mode]
    npl, h, rb = fe.out_shape(kind, w)
    pitch = fc.out_pitches(w)[which]
    x, y = 3, 5
    W, H = 64, y + h
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
    full = fe.oracle_rows(kind, W, H, hs, vs, qts, planes).reshape(npl, H, -1)
    bpp = rb // w
    want = full[:, y:y + h, x * bpp:(x + w) * bpp]
    d = zj.FrameDesc.make(W, H, hs, vs, 3, cs_of(zj, kind), qts, out_layout=1 if kind == "chw" else 0)
    assert fc.crosses(pitch, h, npl) and zj.crop_out_len(d, w, h, pitch) == npl * h * pitch
    need(torch, npl * h * pitch)
    below = [r % H for r in fe.uncovered(kind, H, hs, vs)][:len(fe.uncovered(kind, H, hs, vs)) // npl]
    zero_rows = [r - y + p * h for p in range(npl) for r in below]
    dev = upload(torch, planes)
    far = DevFar(torch, npl, h, rb, pitch)
    torch.cuda.synchronize()
    ctx.decode_crops_device(d, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], [(x, y)], w, h, [far.ptr], out_pitch=pitch)
    ctx.sync()
    check_decode(far, want, pitch, zero_rows, False, f"crop {mode} {kind} {w}x{h} at ({x},{y}) pitch {pitch}")


@functools.lru_cache(maxsize=None)
def reduced_case(mode, kind, sl):
    """(W, H, planes, qts, the model's reduced frame) -- once for both pitches"""
    import scaled_model as sm
    synth = importlib.import_module("zune-jpeg_amd.synth")
    hs, vs = fe.MODES[mode]
    rh = {("rgb", 1): 4128, ("rgb", 3): 4104, ("gray", 1): 4128, ("gray", 3): 4104, ("chw", 1): 2056, ("chw", 3): 2052}[(kind, sl)]
    W, H = 96, rh << sl
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
    exp = sm.decode_scaled(W, H, hs, vs, 3, sm.GRAYSCALE if kind == "gray" else sm.RGB, qts, planes, sl, chw=kind == "chw", clamp_dc=False)
    assert sm.scaled_size(W, H, sl) == (W >> sl, rh)
    return W, H, planes, qts, np.asarray(exp)


@OUT_PITCH
@pytest.mark.parametrize("sl", [1, 3])
@pytest.mark.parametrize("kind", fe.KINDS)
@pytest.mark.parametrize("mode", list(fe.MODES))
def test_reduced_decode(zj, ctx, torch, mode, kind, sl, which):
    """frames 96 x 8256 at 1/2 and 96 x 32832 at 1/8 (CHW: 96 x 4112 and 96 x 16416)"""
    hs, vs = fe.MODES[mode]
    W, H, planes, qts, exp = reduced_case(mode, kind, sl)
    rw, rh = W >> sl, H >> sl
    npl, rb = (3, rw) if kind == "chw" else (1, rw * (1 if kind == "gray" else 3))
    pitch = fc.out_pitches(rw)[which]
    d = zj.FrameDesc.make(W, H, hs, vs, 3, cs_of(zj, kind), qts, out_layout=1 if kind == "chw" else 0)
    assert fc.crosses(pitch, rh, npl) and zj.scaled_crop_out_len(d, 1 << sl, rw, rh, pitch) == npl * rh * pitch
    need(torch, npl * rh * pitch)
    dev = upload(torch, planes)
    far = DevFar(torch, npl, rh, rb, pitch)
    torch.cuda.synchronize()
    ctx.decode_crops_scaled_device(d, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], 1 << sl, [far.ptr], out_pitch=pitch)
    ctx.sync()
    check_decode(far, exp.reshape(npl * rh, rb), pitch, [], False, f"reduced 1/{1 << sl} {mode} {kind} {rw}x{rh} pitch {pitch}")


# ---- c. frame x stride -----------------------------------------------------------------------------------------------------

def all_poison(torch, t):
    ok = torch.ones((), dtype=torch.bool, device=t.device)
    for lo in range(0, t.numel(), 1 << 29):
        ok &= (t[lo:lo + (1 << 29)] == POISON).all()
    return bool(ok)


@pytest.mark.parametrize("nframes,out_stride", [(3, fc.LINE31 + 4096), (2, fc.LINE32 + 4096)], ids=["3_past_2^31", "2_past_2^32"])
def test_strided_batch(zj, ctx, torch, synth, nframes, out_stride):
    """64 x 64 frames whose planes lie 2^30 elements (2 GB) apart and whose pixels lie out_stride bytes apart"""
    w = h = 64
    stride = 1 << 30                                         # int16 elements
    frames = [synth.make_frame(w, h, 2, 2, 3, seed=31, frame_index=i) for i in range(nframes)]
    qts = frames[0][1]
    d = zj.FrameDesc.make(w, h, 2, 2, 3, zj.ColorSpace.RGB, qts)
    out_len = zj.lib().zj_out_len(C.byref(d))
    ylen, clen = frames[0][0][0].size, frames[0][0][1].size
    assert 2 * stride * (nframes - 1) >= (fc.LINE32 if nframes == 3 else fc.LINE31) and out_stride * (nframes - 1) >= fc.LINE32
    total = 2 * ((nframes - 1) * stride * 3 + ylen + 2 * clen) + (nframes - 1) * out_stride + out_len
    need(torch, total)
    dev = [torch.empty(((nframes - 1) * stride + n,), dtype=torch.int16, device="cuda") for n in (ylen, clen, clen)]
    for i, (planes, _) in enumerate(frames):
        for c in range(3):
            dev[c][i * stride:i * stride + planes[c].size].copy_(torch.from_numpy(np.ascontiguousarray(planes[c], np.int16)))
    out = torch.full(((nframes - 1) * out_stride + out_len,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_planes_device_strided(d, nframes, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), out.data_ptr(), stride, stride,
                                     out_stride)
    ctx.sync()
    f = oc.make_frame(w, h, 2, 2, 3, oc.RGB, qts)
    for i, (planes, _) in enumerate(frames):
        rc, exp = oc.decode_planes(f, planes)
        assert rc == 0
        assert np.array_equal(out[i * out_stride:i * out_stride + out_len].cpu().numpy(), exp), f"frame {i} at byte {i * out_stride:#x}"
        if i + 1 < nframes:
            assert all_poison(torch, out[i * out_stride + out_len:(i + 1) * out_stride]), f"the space behind frame {i} was written"


# ---- d. slot x image bytes -------------------------------------------------------------------------------------------------

def slots_to_check(n, img_bytes):
    """the first and the last slot and those on both sides of each line"""
    s31, s32 = fc.LINE31 // img_bytes, fc.LINE32 // img_bytes
    assert 0 < s31 < s32 < n and (n - 1) * img_bytes >= fc.LINE32, "the last slot does not start past 2^32"
    return sorted({0, s31, s31 + 1, s32, s32 + 1, n - 1} & set(range(n)))


def check_slots(torch, out, img_bytes, n, nsrc, single):
    """slot i of the launch equals the same source through a call of its own (single(i) -> tensor) for the slots beside the
    lines, and the slot that shares its source for every other one"""
    checked = slots_to_check(n, img_bytes)
    slot = lambda i: out[i * img_bytes:(i + 1) * img_bytes]
    for i in checked:
        assert torch.equal(slot(i), single(i)), f"slot {i} (byte {i * img_bytes:#x}) differs from a call of its own"
    anchor = {}
    for i in checked:
        anchor.setdefault(i % nsrc, i)
    for k in range(nsrc):
        if k not in anchor:
            assert torch.equal(slot(k), single(k)), f"slot {k}"
            anchor[k] = k
    for i in range(n):
        if i not in checked:
            assert torch.equal(slot(i), slot(anchor[i % nsrc])), f"slot {i} differs from slot {anchor[i % nsrc]} of the same source"


@pytest.mark.parametrize("kind", ["bilinear", "antialiased", "bicubic"])
def test_resize_slots(zj, ctx, torch, kind):
    import emu_to_tensor_c as et
    n, side = 128, 1680
    img_bytes = side * side * 3 * 4
    assert n == 128 == et.batch()          # (zj_resize.h: RESIZE_BATCH, as zj_to_tensor.h: TT_BATCH -- one launch)
    assert img_bytes == 33_868_800 and 63 * img_bytes < fc.LINE31 <= 64 * img_bytes and 127 * img_bytes > fc.LINE32
    need(torch, n * img_bytes + 2 * img_bytes)
    rng = np.random.default_rng(7)
    sizes = [(9, 7), (16, 16), (5, 12), (23, 4), (13, 13)]
    srcs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]
    scale, bias = _norm(3)
    kw = dict(scale=scale, bias=bias, antialias=kind != "bilinear", interpolation="bicubic" if kind == "bicubic" else "bilinear")
    out = torch.full((n * img_bytes,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.resize_device([srcs[i % 5].data_ptr() for i in range(n)], [sizes[i % 5] for i in range(n)], 3, zj.LAYOUT_HWC, side, side,
                      zj.DTYPE_F32, zj.TENSOR_NHWC, out.data_ptr(), **kw)
    ctx.sync()

    def single(i):
        one = torch.full((img_bytes,), POISON, dtype=torch.uint8, device="cuda")
        ctx.resize_device([srcs[i % 5].data_ptr()], [sizes[i % 5]], 3, zj.LAYOUT_HWC, side, side, zj.DTYPE_F32, zj.TENSOR_NHWC,
                          one.data_ptr(), **kw)
        ctx.sync()
        return one
    check_slots(torch, out, img_bytes, n, 5, single)


def test_to_tensor_slots(zj, ctx, torch):
    import emu_to_tensor_c as et
    n, side = 128, 1680
    img_bytes = side * side * 3 * 4
    assert n <= et.batch() and 63 * img_bytes < fc.LINE31 <= 64 * img_bytes
    need(torch, n * img_bytes + 2 * img_bytes)
    gen = torch.Generator(device="cuda").manual_seed(11)
    srcs = [torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3)]
    scale, bias = _norm(3)
    out = torch.full((n * img_bytes,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.to_tensor_device([srcs[i % 3].data_ptr() for i in range(n)], side, side, 3, 3, zj.DTYPE_F32, zj.TENSOR_NHWC, out.data_ptr(),
                         scale=scale, bias=bias)
    ctx.sync()

    def single(i):
        one = torch.full((img_bytes,), POISON, dtype=torch.uint8, device="cuda")
        ctx.to_tensor_device([srcs[i % 3].data_ptr()], side, side, 3, 3, zj.DTYPE_F32, zj.TENSOR_NHWC, one.data_ptr(), scale=scale, bias=bias)
        ctx.sync()
        return one
    check_slots(torch, out, img_bytes, n, 3, single)


def test_warp_slots(zj, ctx, torch):
    import emu_warp_c as ew
    n, side = 48, 2760
    img_bytes = side * side * 3 * 4
    assert n <= ew.batch() == 48 and img_bytes == 91_411_200 and 23 * img_bytes < fc.LINE31 <= 24 * img_bytes
    need(torch, n * img_bytes + 2 * img_bytes)
    rng = np.random.default_rng(13)
    sizes = [(9, 7), (16, 16), (5, 12), (23, 4), (13, 13)]
    srcs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for w, h in sizes]
    # each source stretched over the output, turned a little: taps everywhere, some outside
    ms = []
    for w, h in sizes:
        sx, sy = w / side, h / side
        ms.append((sx, 0.1 * sy, -0.5, -0.1 * sx, sy, 0.25))
    scale, bias = _norm(3)
    kw = dict(scale=scale, bias=bias, fill=(7, 130, 255), edge="fill")
    out = torch.full((n * img_bytes,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.warp_device([srcs[i % 5].data_ptr() for i in range(n)], [sizes[i % 5] for i in range(n)], 3, [ms[i % 5] for i in range(n)],
                    side, side, zj.DTYPE_F32, zj.TENSOR_NHWC, out.data_ptr(), **kw)
    ctx.sync()

    def single(i):
        one = torch.full((img_bytes,), POISON, dtype=torch.uint8, device="cuda")
        ctx.warp_device([srcs[i % 5].data_ptr()], [sizes[i % 5]], 3, [ms[i % 5]], side, side, zj.DTYPE_F32, zj.TENSOR_NHWC, one.data_ptr(), **kw)
        ctx.sync()
        return one
    check_slots(torch, out, img_bytes, n, 5, single)


# ---- e. one image past 2^32 ------------------------------------------------------------------------------------------------

BIG_W, BIG_H = 16384, 21900


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("cin", [1, 3])
def test_to_tensor_one_image(zj, ctx, torch, cin, layout):
    """scale 2^-8 and bias 0: the value is the byte / 256, exact in float32"""
    w, h = BIG_W, BIG_H
    row = w * 3 * 4
    assert row == 196_608 and (h - 1) * row >= fc.LINE32 and 2 * w * h * 4 >= fc.LINE31
    need(torch, h * row + w * h * cin + (1 << 30))
    gen = torch.Generator(device="cuda").manual_seed(5 + cin)
    src = torch.randint(0, 256, (h, w, cin), dtype=torch.uint8, device="cuda", generator=gen)
    out = torch.full((h * w * 3,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.to_tensor_device([src.data_ptr()], w, h, cin, 3, zj.DTYPE_F32, zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW,
                         out.data_ptr(), scale=np.float32([2.0 ** -8] * 3), bias=np.float32([0, 0, 0]))
    ctx.sync()
    step = 1024
    ok = torch.ones((), dtype=torch.bool, device="cuda")
    for r0 in range(0, h, step):
        want = src[r0:r0 + step].float() * 2.0 ** -8                      # [rows, w, cin]
        if cin == 1:
            want = want.expand(-1, -1, 3)
        if layout == "NHWC":
            got = out.view(h, w, 3)[r0:r0 + step]
        else:
            got = out.view(3, h, w)[:, r0:r0 + step].permute(1, 2, 0)
        ok &= (got == want).all()
    assert bool(ok)
    for r in (0, fc.LINE31 // row, fc.LINE31 // row + 1, fc.LINE32 // row, fc.LINE32 // row + 1, h - 1):   # named, for the message
        got = out.view(h, w, 3)[r] if layout == "NHWC" else out.view(3, h, w)[:, r].permute(1, 0)
        want = src[r].float() * 2.0 ** -8
        assert torch.equal(got, want.expand(-1, 3) if cin == 1 else want), f"row {r}"


def test_crop_tensor_one_image(zj, ctx, torch, synth):
    """a 16384 x 21900 window of a 4:2:0 frame into f32 NHWC: rows 10922 and 21845 begin the first rows past 2^31 and 2^32;
    every probed band of rows equals a short window of its own over the same frame rows, and the twelve rows below the last
    complete strip are the converted zero"""
    w, h = BIG_W, BIG_H
    row = w * 3 * 4
    assert (fc.LINE31 // row, fc.LINE32 // row) == (10922, 21845)
    covered = h // 32 * 32
    assert h - covered == 12 and covered * row >= fc.LINE32
    need(torch, h * row + 3 * (1 << 30))
    dev = torch.device("cuda", 0)
    planes, qts = synth.make_frame_t(w, h, 2, 2, 3, seed=99, frame_index=0, device=dev)
    d = zj.FrameDesc.make(w, h, 2, 2, 3, zj.ColorSpace.RGB, qts)
    scale, bias = np.float32([1 / 255] * 3), np.float32([-0.5, 0.25, 1.0])
    out = torch.full((h * w * 3,), float("nan"), dtype=torch.float32, device="cuda")
    ptrs = [[p.data_ptr()] for p in planes]
    torch.cuda.synchronize()
    ctx.decode_crops_tensor_device(d, ptrs[0], ptrs[1], ptrs[2], [(0, 0)], w, h, zj.DTYPE_F32, zj.TENSOR_NHWC, out.data_ptr(),
                                   scale=scale, bias=bias)
    ctx.sync()
    rows = out.view(h, w, 3)
    assert not bool(torch.isnan(out[:1 << 20]).any())
    band = 8
    for r0 in (0, fc.LINE31 // row - 4, fc.LINE32 // row - 4, covered - band, h - band):
        one = torch.full((band * w * 3,), float("nan"), dtype=torch.float32, device="cuda")
        ctx.decode_crops_tensor_device(d, ptrs[0], ptrs[1], ptrs[2], [(0, r0)], w, band, zj.DTYPE_F32, zj.TENSOR_NHWC, one.data_ptr(),
                                       scale=scale, bias=bias)
        ctx.sync()
        assert torch.equal(rows[r0:r0 + band], one.view(band, w, 3)), f"rows {r0}..{r0 + band - 1} (byte {r0 * row:#x})"
    zero = torch.from_numpy(bias).cuda()                                   # 0 x scale + bias
    assert torch.equal(rows[covered:], zero.expand(h - covered, w, 3)), "the rows below the last complete strip"
    assert not bool(torch.isnan(rows[covered - 32:covered]).any()) and bool((rows[covered - 32:covered] != zero).any())
