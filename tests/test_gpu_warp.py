"""GPU: affine-warped images into a normalised tensor (zj_warp_device, zj_decode_crops_warped_device, tensors.warp_to_tensor
and decode_warped_to_tensor) on an MI355X.  The stage must equal the numpy model (tests/warp_model.py) bit
for bit and, where the definition reduces to them, the library's own older stages byte for byte: zj_to_tensor_device at the
identity, zj_orient_device + zj_to_tensor_device at the eight orientation matrices, zj_resize_device at x 2 and x 1/2 with
edge replication.  The plane call must equal the stage applied to the u8 image zj_decode_crops_device writes for the whole
frame.  Every output lies between guard bytes that must stay untouched."""
import ctypes as C
import importlib
import math
import zlib

import numpy as np
import pytest

import orient_model as om
import resize_model as rm
import warp_model as wm
from test_gpu_crop_tensor import ESZ, GUARD, KINDS, MODES, body, factors, frame_on_device, guarded, layout_code, ptrs, run_u8_crops
from test_gpu_to_tensor import images_on_device

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
COMBOS = [(dt, lay) for dt in (rm.F32, rm.F16, rm.BF16, rm.U8) for lay in ("NCHW", "NHWC")]
FILLS = [(0, 0, 0), (7, 130, 255)]
EDGES = {wm.FILL: "fill", wm.REPLICATE: "replicate"}
ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def tz():
    return importlib.import_module("zune-jpeg_amd.tensors")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)
    yield c
    c.close()


def matrices(w, h, ow, oh):
    """the emulation test's matrices: the eight orientations, 17 degrees, a shear, x 3.7, wholly outside, half outside"""
    ms = [wm.orientation_matrix(o, w, h) for o in range(1, 9)]
    cx, cy, ox, oy = w / 2, h / 2, ow / 2, oh / 2
    co, si = math.cos(math.radians(17)), math.sin(math.radians(17))
    sx, sy = min(w / ow, 100.0), min(h / oh, 100.0)
    ms.append((co * sx, -si * sy, cx - co * sx * ox + si * sy * oy, si * sx, co * sy, cy - si * sx * ox - co * sy * oy))
    ms.append((sx, 0.3 * sx, -0.3 * sx * oy, 0.0, sy, 0.0))
    ms.append((3.7, 0.0, 0.0, 0.0, 3.7, 0.0))
    ms.append((1.0, 0.0, float(w + 5), 0.0, 1.0, 0.0))
    ms.append((1.0, 0.0, -ow / 2 - 0.25, 0.0, 1.0, -oh / 2 + 0.375))
    return ms


def run_stage(zj, ctx, torch, ptrs_, sizes, pitches, ch, ms, ow, oh, dtype, layout, scale, bias, fill, edge):
    per = ch * ow * oh * ESZ[dtype]
    buf = guarded(torch, len(ptrs_) * per)
    ctx.warp_device(ptrs_, sizes, ch, ms, ow, oh, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, scale, bias, fill, EDGES[edge],
                    pitches)
    ctx.sync()
    return body(torch, buf, len(ptrs_) * per)


def model(imgs, ms, ow, oh, dtype, layout, scale, bias, fill, edge):
    return np.concatenate([np.ascontiguousarray(wm.warp(im, wm.fixed(m), ow, oh, dtype, scale, bias, edge, fill, layout)).view(np.uint8)
                           .reshape(-1) for im, m in zip(imgs, ms)])


def differ(got, exp, what):
    g = got.cpu().numpy() if hasattr(got, "cpu") else got
    e = exp.cpu().numpy() if hasattr(exp, "cpu") else exp
    if not np.array_equal(g, e):
        bad = np.nonzero(g != e)[0]
        raise AssertionError(f"{what}: {bad.size} of {g.size} bytes differ, first at {bad[:6].tolist()}")


# ---- 1. the stage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("edge", [wm.FILL, wm.REPLICATE], ids=["fill", "replicate"])
def test_stage_equals_the_model(zj, ctx, torch, ch, edge):
    """sources and outputs of the emulation test (a subset), three images a call, every matrix"""
    rng = np.random.default_rng(zlib.crc32(f"warp-{ch}-{edge}".encode()))
    k = 0
    for (w, h) in [(1, 1), (2, 1), (7, 5), (53, 37), (258, 3)]:
        for (ow, oh) in [(1, 1), (9, 3), (17, 2), (65, 33)]:
            all_ms = matrices(w, h, ow, oh)
            for m0 in range(0, len(all_ms), 3):
                ms = [all_ms[(m0 + i) % len(all_ms)] for i in range(3)]
                dtype, layout = COMBOS[k % 8]
                pads, mis = [[0, 1, 13], [13, 0, 1]][k % 2], [(k + i) % 4 for i in range(3)]
                dev, ptrs_, pitches, imgs = images_on_device(torch, rng, 3, w, h, ch, pads, mis)
                scale, bias = factors(rng, ch)
                fill = FILLS[(k // 3) % 2]
                got = run_stage(zj, ctx, torch, ptrs_, [(w, h)] * 3, pitches, ch, ms, ow, oh, dtype, layout, scale, bias, fill, edge)
                differ(got, model(imgs, ms, ow, oh, dtype, layout, scale, bias, fill, edge),
                       f"{w}x{h} C {ch} -> {ow}x{oh} dtype {dtype} {layout} pads {pads} misalign {mis} matrices {m0}..")
                k += 1


def test_images_of_their_own_sizes_and_more_than_one_launch(zj, ctx, torch):
    rng = np.random.default_rng(50)
    n = 50
    sizes = [(int(rng.integers(1, 40)), int(rng.integers(1, 30))) for _ in range(n)]
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (w, h) in sizes]
    devs = [torch.from_numpy(im).cuda() for im in host]
    torch.cuda.synchronize()
    ms = [matrices(w, h, 21, 13)[i % 13] for i, (w, h) in enumerate(sizes)]
    scale, bias = factors(rng, 3)
    for (dtype, layout, edge) in [(rm.BF16, "NCHW", wm.FILL), (rm.F32, "NHWC", wm.REPLICATE)]:
        got = run_stage(zj, ctx, torch, [t.data_ptr() for t in devs], sizes, None, 3, ms, 21, 13, dtype, layout, scale, bias, FILLS[1], edge)
        differ(got, model(host, ms, 21, 13, dtype, layout, scale, bias, FILLS[1], edge), f"50 images dtype {dtype} {layout}")


@pytest.mark.parametrize("ch", [1, 3])
def test_the_identity_is_the_to_tensor_stage(zj, ctx, torch, ch):
    rng = np.random.default_rng(60 + ch)
    for (w, h) in [(7, 3), (33, 17), (257, 5)]:
        for i, (dtype, layout) in enumerate(COMBOS):
            dev, ptrs_, pitches, imgs = images_on_device(torch, rng, 3, w, h, ch, [0, 1, 13], [(i + k) % 4 for k in range(3)])
            scale, bias = factors(rng, ch)
            got = run_stage(zj, ctx, torch, ptrs_, [(w, h)] * 3, pitches, ch, [(1, 0, 0, 0, 1, 0)] * 3, w, h, dtype, layout, scale, bias,
                            FILLS[1], i & 1)
            per = ch * w * h * ESZ[dtype]
            buf = guarded(torch, 3 * per)
            ctx.to_tensor_device(ptrs_, w, h, ch, ch, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, scale, bias, None, pitches)
            ctx.sync()
            differ(got, body(torch, buf, 3 * per), f"identity {w}x{h} C {ch} dtype {dtype} {layout}")


@pytest.mark.parametrize("ch", [1, 3])
def test_the_orientation_matrices_are_the_orient_stage(zj, ctx, torch, ch):
    rng = np.random.default_rng(70 + ch)
    w, h = 37, 22
    dev, ptrs_, pitches, imgs = images_on_device(torch, rng, 8, w, h, ch, [0, 5], [0, 1, 2, 3])
    for j, (dtype, layout) in enumerate([(rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NHWC"), (rm.F16, "NCHW")]):
        scale, bias = factors(rng, ch)
        for transposed in (False, True):
            os_ = [o for o in range(1, 9) if (o >= 5) == transposed]
            dw, dh = om.oriented_size(os_[0], w, h)
            idx = [o - 1 for o in os_]
            got = run_stage(zj, ctx, torch, [ptrs_[i] for i in idx], [(w, h)] * 4, [pitches[i] for i in idx], ch,
                            [wm.orientation_matrix(o, w, h) for o in os_], dw, dh, dtype, layout, scale, bias, FILLS[1], j & 1)
            turned = torch.empty(4 * dw * dh * ch, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            outs = [turned.data_ptr() + i * dw * dh * ch for i in range(4)]
            ctx.orient_device([ptrs_[i] for i in idx], [(w, h)] * 4, ch, zj.LAYOUT_HWC, os_, outs, [pitches[i] for i in idx])
            per = ch * dw * dh * ESZ[dtype]
            buf = guarded(torch, 4 * per)
            ctx.to_tensor_device(outs, dw, dh, ch, ch, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, scale, bias)
            ctx.sync()
            differ(got, body(torch, buf, 4 * per), f"orientations {os_} C {ch} dtype {dtype} {layout}")


@pytest.mark.parametrize("ch", [1, 3])
def test_a_scale_by_two_and_by_half_is_the_bilinear_resize(zj, ctx, torch, ch):
    rng = np.random.default_rng(80 + ch)
    w, h = 46, 30
    dev, ptrs_, pitches, imgs = images_on_device(torch, rng, 3, w, h, ch, [0, 1, 13], [1, 2, 3])
    for j, (dtype, layout) in enumerate(COMBOS):
        scale, bias = factors(rng, ch)
        for (ow, oh) in [(2 * w, 2 * h), (w // 2, h // 2), (2 * w, h // 2)]:
            m = (w / ow, 0, 0, 0, h / oh, 0)
            got = run_stage(zj, ctx, torch, ptrs_, [(w, h)] * 3, pitches, ch, [m] * 3, ow, oh, dtype, layout, scale, bias, None, wm.REPLICATE)
            per = ch * ow * oh * ESZ[dtype]
            buf = guarded(torch, 3 * per)
            ctx.resize_device(ptrs_, [(w, h)] * 3, ch, zj.LAYOUT_HWC, ow, oh, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, scale,
                              bias, None, pitches)
            ctx.sync()
            differ(got, body(torch, buf, 3 * per), f"{w}x{h} -> {ow}x{oh} C {ch} dtype {dtype} {layout}")


def test_stage_rejects_bad_arguments(zj, ctx, torch):
    L = zj.lib()
    rng = np.random.default_rng(5)
    dev, ptrs_, pitches, imgs = images_on_device(torch, rng, 1, 8, 8, 3, [0], [0])
    buf = guarded(torch, 3 * 8 * 8 * 4)
    out = C.c_void_p(buf.data_ptr() + GUARD)
    ins = (C.c_void_p * 1)(ptrs_[0])
    wh = (C.c_uint * 2)(8, 8)
    ok = (C.c_float * 3)(1.0, 1.0, 1.0)
    inf = (C.c_float * 3)(1.0, float("inf"), 1.0)
    M = lambda *v: (C.c_double * 6)(*v)
    ident = M(1, 0, 0, 0, 1, 0)
    hnd = ctx.handle
    call = lambda n, i, sizes, pit, ch, m, ow, oh, dt, lay, sc, bi, edge, dst: L.zj_warp_device(hnd, n, i, sizes, pit, ch, m, ow, oh, dt, lay,
                                                                                                sc, bi, None, edge, dst, None)
    assert call(1, ins, wh, None, 3, ident, 8, 8, 4, 0, ok, ok, 0, out) == ARG          # no such dtype
    assert call(1, ins, wh, None, 3, ident, 8, 8, 0, 2, ok, ok, 0, out) == ARG          # no such layout
    assert call(1, ins, wh, None, 3, ident, 8, 8, 0, 0, inf, ok, 0, out) == ARG
    assert call(1, ins, wh, None, 3, ident, 8, 8, 0, 0, ok, ok, 2, out) == ARG and call(1, ins, wh, None, 3, ident, 8, 8, 0, 0, ok, ok, -1, out) == ARG
    assert call(1, ins, wh, None, 3, ident, 0, 8, 0, 0, ok, ok, 0, out) == ARG and call(1, ins, wh, None, 3, ident, 8, 8193, 0, 0, ok, ok, 0, out) == ARG
    assert call(1, ins, wh, (C.c_uint * 1)(23), 3, ident, 8, 8, 0, 0, ok, ok, 0, out) == ARG   # a pitch below a row
    assert call(1, ins, (C.c_uint * 2)(0, 8), None, 3, ident, 8, 8, 0, 0, ok, ok, 0, out) == ARG
    assert call(1, ins, (C.c_uint * 2)(8, 65536), None, 3, ident, 8, 8, 0, 0, ok, ok, 0, out) == ARG
    assert call(0, ins, wh, None, 3, ident, 8, 8, 0, 0, ok, ok, 0, out) == ARG and call(1, ins, wh, None, 2, ident, 8, 8, 0, 0, ok, ok, 0, out) == ARG
    assert call(1, None, wh, None, 3, ident, 8, 8, 0, 0, ok, ok, 0, out) == ARG and call(1, ins, wh, None, 3, None, 8, 8, 0, 0, ok, ok, 0, out) == ARG
    assert call(1, (C.c_void_p * 1)(None), wh, None, 3, ident, 8, 8, 0, 0, ok, ok, 0, out) == ARG
    assert call(1, ins, wh, None, 3, ident, 8, 8, 0, 0, ok, ok, 0, None) == ARG
    assert call(1, ins, wh, None, 3, ident, 8, 8, 0, 0, ok, ok, 0, C.c_void_p(buf.data_ptr() + GUARD + 2)) == ARG  # not aligned to a float
    for bad in (M(float("nan"), 0, 0, 0, 1, 0), M(1, 128, 0, 0, 1, 0), M(1, 0, 0, -128, 1, 0), M(1, 0, 2.0 ** 31, 0, 1, 0),
                M(1, 0, 0, 0, 1, float("-inf"))):
        assert call(1, ins, wh, None, 3, bad, 8, 8, 0, 0, ok, ok, 0, out) == ARG
    ctx.sync()
    assert bool((buf == 0xAA).all()), "a refused call wrote"
    assert call(1, ins, wh, None, 3, ident, 8, 8, 0, 0, ok, ok, 0, out) == 0
    ctx.sync()
    one = np.ones(3, np.float32)
    differ(body(torch, buf, 3 * 8 * 8 * 4), model(imgs, [(1, 0, 0, 0, 1, 0)], 8, 8, rm.F32, "NCHW", one, one, None, wm.FILL), "the accepted call")


# ---- 2. the plane call ------------------------------------------------------------------------------------------------
def frame_matrices(W, H, ow, oh):
    """inside the frame; a rotation about its centre that crosses every edge; across the left / top, right / bottom edge; missing
    the frame on each side"""
    co, si = math.cos(math.radians(30)), math.sin(math.radians(30))
    s = 1.3 * max(W / ow, H / oh)
    return [(0.5, 0.0, W / 4, 0.0, 0.5, H / 4),
            (co * s, -si * s, W / 2 - co * s * ow / 2 + si * s * oh / 2, si * s, co * s, H / 2 - si * s * ow / 2 - co * s * oh / 2),
            (1.0, 0.0, -ow / 3, 0.0, 1.0, -oh / 2 + 0.25), (1.0, 0.0, W - ow / 2 + 0.5, 0.0, 1.0, H - oh / 3),
            (1.0, 0.0, float(W + 2), 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, -float(oh + 3)),
            (1.0, 0.0, -float(ow + 1), 0.0, 1.0, float(H + 1)), (0.0, 1.0, 0.0, -1.0, 0.0, float(H))]


def run_planes(zj, ctx, torch, d, frames, ch, ms, ow, oh, dtype, layout, scale, bias, fill, edge):
    per = ch * ow * oh * ESZ[dtype]
    buf = guarded(torch, len(frames) * per)
    y, cb, cr = ptrs(frames)
    ctx.decode_crops_warped_device(d, y, cb, cr, ms, ow, oh, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, scale, bias, fill,
                                   EDGES[edge])
    ctx.sync()
    return body(torch, buf, len(frames) * per)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["rgb", "gray"])
def test_plane_call_equals_the_stage_over_the_full_decode(zj, ctx, torch, synth, mode, kind):
    hs, vs = MODES[mode]
    ch = 1 if kind == "gray" else 3
    rng = np.random.default_rng(zlib.crc32(f"warp-planes-{mode}-{kind}".encode()))
    k = 0
    for (W, H) in [(96, 80), (517, 40)]:
        for flags in (0, zj.FLAG_CORRECTED):
            d, dev = frame_on_device(zj, torch, synth, W, H, hs, vs, kind, flags, seed=W + flags)
            if zj.crop_out_len(d, 1, 1) == 0:  # (a reference panic: refused as the crop call refuses it)
                with pytest.raises(zj.ZjError):
                    ctx.decode_crops_warped_device(d, *ptrs([dev]), [(1, 0, 0, 0, 1, 0)], 8, 8, rm.F32, 0, dev[0].data_ptr())
                continue
            full = run_u8_crops(zj, ctx, torch, d, [dev], [(0, 0)], W, H)[0]
            full_dev = torch.from_numpy(np.ascontiguousarray(full)).cuda()
            torch.cuda.synchronize()
            for (ow, oh) in [(33, 21), (64, 48)]:
                ms = frame_matrices(W, H, ow, oh)
                for edge in (wm.FILL, wm.REPLICATE):
                    dtype, layout = COMBOS[k % 8]
                    scale, bias = factors(rng, ch)
                    fill = FILLS[k % 2]
                    got = run_planes(zj, ctx, torch, d, [dev] * len(ms), ch, ms, ow, oh, dtype, layout, scale, bias, fill, edge)
                    ref = run_stage(zj, ctx, torch, [full_dev.data_ptr()] * len(ms), [(W, H)] * len(ms), None, ch, ms, ow, oh, dtype, layout,
                                    scale, bias, fill, edge)
                    differ(got, ref, f"{mode} {kind} {W}x{H} flags {flags} -> {ow}x{oh} dtype {dtype} {layout} edge {edge}")
                    k += 1
    assert k or mode == "v"  # (something was compared)


def test_plane_call_shows_a_gray_frame_as_rgb(zj, ctx, torch, synth):
    W, H = 96, 80
    planes, qts = synth.make_frame(W, H, 1, 1, 1, seed=9)
    d = zj.FrameDesc.make(W, H, 1, 1, 1, zj.ColorSpace.RGB, qts)
    d.flags = zj.FLAG_GRAY_TO_RGB
    dg = zj.FrameDesc.make(W, H, 1, 1, 1, zj.ColorSpace.GRAYSCALE, qts)
    y = torch.from_numpy(np.ascontiguousarray(planes[0], np.int16)).cuda()
    torch.cuda.synchronize()
    full = run_u8_crops(zj, ctx, torch, dg, [(y, y, y)], [(0, 0)], W, H)[0]
    rgb = torch.from_numpy(np.ascontiguousarray(np.repeat(full, 3, axis=2))).cuda()
    torch.cuda.synchronize()
    ms = frame_matrices(W, H, 40, 24)
    rng = np.random.default_rng(11)
    scale, bias = factors(rng, 3)
    for edge in (wm.FILL, wm.REPLICATE):
        per = 3 * 40 * 24 * 2
        buf = guarded(torch, len(ms) * per)
        ctx.decode_crops_warped_device(d, [y.data_ptr()] * len(ms), None, None, ms, 40, 24, rm.BF16, zj.TENSOR_NCHW, buf.data_ptr() + GUARD,
                                       scale, bias, FILLS[1], EDGES[edge])
        ctx.sync()
        ref = run_stage(zj, ctx, torch, [rgb.data_ptr()] * len(ms), [(W, H)] * len(ms), None, 3, ms, 40, 24, rm.BF16, "NCHW", scale, bias,
                        FILLS[1], edge)
        differ(body(torch, buf, len(ms) * per), ref, f"gray as RGB, edge {edge}")


def test_plane_call_rejects_bad_arguments(zj, ctx, torch, synth):
    L = zj.lib()
    d, dev = frame_on_device(zj, torch, synth, 64, 32, 2, 2, "rgb", 0, seed=2)
    buf = guarded(torch, 3 * 8 * 8 * 4)
    out = C.c_void_p(buf.data_ptr() + GUARD)
    P = lambda t: (C.c_void_p * 1)(t.data_ptr())
    y, cb, cr = P(dev[0]), P(dev[1]), P(dev[2])
    ident = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    call = lambda dd, yy, m, ow, oh, dt, lay, edge, dst: L.zj_decode_crops_warped_device(ctx.handle, C.byref(dd), 1, yy, cb, cr, m, ow, oh, dt,
                                                                                         lay, None, None, None, edge, dst, None)
    assert call(d, y, ident, 8, 8, 4, 0, 0, out) == ARG and call(d, y, ident, 8, 8, 0, 2, 0, out) == ARG
    assert call(d, y, ident, 8, 8, 0, 0, 2, out) == ARG and call(d, y, ident, 0, 8, 0, 0, 0, out) == ARG
    assert call(d, None, ident, 8, 8, 0, 0, 0, out) == ARG and call(d, y, None, 8, 8, 0, 0, 0, out) == ARG
    assert call(d, y, ident, 8, 8, 0, 0, 0, None) == ARG
    assert call(d, y, (C.c_double * 6)(1, 0, 0, 0, 200, 0), 8, 8, 0, 0, 0, out) == ARG
    rgba, _ = frame_on_device(zj, torch, synth, 64, 32, 2, 2, "rgb", 0, seed=2)
    rgba.out_colorspace = int(zj.ColorSpace.RGBA)
    assert call(rgba, y, ident, 8, 8, 0, 0, 0, out) == UNSUPPORTED
    ctx.sync()
    assert bool((buf == 0xAA).all()), "a refused call wrote"
    assert call(d, y, ident, 8, 8, 0, 0, 0, out) == 0
    ctx.sync()


# ---- 3. the wrappers --------------------------------------------------------------------------------------------------
def grid_sample_ref(torch, img, m, ow, oh, edge):
    """float64 on the CPU: img [h, w, C] u8 -> [C, oh, ow]"""
    import torch.nn.functional as F
    h, w, _ = img.shape
    Y, X = np.meshgrid(np.arange(oh) + 0.5, np.arange(ow) + 0.5, indexing="ij")
    grid = np.stack([2 * (m[0] * X + m[1] * Y + m[2]) / w - 1, 2 * (m[3] * X + m[4] * Y + m[5]) / h - 1], -1)[None]
    src = torch.from_numpy(img.transpose(2, 0, 1)[None].astype(np.float64))
    return F.grid_sample(src, torch.from_numpy(grid).double(), mode="bilinear", padding_mode="border" if edge == "replicate" else "zeros",
                         align_corners=False)[0]


def test_tensors_wrappers(zj, tz, ctx, torch, synth):
    """warp_to_tensor and decode_warped_to_tensor against float64 grid_sample of the u8 image: 2.0 grey levels (the derived
    bound of tests/test_warp_model.py) times the normalisation's scale per element; bf16 adds its rounding, 2^-9 of the value"""
    rng = np.random.default_rng(21)
    W, H, ow, oh = 96, 80, 64, 48
    d, dev = frame_on_device(zj, torch, synth, W, H, 2, 2, "rgb", 0, seed=5)
    full = run_u8_crops(zj, ctx, torch, d, [dev], [(0, 0)], W, H)[0]
    img = torch.from_numpy(np.ascontiguousarray(full)).cuda()
    ms = [tz.warp_matrix((ow, oh), (W / 2, H / 2), angle=a, scale=s, shear=sh, translate=t, hflip=f)
          for a, s, sh, t, f in [(0, 1, (0, 0), (0, 0), False), (15, 0.8, (0, 0), (3, -2), False), (-45, 1.3, (10, 0), (0, 0), True),
                                 (90, (0.5, 0.7), (0, -8), (-20, 5), False)]]
    mean, std = torch.tensor(MEAN, dtype=torch.float64), torch.tensor(STD, dtype=torch.float64)
    for edge in ("fill", "replicate"):
        for dtype in (torch.float32, torch.bfloat16):
            a = tz.warp_to_tensor(ctx, [img] * len(ms), ms, (ow, oh), dtype=dtype, mean=MEAN, std=STD, edge=edge)
            b = tz.decode_warped_to_tensor(ctx, d, [dev] * len(ms), ms, (ow, oh), dtype=dtype, mean=MEAN, std=STD, edge=edge)
            torch.cuda.synchronize()
            assert a.dtype == dtype and tuple(a.shape) == (len(ms), 3, oh, ow) and torch.equal(a, b)
            for i, m in enumerate(ms):
                ref = (grid_sample_ref(torch, full, m, ow, oh, edge) / 255 - mean[:, None, None]) / std[:, None, None]
                # 2.0 grey levels times the scale.  float32 adds four roundings: of the product and of the sum (both below 8 in
                # magnitude, since 1 / std < 4.5 and |mean / std| < 2.2: half a unit is 2^-22 each), of the float32 scale (2^-24
                # of a product below 4.5: under 2^-22) and of the bias (under 2^-23): under 2^-20 in all.  bf16 on top: half a
                # unit in the last of 8 bits of the value
                t0 = 2.0 / (255 * std[:, None, None]) + 2.0 ** -20
                tol = t0 + (ref.abs() + t0) * 2.0 ** -9 if dtype == torch.bfloat16 else t0
                err = (a[i].double().cpu() - ref).abs()
                assert bool((err <= tol).all()), (edge, dtype, i, float((err - tol).max()))
    u8 = tz.warp_to_tensor(ctx, [img], [ms[0]], (ow, oh), dtype=torch.uint8, layout="NHWC", fill=(1, 2, 3))
    torch.cuda.synchronize()
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1, oh, ow, 3)
    with pytest.raises(ValueError):
        tz.warp_to_tensor(ctx, [img], ms[:2], (ow, oh))
    with pytest.raises(ValueError):
        tz.warp_to_tensor(ctx, [img], ms[:1], (ow, oh), edge="wrap")


# ---- 4. the file call -------------------------------------------------------------------------------------------------
def displayed_u8(zj, ctx, torch, blob, opt, dw, dh):
    """the u8 image [dh, dw, 3] a file decodes to, on the device: the resized-crop oriented file call at out == the whole
    displayed image, which is that image itself"""
    from test_gpu_to_tensor import resized_call
    return resized_call(zj, ctx, torch, blob, opt, (0, 0, dw, dh), rm.U8, "NHWC", None, None, False, oriented=True).clone()


def warped_call(zj, ctx, torch, blob, opt, m, ow, oh, dtype, layout, scale, bias, fill, edge, oriented=True):
    per = 3 * ow * oh * ESZ.get(dtype, 4)
    buf = guarded(torch, per)
    dec = zj.Decoder(opt, ctx)
    try:
        dec.prepare(blob)
        try:
            n = dec.finish_pixels_warped_device(m, ow, oh, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, per, scale, bias, fill,
                                                EDGES[edge] if edge in EDGES else edge, oriented)
            assert n == per, "*out_len is not the image's size"
            rc, text = 0, ""
        except zj.ZjError as e:
            rc, text = e.status, str(e)
    finally:
        dec.close()
    return rc, body(torch, buf, per), text


def file_cases(synth, je):
    """(name, blob, stored w, h, orientation): a colour, a gray, a CMYK, a 4:1:1 and a turned file"""
    import sampling_cases as sc
    from test_gpu_cmyk import four_file
    from test_gpu_sampling import odd_file
    from test_gpu_to_tensor import colour_file, gray_file
    return [("colour", colour_file(je, synth, 97, 61, 2, 2, 4), 97, 61, 1), ("gray", gray_file(je, synth), 120, 50, 1),
            ("cmyk", four_file(synth, 100, 75, "hv", 21, adobe=2), 100, 75, 1),
            ("411", odd_file(synth, 100, 75, sc.SAMPLINGS[0], 21), 100, 75, 1),
            ("turned", colour_file(je, synth, 64, 48, 2, 2, 5, orientation=6), 64, 48, 6)]


@pytest.fixture(scope="module")
def je():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import jpeg_enc
    return jpeg_enc


@pytest.mark.parametrize("entropy", ["ENTROPY_CPU", "ENTROPY_GPU_ALWAYS"])
def test_file_call_equals_the_stage_over_the_displayed_image(zj, ctx, torch, synth, je, entropy):
    from test_gpu_to_tensor import options
    opt = options(zj, entropy)
    rng = np.random.default_rng(zlib.crc32(entropy.encode()))
    k = 0
    for name, blob, W, H, o in file_cases(synth, je):
        dw, dh = om.oriented_size(o, W, H)
        ow, oh = 40, 28
        try:
            img = displayed_u8(zj, ctx, torch, blob, opt, dw, dh)
        except zj.ZjError as e:
            # (only a file the resized-crop file call itself does not finish in this entropy mode: the warped call must
            # refuse it with the same status and write nothing)
            assert entropy != "ENTROPY_CPU" and name in ("cmyk", "411"), (name, entropy, str(e))
            try:
                rc, got, text = warped_call(zj, ctx, torch, blob, opt, (1, 0, 0, 0, 1, 0), ow, oh, rm.F32, "NCHW", None, None, None, wm.FILL)
            except zj.ZjError as e2:  # (refused when it is prepared)
                rc, got = e2.status, None
            assert rc == e.status, (name, entropy, rc, e.status)
            assert got is None or bool((got == 0xAA).all())
            continue
        for m in frame_matrices(dw, dh, ow, oh):
            for edge in (wm.FILL, wm.REPLICATE):
                dtype, layout = [(rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NHWC"), (rm.F16, "NCHW")][k % 4]
                scale, bias = factors(rng, 3)
                rc, got, text = warped_call(zj, ctx, torch, blob, opt, m, ow, oh, dtype, layout, scale, bias, FILLS[k % 2], edge)
                assert rc == 0, (name, m, rc, text)
                ref = run_stage(zj, ctx, torch, [img.data_ptr()], [(dw, dh)], None, 3, [m], ow, oh, dtype, layout, scale, bias, FILLS[k % 2], edge)
                differ(got, ref, f"{name} {entropy} matrix {m} edge {edge} dtype {dtype} {layout}")
                k += 1
    assert k >= 3 * 16


def test_file_call_refusals_and_the_files_wrapper(zj, tz, ctx, torch, synth, je):
    from test_gpu_to_tensor import options
    opt = options(zj)
    cases = file_cases(synth, je)
    name, blob, W, H, o = cases[0]
    ident = (1, 0, 0, 0, 1, 0)
    for bad_m in ((float("nan"), 0, 0, 0, 1, 0), (1, 0, 0, 0, 128, 0)):
        rc, got, text = warped_call(zj, ctx, torch, blob, opt, bad_m, 16, 16, rm.F32, "NCHW", None, None, None, wm.FILL)
        assert rc == ARG and bool((got == 0xAA).all())
    rc, got, text = warped_call(zj, ctx, torch, blob, opt, ident, 16, 16, 4, "NCHW", None, None, None, wm.FILL)
    assert rc == ARG and bool((got == 0xAA).all())
    rc, got, text = warped_call(zj, ctx, torch, blob, opt, ident, 16, 8193, rm.U8, "NCHW", None, None, None, wm.FILL)
    assert rc == ARG
    ycc = options(zj)  # (the resized call's refusal: a gray file shown as RGB has no YCbCr form)
    ycc.out_colorspace = zj.ColorSpace.YCbCr
    rc, got, text = warped_call(zj, ctx, torch, cases[1][1], ycc, ident, 16, 16, rm.F32, "NCHW", None, None, None, wm.FILL)
    assert rc == UNSUPPORTED and "GRAY_TO_RGB" in text and bool((got == 0xAA).all())
    chw = options(zj)
    chw.out_layout = zj.LAYOUT_CHW
    rc, got, text = warped_call(zj, ctx, torch, blob, chw, ident, 16, 16, rm.F32, "NCHW", None, None, None, wm.FILL)
    assert rc == UNSUPPORTED and bool((got == 0xAA).all())
    # the wrapper: image k is the single-file call's
    ms = [tz.warp_matrix((32, 24), (om.oriented_size(o, W, H)[0] / 2, om.oriented_size(o, W, H)[1] / 2), angle=20 * i, scale=0.4)
          for i, (_, _, W, H, o) in enumerate(cases)]
    out = tz.decode_files_warped_to_tensor(ctx, [c[1] for c in cases], ms, (32, 24), dtype=torch.float32, layout="NHWC", mean=MEAN, std=STD,
                                           fill=(114, 114, 114), options=opt, workers=2, apply_orientation=True)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (len(cases), 24, 32, 3)
    s, b = tz.normalize_factors(3, MEAN, STD)
    for i, c in enumerate(cases):
        rc, one, _ = warped_call(zj, ctx, torch, c[1], opt, ms[i], 32, 24, rm.F32, "NHWC", s, b, (114, 114, 114), wm.FILL)
        assert rc == 0 and torch.equal(out[i].reshape(-1).view(torch.uint8), one), c[0]
    with pytest.raises(zj.DecodeError) as e:
        tz.decode_files_warped_to_tensor(ctx, [cases[0][1], cases[0][1][:300], cases[1][1]], ms[:3], (32, 24), options=opt)
    assert "file 1" in str(e.value)


# ---- 5. the batch call ------------------------------------------------------------------------------------------------
def test_batch_of_every_kind(zj, tz, ctx, torch, synth, je):
    """twelve files -- ordinary 4:2:0 / 4:4:4 / 4:2:2 / 4:4:0, gray, CMYK, 4:1:1, two turned, one damaged in the middle --, each
    under its own matrix, one of which misses its frame and one of which the warp refuses: image by image the single-file
    call's bytes, with its status; a failed file's image untouched"""
    from test_gpu_to_tensor import I_DAMAGED, batch_files, options
    blobs = batch_files(synth, je)
    n, ow, oh = len(blobs), 40, 28
    assert n == 12 and I_DAMAGED == 7
    opt = options(zj)
    rng = np.random.default_rng(12)
    decs, sizes = [], []
    for k, b in enumerate(blobs):
        dec = zj.Decoder(opt, ctx)
        try:
            info = dec.prepare(b)[1]
            sizes.append(om.oriented_size(dec.orientation, int(info.width), int(info.height)))
        except zj.ZjError:
            assert k == I_DAMAGED
            sizes.append((96, 72))
        decs.append(dec)
    ms = [frame_matrices(dw, dh, ow, oh)[k % 4] for k, (dw, dh) in enumerate(sizes)]
    I_MISSES, I_REFUSED = 3, 10
    ms[I_MISSES] = frame_matrices(*sizes[I_MISSES], ow, oh)[4]        # the output sees nothing of the frame: all fill
    ms[I_REFUSED] = (1.0, 0.0, 0.0, 0.0, 128.0, 0.0)                   # not a matrix the warp takes
    scale, bias = factors(rng, 3)
    try:
        for (dtype, layout, edge) in [(rm.BF16, "NCHW", wm.FILL), (rm.F32, "NHWC", wm.REPLICATE)]:
            per = 3 * ow * oh * ESZ[dtype]
            buf = guarded(torch, n * per)
            rcs = zj.finish_pixels_warped_batch(decs, ctx, ms, ow, oh, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD, n * per,
                                                scale, bias, FILLS[1], EDGES[edge], apply_orientation=True)
            got = body(torch, buf, n * per)
            for k in range(n):
                img = got[k * per:(k + 1) * per]
                if k == I_DAMAGED:
                    assert rcs[k] != 0 and bool((img == 0xAA).all())
                    continue
                rc, one, text = warped_call(zj, ctx, torch, blobs[k], opt, ms[k], ow, oh, dtype, layout, scale, bias, FILLS[1], edge)
                assert rcs[k] == rc, (k, rcs, text)
                assert torch.equal(img, one), (dtype, layout, k)  # (a failed file: the poison in both)
                assert (rc != 0) == (k == I_REFUSED), (k, rc, text)
            if edge == wm.FILL:  # the file whose output misses its frame: the converted fill, whatever the file holds
                miss = got[I_MISSES * per:(I_MISSES + 1) * per]
                assert torch.equal(miss[:2], miss[2:4]) and not bool((miss == 0xAA).all())
    finally:
        for d in decs:
            d.close()
    # the same through the tensors wrapper
    good = [k for k in range(n) if k not in (I_DAMAGED, I_REFUSED)]
    out = tz.decode_files_warped_to_tensor(ctx, [blobs[k] for k in good], [ms[k] for k in good], (ow, oh), dtype=torch.float32,
                                           layout="NHWC", mean=MEAN, std=STD, fill=FILLS[1], options=opt, workers=2, apply_orientation=True)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (len(good), oh, ow, 3)
    s, b = tz.normalize_factors(3, MEAN, STD)
    for i, k in enumerate(good):
        rc, one, _ = warped_call(zj, ctx, torch, blobs[k], opt, ms[k], ow, oh, rm.F32, "NHWC", s, b, FILLS[1], wm.FILL)
        assert rc == 0 and torch.equal(out[i].reshape(-1).view(torch.uint8), one), k
    with pytest.raises(zj.DecodeError) as e:
        tz.decode_files_warped_to_tensor(ctx, [blobs[0], blobs[2], blobs[I_REFUSED], blobs[4]], [ms[0], ms[2], ms[I_REFUSED], ms[4]],
                                         (ow, oh), options=opt, workers=2, apply_orientation=True)
    assert "file 2" in str(e.value)


def test_batch_call_rejects_bad_arguments(zj, ctx, torch, synth, je):
    L = zj.lib()
    from test_gpu_to_tensor import colour_file, options
    dec = zj.Decoder(options(zj), ctx)
    ycc = options(zj)
    ycc.out_colorspace = zj.ColorSpace.YCbCr
    other = zj.Decoder(ycc, ctx)
    try:
        dec.prepare(colour_file(je, synth, 97, 61, 2, 2, 4))
        other.prepare(colour_file(je, synth, 97, 61, 2, 2, 4))
        buf = guarded(torch, 2 * 3 * 8 * 8 * 4)
        out = C.c_void_p(buf.data_ptr() + GUARD)
        m = (C.c_double * 12)(1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0)
        rcs = (C.c_int * 2)(7, 7)
        ds = (C.c_void_p * 2)(dec._d, dec._d)
        call = lambda dd, nn, cc, mm, dst, cap, rr: L.zj_decoder_finish_pixels_warped_batch_device(dd, nn, cc, mm, 0, 8, 8, 0, 0, None, None, None,
                                                                                                   0, dst, cap, rr)
        assert call(None, 2, ctx.handle, m, out, 1536, rcs) == ARG and call(ds, 0, ctx.handle, m, out, 1536, rcs) == ARG
        assert call(ds, 2, None, m, out, 1536, rcs) == ARG and call(ds, 2, ctx.handle, None, out, 1536, rcs) == ARG
        assert call(ds, 2, ctx.handle, m, None, 1536, rcs) == ARG and call(ds, 2, ctx.handle, m, out, 1536, None) == ARG
        assert call(ds, 2, ctx.handle, m, out, 1535, rcs) == ARG                                  # room for one image only
        assert call((C.c_void_p * 2)(dec._d, other._d), 2, ctx.handle, m, out, 1536, rcs) == ARG  # two colour spaces
        assert call((C.c_void_p * 2)(None, None), 2, ctx.handle, m, out, 1536, rcs) == ARG
        assert list(rcs) == [7, 7] and bool((buf == 0xAA).all()), "a refused call wrote"
        assert call((C.c_void_p * 2)(dec._d, None), 2, ctx.handle, m, out, 1536, rcs) == 0 and list(rcs) == [0, ARG]
        assert bool((buf[GUARD + 768:] == 0xAA).all()) and not bool((buf[GUARD:GUARD + 768] == 0xAA).all())
    finally:
        dec.close()
        other.close()
