"""GPU: the output conversions of every tensor stage (zj_resize.h: resize_f32, resize_pack2<F16 / BF16>, resize_u8, as the
compiler lowers them for gfx950: packed multiplies and adds, v_cvt_pk_f16_f32, v_cvt_pk_bf16_f32) at the edges of float32,
half and bfloat16 on an MI355X -- subnormal products, sums and results, ties between two halves (subnormal ones too), 65504
and 65520, float32 just under FLT_MAX into bfloat16, overflow to inf, cancellation to +0, -0, and the bicubic filter's two
clamps.  The cases are tests/convert_cases.py's (test_convert_cases.py shows that every class is reached by every stage);
every output must equal the stage's numpy model bit for bit, compared as integers, between guard bytes that stay untouched.  A
mismatch names the edge class of the first differing element.

Entry points: zj_resize_device; zj_resize_filtered_device with the triangle and the bicubic filter; zj_to_tensor_device;
zj_decode_crops_tensor_device (its windows reach the rows the reference leaves at zero: the converted fill); zj_warp_device
with fill and with replicate; zj_decode_crops_resized_prescaled_device over a 1/2 reduced decode.  F32, F16, BF16 and U8, NCHW
and NHWC, one and three channels, every factor set.  One launch of four small images per case; the launches of a test share
one output buffer and one synchronisation."""
import importlib

import numpy as np
import pytest

import convert_cases as cc
import resize_model as rm
import warp_model as wm
from test_gpu_crop_tensor import convert as convert_crops
from test_gpu_crop_tensor import layout_code, run_u8_crops
from test_gpu_resize_bicubic import from_v

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered")]
GUARD = 256
ESZ = {cc.F32: 4, cc.F16: 2, cc.BF16: 2, cc.U8: 1}
DTYPES = [cc.F32, cc.F16, cc.BF16, cc.U8]
IDS = ["f32", "f16", "bf16", "u8"]
LAYOUTS = ["NCHW", "NHWC"]
N = 4  # images of a launch


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


def factor_cases(channels, dtype):
    """U8 takes no factors: one launch"""
    cases = list(cc.factor_cases(channels))
    return cases[:1] if dtype == cc.U8 else cases


class Slots:
    """one device buffer for the outputs of a test's launches, each between GUARD bytes of 0xAA"""

    def __init__(self, torch, lengths):
        self.offs, at = [], GUARD
        for n in lengths:
            self.offs.append(at)
            at += (n + 15) // 16 * 16 + GUARD
        self.lengths = lengths
        self.buf = torch.full((at,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the fill is torch's, the stores the library's stream)

    def ptr(self, k):
        return self.buf.data_ptr() + self.offs[k]

    def read(self):
        """the outputs on the host, after checking every byte between them"""
        a = self.buf.cpu().numpy()
        inside = np.zeros(a.size, bool)
        for o, n in zip(self.offs, self.lengths):
            inside[o:o + n] = True
        assert (a[~inside] == 0xAA).all(), "a byte outside an output tensor was written"
        return [a[o:o + n] for o, n in zip(self.offs, self.lengths)]


def upload(torch, imgs, pads=(0, 5, 1, 13)):
    """[C, h, w] images as interleaved rows, each at a pitch and a misalignment of its own: (buffer, pointers, pitches)"""
    blobs, offs, pitches, at = [], [], [], 0
    for i, img in enumerate(imgs):
        c, h, w = img.shape
        pitch = w * c + pads[i % len(pads)]
        rows = np.full((h, pitch), 0xEE, np.uint8)
        rows[:, :w * c] = img.transpose(1, 2, 0).reshape(h, w * c)
        at = (at + 3) // 4 * 4 + i % 4
        offs.append(at); pitches.append(pitch); blobs.append(rows.reshape(-1))
        at += rows.size
    host = np.zeros(at + 16, np.uint8)
    for o, b in zip(offs, blobs):
        host[o:o + b.size] = b
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return dev, [dev.data_ptr() + o for o in offs], pitches


def run_cases(torch, ctx, channels, dtype, layout, sizes, launch, expected, what):
    """launch(size, scale, bias, out pointer) for every size and factor case, one synchronisation, then every image against
    expected(size, i, scale, bias) -> (the model's output, v [C, oh, ow], flipped)"""
    cases = [(size, f) for size in sizes for f in factor_cases(channels, dtype)]
    per = {size: channels * size[0] * size[1] * ESZ[dtype] for size in sizes}
    slots = Slots(torch, [N * per[size] for size, _ in cases])
    for k, (size, (name, scale, bias)) in enumerate(cases):
        launch(size, scale, bias, slots.ptr(k))
    ctx.sync()
    for out, (size, (name, scale, bias)) in zip(slots.read(), cases):
        for i in range(N):
            exp, v, flip = expected(size, i, scale, bias)
            cc.check(out[i * per[size]:(i + 1) * per[size]], exp, dtype, v, scale, bias, flip, layout,
                     f"{what} C {channels} dtype {dtype} {layout} factors {name} image {i} -> {size[0]}x{size[1]}")


# ---- the three resizes over u8 images in device memory -----------------------------------------------------------------
FILTERS = {"resize": dict(), "resize_aa": dict(antialias=True), "resize_bicubic": dict(antialias=True, interpolation="bicubic")}


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("stage", list(FILTERS))
def test_resizes(zj, ctx, torch, stage, dtype, layout, channels):
    dev, ptrs, pitches = upload(torch, cc.images(*cc.SRC, channels))
    vals = cc.cached_values(stage, channels)

    def launch(size, scale, bias, out):
        ctx.resize_device(ptrs, [cc.SRC] * N, channels, zj.LAYOUT_HWC, size[0], size[1], dtype, layout_code(zj, layout), out, scale, bias,
                          cc.FLIPS, pitches, **FILTERS[stage])

    def expected(size, i, scale, bias):
        v = vals[size, i]
        return from_v(v, dtype, scale, bias, cc.FLIPS[i], layout), v, cc.FLIPS[i]

    run_cases(torch, ctx, channels, dtype, layout, cc.OUTS, launch, expected, stage)


# ---- u8 images into a tensor at their own size -----------------------------------------------------------------------------
@pytest.mark.parametrize("chans", [(1, 1), (1, 3), (3, 3)], ids=["1to1", "1to3", "3to3"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_to_tensor(zj, ctx, torch, dtype, layout, chans):
    cin, cout = chans
    src = {size: cc.images(*size, cin) for size in cc.OUTS}
    up = {size: upload(torch, src[size], pads=(0, 1, 13, 0)) for size in cc.OUTS}

    def launch(size, scale, bias, out):
        ctx.to_tensor_device(up[size][1], size[0], size[1], cin, cout, dtype, layout_code(zj, layout), out, scale, bias, cc.FLIPS,
                             up[size][2])

    def expected(size, i, scale, bias):
        img = src[size][i] if cin == cout else np.repeat(src[size][i], cout, axis=0)
        return rm.resize(img, size[0], size[1], dtype, scale, bias, cc.FLIPS[i], layout), img.astype(np.int64) << 16, cc.FLIPS[i]

    run_cases(torch, ctx, cout, dtype, layout, cc.OUTS, launch, expected, f"to_tensor {cin}->{cout}")


# ---- crop windows of coefficient planes into a tensor: the model is the conversion of zj_decode_crops_device's own crop -----
def planes_on_device(zj, torch, args, planes):
    w, h, hs, vs, ncomp, cs, qts = args
    d = zj.FrameDesc.make(w, h, hs, vs, ncomp, cs, qts)
    dev = [torch.from_numpy(np.ascontiguousarray(p, np.int16)).cuda() for p in planes]
    torch.cuda.synchronize()
    return d, dev


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_crop_tensor(zj, ctx, torch, dtype, layout, channels):
    args, planes, _ = cc.crop_frame(channels)
    d, dev = planes_on_device(zj, torch, args, planes)
    y, cb, cr = [[p.data_ptr()] * N for p in dev]
    crops = {size: run_u8_crops(zj, ctx, torch, d, [dev] * N, cc.CROP_ORIGINS[size], *size) for size in cc.OUTS}  # [N, h, w, C]
    for size in cc.OUTS:
        assert any(not c[-1].any() for c in crops[size]), "no window reaches the rows that stay zero: the converted fill is not run"

    def launch(size, scale, bias, out):
        ctx.decode_crops_tensor_device(d, y, cb, cr, cc.CROP_ORIGINS[size], size[0], size[1], dtype, layout_code(zj, layout), out, scale,
                                       bias, cc.FLIPS)

    def expected(size, i, scale, bias):
        c = crops[size][i:i + 1]
        return convert_crops(c, dtype, layout, scale, bias, cc.FLIPS[i:i + 1]), c[0].transpose(2, 0, 1).astype(np.int64) << 16, cc.FLIPS[i]

    run_cases(torch, ctx, channels, dtype, layout, cc.OUTS, launch, expected, "crop_tensor")


# ---- the affine warp: fill (the converted fill bytes) and replicate ----------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("edge", [wm.FILL, wm.REPLICATE], ids=["fill", "replicate"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_warp(zj, ctx, torch, dtype, layout, edge, channels):
    imgs = cc.images(*cc.SRC, channels)
    dev, ptrs, pitches = upload(torch, imgs, pads=(0, 1, 13, 0))
    vals = cc.cached_values("warp_fill" if edge == wm.FILL else "warp_replicate", channels)
    ms = {size: cc.warp_matrices(*cc.SRC, *size) for size in cc.OUTS}

    def launch(size, scale, bias, out):
        ctx.warp_device(ptrs, [cc.SRC] * N, channels, ms[size], size[0], size[1], dtype, layout_code(zj, layout), out, scale, bias,
                        cc.WARP_FILL[:channels], "fill" if edge == wm.FILL else "replicate", pitches)

    def expected(size, i, scale, bias):
        v = vals[size, i]
        return wm.convert(v, dtype, scale, bias, layout), v, False

    run_cases(torch, ctx, channels, dtype, layout, cc.OUTS, launch, expected, f"warp edge {edge}")


# ---- resized crops over a reduced-size decode (max_prescale 2): tests/scaled_model.py's 1/2 frame under the bilinear model --
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_prescaled_resized_crops(zj, ctx, torch, dtype, layout, channels):
    import scaled_model as sm
    args, planes, _ = cc.scaled_frame(channels)
    d, dev = planes_on_device(zj, torch, args, planes)
    y, cb, cr = [[p.data_ptr()] * N for p in dev]
    for (x, yy, w, h) in cc.SCALED_WINDOWS:
        assert all(sm.prescale_log2(w, h, ow, oh, 1) == 1 for ow, oh in cc.OUTS)
    vals = cc.cached_values("scaled", channels)

    def launch(size, scale, bias, out):
        ctx.decode_crops_resized_device(d, y, cb, cr, cc.SCALED_WINDOWS, size[0], size[1], dtype, layout_code(zj, layout), out, scale,
                                        bias, cc.FLIPS, None, False, 2)

    def expected(size, i, scale, bias):
        v = vals[size, i]
        return from_v(v, dtype, scale, bias, cc.FLIPS[i], layout), v, cc.FLIPS[i]

    run_cases(torch, ctx, channels, dtype, layout, cc.OUTS, launch, expected, "resized crop over a 1/2 decode")
