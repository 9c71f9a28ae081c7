"""CPU: the conversion-edge cases (tests/convert_cases.py) through every emulation build whose store ends in zj_resize.h's
conversions -- emu_resize, emu_resize_aa, emu_resize_bicubic, emu_to_tensor, emu_crop_tensor, emu_warp -- against the stage's
numpy model, bit for bit, compared as integers.  The emulations convert in software (resize_f16_bits, resize_bf16_bits); this
takes them from scalar spot values to whole images whose elements sit on the edges of float32, half and bfloat16
(test_convert_cases.py counts them), and shows that model and emulation agree there before anything runs on a GPU.  A
mismatch names the edge class of the first differing element."""
import numpy as np
import pytest

import convert_cases as cc
import emu_crop_c as ec
import emu_crop_tensor_c as ect
import emu_resize_aa_c as ea
import emu_resize_bicubic_c as eb
import emu_resize_c as er
import emu_to_tensor_c as et
import emu_warp_c as ew
import resize_aa_model as am
import resize_bicubic_model as bm
import resize_model as rm
import warp_model as wm

pytestmark = pytest.mark.filterwarnings("ignore:overflow encountered")  # (the models overflow to inf on purpose)
LAYOUTS = ["NCHW", "NHWC"]
DTYPES = [cc.F32, cc.F16, cc.BF16, cc.U8]
IDS = ["f32", "f16", "bf16", "u8"]
GUARD, POISON = 64, 0xAA


def factor_cases(channels, dtype):
    """U8 takes no factors: one launch"""
    cases = list(cc.factor_cases(channels))
    return cases[:1] if dtype == cc.U8 else cases


def hwc_buffers(imgs, pad):
    """[C, h, w] images as interleaved rows at a pitch of their own: (buffers, pitches)"""
    bufs, pitches = [], []
    for i, img in enumerate(imgs):
        c, h, w = img.shape
        pitch = w * c + pad[i % len(pad)]
        buf = np.full((h, pitch), 0xEE, np.uint8)
        buf[:, :w * c] = img.transpose(1, 2, 0).reshape(h, w * c)
        bufs.append(buf.reshape(-1))
        pitches.append(pitch)
    return bufs, pitches


RESIZERS = {"resize": (er, rm), "resize_aa": (ea, am), "resize_bicubic": (eb, bm)}


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("stage", list(RESIZERS))
def test_resizes(stage, dtype, layout, channels):
    emu, model = RESIZERS[stage]
    imgs = cc.images(*cc.SRC, channels)
    bufs, pitches = hwc_buffers(imgs, [0, 5, 1, 13])
    vals = cc.cached_values(stage, channels)
    esz = et.ELEM[dtype]
    for (ow, oh) in cc.OUTS:
        per = channels * ow * oh * esz
        for name, scale, bias in factor_cases(channels, dtype):
            s, b = rm.factors(channels, scale, bias)
            out = emu.resize(bufs, [cc.SRC] * len(imgs), pitches, channels, False, ow, oh, dtype, layout == "NHWC", s, b, cc.FLIPS)
            for i, img in enumerate(imgs):
                exp = model.resize(img, ow, oh, dtype, scale, bias, cc.FLIPS[i], layout)
                cc.check(out[i * per:(i + 1) * per], exp, dtype, vals[(ow, oh), i], scale, bias, cc.FLIPS[i], layout,
                         f"{stage} {name} image {i} -> {ow}x{oh}")


def aligned(n, to=64):
    buf = np.empty(n + to, np.uint8)
    off = (-buf.ctypes.data) % to
    return buf[off:off + n]


def three(x, fill):
    out = np.full(3, fill, np.float32)
    out[:len(x)] = x
    return out


@pytest.mark.parametrize("chans", [(1, 1), (1, 3), (3, 3)], ids=["1to1", "1to3", "3to3"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_to_tensor(dtype, layout, chans):
    cin, cout = chans
    esz = et.ELEM[dtype]
    for (w, h) in cc.OUTS:
        imgs = cc.images(w, h, cin)
        bufs, pitches = hwc_buffers(imgs, [0, 1, 13, 0])
        shown = [np.repeat(im, cout, axis=0) if cin != cout else im for im in imgs]
        per = cout * w * h * esz
        for name, scale, bias in factor_cases(cout, dtype):
            s, b = rm.factors(cout, scale, bias)
            arena = aligned(2 * GUARD + esz + len(imgs) * per)
            arena[:] = POISON
            off = GUARD + esz  # (one element off a 64-byte boundary)
            wmap, outside, bad_loads = et.to_tensor([x.ctypes.data for x in bufs], w, h, pitches, cin, cout, dtype, layout == "NHWC",
                                                    three(s, 1), three(b, 0), cc.FLIPS, arena, off)
            assert outside == 0 and bad_loads == 0
            assert (arena[:off] == POISON).all() and (arena[off + len(imgs) * per:] == POISON).all()
            for i, img in enumerate(shown):
                exp = rm.resize(img, w, h, dtype, scale, bias, cc.FLIPS[i], layout)
                cc.check(arena[off + i * per:off + (i + 1) * per], exp, dtype, img.astype(np.int64) << 16, scale, bias, cc.FLIPS[i],
                         layout, f"to_tensor {cin}->{cout} {name} image {i} {w}x{h}")


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_crop_tensor(dtype, layout, channels):
    """windows over the frame's last rows, which the reference leaves at zero: the stage's fill path converts a zero byte"""
    args, planes, _ = cc.crop_frame(channels)
    d = ec.desc(*args)
    esz = ect.ELEM[dtype]
    for (w, h) in cc.OUTS:
        origins = cc.CROP_ORIGINS[w, h]
        crops = cc.crop_sources(channels, (w, h))
        assert any(not c[:, -1].any() for c in crops), "no window reaches the rows that stay zero"
        per = channels * w * h * esz
        for name, scale, bias in factor_cases(channels, dtype):
            rc, buf = ect.decode_crops_tensor(d, [planes] * len(origins), origins, w, h, dtype, layout, scale, bias, cc.FLIPS)
            assert rc == 0
            for i, crop in enumerate(crops):
                exp = rm.resize(crop, w, h, dtype, scale, bias, cc.FLIPS[i], layout)
                cc.check(buf[i * per:(i + 1) * per], exp, dtype, crop.astype(np.int64) << 16, scale, bias, cc.FLIPS[i], layout,
                         f"crop_tensor {name} window {i} {w}x{h}")


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("edge", [wm.FILL, wm.REPLICATE], ids=["fill", "replicate"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_warp(dtype, layout, edge, channels):
    imgs = cc.images(*cc.SRC, channels)
    bufs, pitches = hwc_buffers(imgs, [0, 1, 13, 0])
    hwc = [im.transpose(1, 2, 0) for im in imgs]
    vals = cc.cached_values("warp_fill" if edge == wm.FILL else "warp_replicate", channels)
    esz = ew.ELEM[dtype]
    for (ow, oh) in cc.OUTS:
        ints = [wm.fixed(m) for m in cc.warp_matrices(*cc.SRC, ow, oh)]
        per = channels * ow * oh * esz
        for name, scale, bias in factor_cases(channels, dtype):
            s, b = rm.factors(channels, scale, bias)
            arena = aligned(2 * GUARD + esz + len(imgs) * per)
            arena[:] = POISON
            off = GUARD + esz
            wmap, outside, bad_loads, _ = ew.warp([x.ctypes.data for x in bufs], [cc.SRC] * len(imgs), pitches, channels, ints, ow, oh,
                                                  dtype, layout == "NHWC", three(s, 1), three(b, 0), cc.WARP_FILL, edge, arena, off)
            assert outside == 0 and bad_loads == 0
            assert (arena[:off] == POISON).all() and (arena[off + len(imgs) * per:] == POISON).all()
            for i, img in enumerate(hwc):
                exp = wm.warp(img, ints[i], ow, oh, dtype, scale, bias, edge, cc.WARP_FILL, layout)
                cc.check(arena[off + i * per:off + (i + 1) * per], exp, dtype, vals[(ow, oh), i], scale, bias, False, layout,
                         f"warp edge {edge} {name} image {i} -> {ow}x{oh}")
