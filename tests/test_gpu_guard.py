"""GPU: every arm of the IDCT block guard (classify_block, zj_device.h) at its limit on an MI355X.  The frames of
tests/guard_cases.py -- class-1 blocks whose guard bound is GUARD_LIMIT and whose pass-1 results end at +-32 766, class-2 blocks
one weight above, DC-only blocks at 0, 255 and, planted, outside a byte, all three classes in every wave, tables that differ
between the components -- through every kernel that classifies: the fused kernels in every variant the library carries
(zj_decode_planes_device, zj_decode_frames_device), the crop kernel, the crop-tensor kernels, the mixed-geometry crop kernel at
identity size and the reduced decode of 4:2:0 at 1/2.  The expectation is the oracle's bytes (oracle_c.decode_planes), for the
reduced decode scaled_model.decode_scaled; never another call of the library.  Every byte between and around the outputs is
checked to be untouched."""
import ctypes as C
import importlib

import numpy as np
import pytest

import guard_cases as gc
import resize_model as rm
import scaled_model as sm
from test_gpu_crop_tensor import GUARD, convert

pytestmark = pytest.mark.gpu
FILL = 0xAA
CASES = [(name, mode) for name in gc.TABLE_NAMES for mode in gc.MODES]
CASE_IDS = [f"{n}-{m}" for n, m in CASES]


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)  # no GPU -> raises; nothing falls back to the CPU
    yield c
    c.set_variant(0)
    c.close()


@pytest.fixture(scope="module", autouse=True)
def cases_hold():
    """the inputs reach what this file's name promises: stated on the CPU, from the coefficients"""
    gc.assert_cases(verbose=False)


_DEV = {}


def on_device(torch, name, mode, w, h, seed=0):
    """the frame's three planes in device memory (uploaded once per module)"""
    key = (name, mode, w, h, seed)
    if key not in _DEV:
        _DEV[key] = [torch.from_numpy(np.array(p, np.int16)).cuda() for p in gc.frame(name, mode, w, h, seed)[0]]
        torch.cuda.synchronize()  # (the uploads are torch's, the reads the library's stream)
    return _DEV[key]


def kinds_for(w):
    """a GRAYSCALE output of a width off the 16-pixel grid is a reference panic (zj_plan.h: make_plan)"""
    return [k for k in gc.KINDS if k != "gray" or w % 16 == 0]


def desc_of(zj, name, mode, w, h, kind, flags=0, out_pitch=0):
    hs, vs = gc.MODES[mode]
    cs, _, dflags, layout = gc.kind_of(kind)
    return zj.FrameDesc.make(w, h, hs, vs, 3, cs, gc.tables(name), flags=flags | dflags, out_layout=layout, out_pitch=out_pitch)


def guarded(torch, nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


def body(buf, nbytes, what):
    """the output's bytes on the host, after checking the guard bytes in front of it and behind it"""
    a = buf.cpu().numpy()
    assert (a[:GUARD] == FILL).all() and (a[GUARD + nbytes:] == FILL).all(), (what, "a byte outside the output was written")
    return a[GUARD:GUARD + nbytes]


def check_rows(got, exp, what):
    """got: (..., rows, pitch) from the device; exp: (..., rows, row bytes) from the oracle.  The padding keeps the fill."""
    row = exp.shape[-1]
    bad = np.argwhere(got[..., :row] != exp)
    assert bad.size == 0, (what, len(bad), bad[:6].tolist())
    assert (got[..., row:] == FILL).all(), (what, "the padding of a row was written")


def shape_of(kind, h, pitch_or_w):
    return (3, h, pitch_or_w) if kind == "chw" else (h, pitch_or_w)


def variants(zj):
    return zj.variants_available()


# ---- the fused kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", CASES, ids=CASE_IDS)
def test_fused_kernels_match_oracle(zj, ctx, torch, name, mode):
    """batches of two different frames: every shape (aligned and ragged), output kind, flag set and variant"""
    for (w, h) in gc.SHAPES[mode]:
        dev = [on_device(torch, name, mode, w, h, s) for s in (0, 1)]
        cat = [torch.cat([dev[0][c], dev[1][c]]) for c in range(3)]
        for kind in kinds_for(w):
            for flags in gc.FLAG_SETS:
                desc = desc_of(zj, name, mode, w, h, kind, flags)
                out_len = zj.lib().zj_out_len(C.byref(desc))
                exp = [gc.expected(name, mode, w, h, kind, flags, s) for s in (0, 1)]
                assert out_len == exp[0].size
                for variant in variants(zj):
                    ctx.set_variant(variant)
                    buf = guarded(torch, 2 * out_len)
                    ctx.decode_planes_device(desc, 2, cat[0].data_ptr(), cat[1].data_ptr(), cat[2].data_ptr(), buf.data_ptr() + GUARD)
                    ctx.sync()
                    got = body(buf, 2 * out_len, (name, mode, w, h, kind, flags, variant)).reshape((2,) + exp[0].shape)
                    for s in (0, 1):
                        check_rows(got[s], exp[s], (name, mode, w, h, kind, flags, variant, s))


@pytest.mark.parametrize("name,mode", CASES, ids=CASE_IDS)
def test_fused_kernels_padded_rows_and_a_scattered_launch(zj, ctx, torch, name, mode):
    """rows at a pitch of the next multiple of 128 bytes and 128 more; two frames as allocations of their own, handed over
    in descending address order (zj_decode_frames_device)"""
    w, h = gc.SHAPES[mode][0]
    dev = [on_device(torch, name, mode, w, h, s) for s in (0, 1)]
    cat = [torch.cat([dev[0][c], dev[1][c]]) for c in range(3)]
    for kind in ("rgb", "rgba", "ycbcr"):
        exp = [gc.expected(name, mode, w, h, kind, 0, s) for s in (0, 1)]
        pitch = (exp[0].shape[1] + 127) // 128 * 128 + 128
        desc = desc_of(zj, name, mode, w, h, kind, 0, out_pitch=pitch)
        out_len = zj.lib().zj_out_len(C.byref(desc))
        assert out_len == pitch * h
        for variant in variants(zj):
            ctx.set_variant(variant)
            buf = guarded(torch, 2 * out_len)
            ctx.decode_planes_device(desc, 2, cat[0].data_ptr(), cat[1].data_ptr(), cat[2].data_ptr(), buf.data_ptr() + GUARD)
            ctx.sync()
            got = body(buf, 2 * out_len, (name, mode, kind, "pitch", variant)).reshape(2, h, pitch)
            for s in (0, 1):
                check_rows(got[s], exp[s], (name, mode, kind, "pitch", variant, s))
    ctx.set_variant(0)
    desc = desc_of(zj, name, mode, w, h, "rgb")
    out_len = zj.lib().zj_out_len(C.byref(desc))
    own = [[t.clone() for t in dev[s]] for s in (0, 1)]          # allocations of their own
    bufs = [guarded(torch, out_len) for _ in (0, 1)]
    order = sorted((0, 1), key=lambda i: -own[i][0].data_ptr())   # luma planes at falling addresses: not a strided batch
    ctx.decode_frames_device(desc, [own[i][0].data_ptr() for i in order], [own[i][1].data_ptr() for i in order],
                             [own[i][2].data_ptr() for i in order], [bufs[i].data_ptr() + GUARD for i in order])
    ctx.sync()
    for s in (0, 1):
        check_rows(body(bufs[s], out_len, (name, mode, "scattered", s)).reshape(h, -1), gc.expected(name, mode, w, h, "rgb", 0, s),
                   (name, mode, "scattered", s))


# ---- the crop kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", CASES, ids=CASE_IDS)
def test_crop_kernel_matches_oracle(zj, ctx, torch, name, mode):
    """the whole frame, a window inside a redone tile, one inside a tile that is not, one across their seam and one pixel of a
    worst-column block: the oracle's frame, cropped"""
    for (w, h) in gc.SHAPES[mode]:
        dev = on_device(torch, name, mode, w, h)
        for kind in ("rgb", "gray", "chw"):
            if kind not in kinds_for(w):
                continue
            desc = desc_of(zj, name, mode, w, h, kind)
            exp = gc.expected(name, mode, w, h, kind)
            for i, (x, y, ww, hh) in enumerate(gc.windows(name, mode, w, h)):
                row = ww * (1 if kind in ("gray", "chw") else 3)
                pitch = 0 if i % 2 == 0 else (row + 127) // 128 * 128 + 3
                ln = zj.crop_out_len(desc, ww, hh, pitch)
                assert ln == (pitch or row) * hh * (3 if kind == "chw" else 1)
                buf = guarded(torch, ln)
                ctx.decode_crops_device(desc, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], [(x, y)], ww, hh,
                                        [buf.data_ptr() + GUARD], pitch)
                ctx.sync()
                what = (name, mode, w, h, kind, (x, y, ww, hh))
                check_rows(body(buf, ln, what).reshape(shape_of(kind, hh, pitch or row)), gc.crop_of(exp, kind, x, y, ww, hh), what)


# ---- the crop-tensor kernels ------------------------------------------------------------------------------------------------
def crop_hwc(name, mode, w, h, kind, win, seed=0):
    """the oracle's crop as [1, h, w, C] uint8"""
    x, y, ww, hh = win
    return np.ascontiguousarray(gc.crop_of(gc.expected(name, mode, w, h, kind, 0, seed), kind, x, y, ww, hh)).reshape(1, hh, ww, -1)


def layout_code(zj, layout):
    return zj.TENSOR_NHWC if layout == "NHWC" else zj.TENSOR_NCHW


TENSOR_FORMS = [(rm.U8, "NCHW"), (rm.U8, "NHWC"), (rm.F32, "NCHW"), (rm.F32, "NHWC")]
ESZ = {rm.U8: 1, rm.F32: 4}


@pytest.mark.parametrize("name,mode", CASES, ids=CASE_IDS)
def test_crop_tensor_kernel_matches_oracle(zj, ctx, torch, name, mode):
    """the same windows into u8 and f32 tensors (scale 1, bias 0), NCHW and NHWC: the conversion of the oracle's crop"""
    for (w, h) in gc.SHAPES[mode]:
        dev = on_device(torch, name, mode, w, h)
        for kind in ("rgb", "gray"):
            if kind not in kinds_for(w):
                continue
            desc = desc_of(zj, name, mode, w, h, kind)
            ch = 1 if kind == "gray" else 3
            for win in gc.windows(name, mode, w, h):
                for (dtype, layout) in TENSOR_FORMS:
                    per = zj.crop_tensor_out_len(desc, win[2], win[3], dtype)
                    assert per == ch * win[2] * win[3] * ESZ[dtype]
                    buf = guarded(torch, per)
                    ctx.decode_crops_tensor_device(desc, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], [win[:2]], win[2],
                                                   win[3], dtype, layout_code(zj, layout), buf.data_ptr() + GUARD)
                    ctx.sync()
                    what = (name, mode, w, h, kind, win, dtype, layout)
                    got = body(buf, per, what)
                    want = convert(crop_hwc(name, mode, w, h, kind, win), dtype, layout, None, None, None)
                    assert np.array_equal(got, want), (what, int((got != want).sum()))


def mixed_frames(zj, torch, names=("q50", "cross", "flat16", "q10")):
    """the first shape of every mode, each under another table set: (name, mode, w, h, descriptor, device planes)"""
    out = []
    for name, mode in zip(names, ("420", "444", "422", "440")):
        w, h = gc.SHAPES[mode][0]
        out.append((name, mode, w, h, desc_of(zj, name, mode, w, h, "rgb"), on_device(torch, name, mode, w, h)))
    return out


@pytest.mark.parametrize("dtype,layout", TENSOR_FORMS)
def test_crop_tensor_mixed_call_matches_oracle(zj, ctx, torch, dtype, layout):
    """4:2:0 and 4:4:4 frames (and the two other modes) with different tables in one mixed call, one window size: inside a
    redone tile, inside one that is not, across their seam"""
    fr = mixed_frames(zj, torch)
    for pick in (1, 2, 3):
        wins = [gc.windows(n, m, w, h)[pick] for (n, m, w, h, _, _) in fr]
        ww, hh = min(v[2] for v in wins), min(v[3] for v in wins)
        per = 3 * ww * hh * ESZ[dtype]
        buf = guarded(torch, len(fr) * per)
        ctx.decode_crops_tensor_mixed_device([f[4] for f in fr], [f[5][0].data_ptr() for f in fr], [f[5][1].data_ptr() for f in fr],
                                             [f[5][2].data_ptr() for f in fr], [v[:2] for v in wins], ww, hh, dtype,
                                             layout_code(zj, layout), buf.data_ptr() + GUARD)
        ctx.sync()
        got = body(buf, len(fr) * per, (pick, dtype, layout))
        want = np.concatenate([convert(crop_hwc(n, m, w, h, "rgb", (v[0], v[1], ww, hh)), dtype, layout, None, None, None)
                               for (n, m, w, h, _, _), v in zip(fr, wins)])
        assert np.array_equal(got, want), (pick, dtype, layout, int((got != want).sum()))


# ---- the mixed-geometry crop kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", CASES, ids=CASE_IDS)
def test_mixed_crop_kernel_at_identity_size_matches_oracle(zj, ctx, torch, name, mode):
    """zj_decode_crops_resized_mixed_device with out == window into u8 (the bilinear resize is then the identity): the crops
    zj_crop_mixed.hip decodes, against the oracle's"""
    for (w, h) in gc.SHAPES[mode]:
        dev = on_device(torch, name, mode, w, h)
        desc = desc_of(zj, name, mode, w, h, "rgb")
        for win in gc.windows(name, mode, w, h):
            per = 3 * win[2] * win[3]
            buf = guarded(torch, per)
            ctx.decode_crops_resized_mixed_device([desc], [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], [win], win[2],
                                                  win[3], rm.U8, zj.TENSOR_NHWC, buf.data_ptr() + GUARD)
            ctx.sync()
            what = (name, mode, w, h, win)
            check_rows(body(buf, per, what).reshape(win[3], -1), gc.crop_of(gc.expected(name, mode, w, h, "rgb"), "rgb", *win), what)


def test_mixed_crop_kernel_takes_every_mode_and_table_set_in_one_call(zj, ctx, torch):
    fr = mixed_frames(zj, torch)
    for pick in (1, 2, 3):
        wins = [gc.windows(n, m, w, h)[pick] for (n, m, w, h, _, _) in fr]
        ww, hh = min(v[2] for v in wins), min(v[3] for v in wins)
        wins = [(v[0], v[1], ww, hh) for v in wins]
        per = 3 * ww * hh
        buf = guarded(torch, len(fr) * per)
        ctx.decode_crops_resized_mixed_device([f[4] for f in fr], [f[5][0].data_ptr() for f in fr], [f[5][1].data_ptr() for f in fr],
                                              [f[5][2].data_ptr() for f in fr], wins, ww, hh, rm.U8, zj.TENSOR_NHWC,
                                              buf.data_ptr() + GUARD)
        ctx.sync()
        got = body(buf, len(fr) * per, pick).reshape(len(fr), hh, -1)
        for i, ((n, m, w, h, _, _), v) in enumerate(zip(fr, wins)):
            check_rows(got[i], gc.crop_of(gc.expected(n, m, w, h, "rgb"), "rgb", *v), (pick, n, m))


# ---- the reduced decode ------------------------------------------------------------------------------------------------------
SCALED_KINDS = {"rgb": sm.RGB, "ycbcr": sm.YCBCR, "chw": sm.RGB}


@pytest.mark.parametrize("name", gc.TABLE_NAMES)
def test_reduced_decode_of_420_matches_the_model(zj, ctx, torch, name):
    """4:2:0 at 1/2: the chroma blocks take the full transform behind classify_block (scaled_finish); at 1/4, on the same
    planes, nothing is classified -- the control"""
    for (w, h) in gc.SHAPES["420"]:
        dev = on_device(torch, name, "420", w, h)
        planes, qts = gc.frame(name, "420", w, h)
        for kind, cs in SCALED_KINDS.items():
            desc = desc_of(zj, name, "420", w, h, kind)
            for scale, sl in ((2, 1), (4, 2)):
                exp = sm.decode_scaled(w, h, 2, 2, 3, cs, qts, planes, sl, chw=kind == "chw")
                rw, rh = zj.scaled_size(desc, scale)
                ln = zj.scaled_crop_out_len(desc, scale, rw, rh, 0)
                assert ln == exp.size
                buf = guarded(torch, ln)
                ctx.decode_crops_scaled_device(desc, [dev[0].data_ptr()], [dev[1].data_ptr()], [dev[2].data_ptr()], scale,
                                               [buf.data_ptr() + GUARD])
                ctx.sync()
                what = (name, w, h, kind, scale)
                got = body(buf, ln, what).reshape(exp.shape)
                assert np.array_equal(got, exp), (what, int((got != exp).sum()))


def test_reduced_decode_through_the_mixed_geometry_path(zj, ctx, torch):
    """zj_scaled_mixed.hip: 4:2:0 frames of two sizes and three table sets, max_prescale 2 and out == window / 2, so that the
    reduced crop leaves through an identity resize; against the model's reduced frame"""
    specs = [("cross", 528, 64), ("q50", 272, 48), ("flat1", 530, 64)]
    ww, hh = 264, 48
    descs = [desc_of(zj, n, "420", w, h, "rgb") for (n, w, h) in specs]
    devs = [on_device(torch, n, "420", w, h) for (n, w, h) in specs]
    per = 3 * (ww // 2) * (hh // 2)
    buf = guarded(torch, len(specs) * per)
    ctx.decode_crops_resized_mixed_device(descs, [d[0].data_ptr() for d in devs], [d[1].data_ptr() for d in devs],
                                          [d[2].data_ptr() for d in devs], [(4, 0, ww, hh)] * len(specs), ww // 2, hh // 2, rm.U8,
                                          zj.TENSOR_NHWC, buf.data_ptr() + GUARD, max_prescale=2)
    ctx.sync()
    got = body(buf, len(specs) * per, "mixed reduced").reshape(len(specs), hh // 2, ww // 2, 3)
    for i, (n, w, h) in enumerate(specs):
        planes, qts = gc.frame(n, "420", w, h)
        exp = sm.decode_scaled(w, h, 2, 2, 3, sm.RGB, qts, planes, 1)[:hh // 2, 2:2 + ww // 2]
        assert np.array_equal(got[i], exp), (n, w, h, int((got[i] != exp).sum()))
