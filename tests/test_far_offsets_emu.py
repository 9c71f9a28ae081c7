"""CPU: the stages' and the decode paths' address arithmetic past 2^31 and 2^32 bytes (far_cases.py).  The emulations under
tests/emu_* compile the kernels' own headers with g++, so a product narrowed to 32 bits overflows there exactly as on the
device; they count the stores (and, where they have a read map, the loads) that fall outside the caller's arena instead of
performing them.  Every image here is a few thousand pixels whose rows lie up to 2^24 (stages) or 2^20 (decode outputs) bytes
apart in a zero buffer that is committed only where it is touched, the input and the output side far at once.  Per case:
no access outside, every image byte written exactly once and no other byte of the gigabytes around them, the values equal
to the stage's model.  Each test asserts its premise -- the largest row offset it makes the kernel form is >= 2^32 -- so a
later change of a limit turns it red, not vacuous."""
import ctypes as C
import importlib

import numpy as np
import pytest

import far_cases as fc
from far_cases import Far

PITCHES = pytest.mark.parametrize("pitch", fc.STAGE_PITCHES, ids=["limit", "odd"])
LAYOUTS = pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
WIDTHS = pytest.mark.parametrize("w", fc.STAGE_WIDTHS)


def stage_shape(chw, w):
    """(planes, h, row bytes) of a 3-channel image w wide at the stage heights"""
    return (3, fc.STAGE_H_CHW, w) if chw else (1, fc.STAGE_H_HWC, 3 * w)


def image_of(far, chw):
    """[3, h, w] (CHW) or [h, w, 3]"""
    return far.rows if chw else far.rows[0].reshape(far.h, -1, 3)


def rows_of(img, chw):
    return img if chw else img.reshape(1, img.shape[0], -1)


def assert_rows(far, want, what):
    """far.rows == want, the rows beside the 2^31 and 2^32 lines named first"""
    got = far.rows.reshape(far.planes * far.h, -1)
    want = np.asarray(want).reshape(got.shape)
    for r in far.far_rows():
        assert np.array_equal(got[r], want[r]), f"{what}: row {r} (offset {r * far.pitch:#x}) differs"
    assert np.array_equal(got, want), what


def test_the_limits_are_the_librarys():
    """OUT_PITCH_MAX through the three length calls (STAGE_PITCH_MAX: test_stage_pack.py).  zj_out_len is make_plan's
    arithmetic without its checks -- a length for any descriptor -- so the frame call's refusal of a pitch above the limit is
    asserted where a context exists (test_gpu_far_offsets.py); the crop and the reduced plans refuse it here."""
    zj = importlib.import_module("zune-jpeg_amd")
    qts = [np.ones(64, np.uint16)] * 3
    for layout, w in ((0, 48), (0, 37), (1, 48)):
        ok = zj.FrameDesc.make(w, 64, 1, 1, 3, zj.ColorSpace.RGB, qts, out_layout=layout, out_pitch=fc.OUT_PITCH_MAX)
        assert zj.lib().zj_out_len(C.byref(ok)) == fc.OUT_PITCH_MAX * 64 * (3 if layout else 1)
        d = zj.FrameDesc.make(w, 64, 1, 1, 3, zj.ColorSpace.RGB, qts, out_layout=layout)
        assert zj.crop_out_len(d, 16, 8, fc.OUT_PITCH_MAX) == fc.OUT_PITCH_MAX * 8 * (3 if layout else 1)
        assert zj.crop_out_len(d, 16, 8, fc.OUT_PITCH_MAX + 16) == 0
        assert zj.scaled_crop_out_len(d, 2, 16, 8, fc.OUT_PITCH_MAX) == fc.OUT_PITCH_MAX * 8 * (3 if layout else 1)
        assert zj.scaled_crop_out_len(d, 2, 16, 8, fc.OUT_PITCH_MAX + 16) == 0


def test_the_geometry_crosses_both_lines():
    for pitch in fc.STAGE_PITCHES:
        assert fc.crosses(pitch, fc.STAGE_H_HWC) and fc.crosses(pitch, fc.STAGE_H_CHW, 3)
        assert not fc.crosses(pitch, fc.STAGE_H_HWC - 2)  # (258 is the smallest height at which the odd pitch does)
        rows = fc.lines(pitch, fc.STAGE_H_HWC)
        assert rows[0] == 0 and rows[-1] == fc.STAGE_H_HWC - 1 and {127, 128, 129, 255, 256, 257} <= set(rows)
    assert fc.STAGE_PITCHES[0] * 256 == fc.LINE32 and fc.STAGE_PITCHES[1] % 2 == 1
    for w in fc.OUT_WIDTHS:
        for pitch in fc.out_pitches(w):
            assert pitch <= fc.OUT_PITCH_MAX and (w % 16 or pitch % 16 == 0)
            assert fc.crosses(pitch, fc.OUT_H_HWC) and fc.crosses(pitch, fc.OUT_H_CHW, 3)
    assert fc.OUT_PITCH_MAX * 4096 == fc.LINE32


# ---- the pitched u8 stages: input and output far at once ---------------------------------------------------------------

@pytest.mark.parametrize("o", range(1, 9))
@LAYOUTS
def test_orient(chw, o):
    """stored 37 x H and H x 37: under the transposing orientations the second one's OUTPUT is the tall image"""
    import emu_orient_c as eo
    import orient_model as om
    H = fc.STAGE_H_CHW if chw else fc.STAGE_H_HWC
    bpp, npl = (1, 3) if chw else (3, 1)
    rng = np.random.default_rng(100 + o)
    for pitch in fc.STAGE_PITCHES:
        for w, h in ((37, H), (H, 37)) if o >= 5 else ((37, H),):
            dw, dh = om.oriented_size(o, w, h)
            src = Far(npl, h, w * bpp, pitch).fill(rng)
            dst = Far(npl, dh, dw * bpp, pitch)
            assert fc.crosses(pitch, max(h, dh), npl), "no offset of this case reaches 2^32"
            wmap, outside = eo.orient([src.buf], [(w, h)], [pitch], 3, chw, [o], dst.buf, [0], [pitch], zeros=fc.zeros)
            what = f"orient {o} stored {w}x{h} pitch {pitch}"
            assert outside == 0, f"{what}: {outside} stores outside the arena"
            assert dst.once(wmap), f"{what}: an image byte not written exactly once, or a padding byte written"
            img = image_of(src, chw)
            assert_rows(dst, rows_of(om.orient_chw(img, o) if chw else om.orient(img, o), chw), what)


@PITCHES
@LAYOUTS
@WIDTHS
def test_gray_to_rgb(w, chw, pitch):
    import emu_expand_c as ex
    npl, h, rb = stage_shape(chw, w)
    src = Far(1, h, w, pitch).fill(np.random.default_rng(w))
    dst = Far(npl, h, rb, pitch)
    assert fc.crosses(pitch, h, npl) and (chw or fc.crosses(pitch, src.h))
    wmap, outside = ex.expand([src.buf.ctypes.data], [(w, h)], [pitch], chw, dst.buf, [0], [pitch], zeros=fc.zeros)
    assert outside == 0 and dst.once(wmap)
    g = src.rows[0]
    assert_rows(dst, np.stack([g, g, g]) if chw else np.repeat(g, 3, axis=1), "gray to RGB")


@PITCHES
@LAYOUTS
@WIDTHS
def test_cmyk(w, chw, pitch):
    """a, k and the output each at the far pitch"""
    import cmyk_stage_cases as sc
    import emu_cmyk_c as ck
    npl, h, rb = stage_shape(chw, w)
    rng = np.random.default_rng(w + 1)
    a, k = Far(npl, h, rb, pitch).fill(rng), Far(1, h, w, pitch).fill(rng)
    dst = Far(npl, h, rb, pitch)
    assert fc.crosses(pitch, h, npl)
    for inverted in (0, 1):
        wmap, outside = ck.combine([a.buf.ctypes.data], [k.buf.ctypes.data], [(w, h)], [pitch], [pitch], chw, [inverted], dst.buf,
                                   [0], [pitch], zeros=fc.zeros)
        assert outside == 0 and dst.once(wmap)
        want = sc.combine(image_of(a, chw), k.rows if chw else k.rows[0][:, :, None], inverted)
        assert_rows(dst, rows_of(want.astype(np.uint8), chw), f"cmyk inverted {inverted}")


@PITCHES
@LAYOUTS
def test_planes(chw, pitch):
    """three planes at the far pitch, ratios 1, 2 and 4 across and 1, 1 and 2 down with odd phases, so that the first two
    planes are as tall as the image and the third crosses 2^31"""
    import emu_planes_c as pk
    import planes_cases as pc
    w = 37
    npl, h, rb = stage_shape(chw, w)
    geo = ((1, 1, 0, 0), (2, 1, 1, 0), (4, 2, 3, 1))
    rng = np.random.default_rng(9)
    sizes = [pc.plane_size(w, h, g) for g in geo]
    offs = [0]
    for pw, ph in sizes:
        offs.append(offs[-1] + ph * pitch)
    src, needed = fc.zeros(offs[-1]), fc.zeros(offs[-1])
    planes = []
    for (pw, ph), o in zip(sizes, offs):
        rows = src[o:o + ph * pitch].reshape(ph, pitch)[:, :pw]
        rows[...] = rng.integers(0, 256, rows.shape, dtype=np.uint8)
        needed[o:o + ph * pitch].reshape(ph, pitch)[:, :pw] = 1
        planes.append(rows)
    dst = Far(npl, h, rb, pitch)
    assert fc.crosses(pitch, h, npl) and fc.crosses(pitch, sizes[1][1], 1, fc.LINE31)
    assert chw or (fc.crosses(pitch, sizes[1][1]) and fc.crosses(pitch, sizes[2][1], 1, fc.LINE31))
    for stored_rgb in (False, True):
        wmap, outside, bad = pk.combine(src, needed, [offs[:3]], [(pitch,) * 3], [(w, h)], [geo], stored_rgb, chw, dst.buf, [0], [pitch],
                                        zeros=fc.zeros)
        assert outside == 0 and bad == 0 and dst.once(wmap)
        e = pc.combine(planes, geo, w, h, stored_rgb).reshape(h, w, 3)
        assert_rows(dst, e.transpose(2, 0, 1) if chw else e.reshape(1, h, 3 * w), f"planes stored_rgb {stored_rgb}")


@PITCHES
@LAYOUTS
@WIDTHS
def test_color(w, chw, pitch):
    """apart, and in place over the same rows"""
    import color_cases as cc
    import color_model as cm
    import emu_color_c as ce
    npl, h, rb = stage_shape(chw, w)
    src = Far(npl, h, rb, pitch).fill(np.random.default_rng(w + 2))
    dst = Far(npl, h, rb, pitch)
    assert fc.crosses(pitch, h, npl)
    q = cm.fixed(cc.jitter())
    want = rows_of(cm.apply_fixed(q, image_of(src, chw), chw), chw)
    rmap, wmap, outside = ce.color(src.buf, [0], [(w, h)], [pitch], chw, [q], dst.buf, [0], [pitch], zeros=fc.zeros)
    assert outside == 0 and dst.once(wmap) and src.once(rmap)
    assert_rows(dst, want, "colour, apart")
    rmap, wmap, outside = ce.color(src.buf, [0], [(w, h)], [pitch], chw, [q], src.buf, [0], [pitch], zeros=fc.zeros)
    assert outside == 0 and src.once(wmap) and src.once(rmap)
    assert_rows(src, want, "colour, in place")


# ---- the tensor stages: far inputs, dense outputs -----------------------------------------------------------------------

def _factors(ch):
    import resize_model as rm
    scale, bias = np.float32([0.02, 0.015, 0.01])[:ch], np.float32([-1.5, 0.25, 2.0])[:ch]
    s, b = rm.factors(ch, scale, bias)
    s3, b3 = np.ones(3, np.float32), np.zeros(3, np.float32)
    s3[:ch], b3[:ch] = s, b
    return scale, bias, s3, b3


@PITCHES
@pytest.mark.parametrize("kind", ["bilinear", "antialiased", "bicubic"])
@LAYOUTS
def test_resize_inputs(chw, kind, pitch):
    """every source row is a tap: the output is as tall as the source (bilinear: each row its own) and narrower"""
    import resize_model as rm
    emu, model = {"bilinear": ("emu_resize_c", "resize_model"), "antialiased": ("emu_resize_aa_c", "resize_aa_model"),
                  "bicubic": ("emu_resize_bicubic_c", "resize_bicubic_model")}[kind]
    emu, model = importlib.import_module(emu), importlib.import_module(model)
    w = 37
    npl, h, rb = stage_shape(chw, w)
    src = Far(npl, h, rb, pitch).fill(np.random.default_rng(5))
    assert fc.crosses(pitch, h, npl)
    scale, bias, s3, b3 = _factors(3)
    img = src.rows if chw else src.rows[0].reshape(h, w, 3).transpose(2, 0, 1)
    for ow, oh in ((29, h), (16, 9)):
        out = emu.resize([src.buf], [(w, h)], [pitch], 3, chw, ow, oh, rm.F32, True, s3, b3, [False])
        exp = model.resize(img, ow, oh, rm.F32, scale, bias, False, "NHWC").reshape(-1)
        assert np.array_equal(rm.raw_view(out, rm.F32).view(np.uint32), exp.view(np.uint32)), (kind, ow, oh)


@PITCHES
@pytest.mark.parametrize("cin,cout", [(1, 3), (3, 3)])
@WIDTHS
def test_to_tensor_inputs(w, cin, cout, pitch):
    import emu_to_tensor_c as et
    import resize_model as rm
    h = fc.STAGE_H_HWC
    src = Far(1, h, w * cin, pitch).fill(np.random.default_rng(w + cin))
    assert fc.crosses(pitch, h)
    scale, bias, s3, b3 = _factors(cout)
    for flip in (False, True):
        arena = np.zeros(cout * w * h * 4, np.uint8)
        wmap, outside, bad_loads = et.to_tensor([src.buf.ctypes.data], w, h, [pitch], cin, cout, rm.F32, True, s3, b3, [flip], arena, 0)
        assert outside == 0 and bad_loads == 0 and wmap.min() == 1 == wmap.max()
        chw_img = src.rows[0].reshape(h, w, cin).transpose(2, 0, 1)
        if cin != cout:
            chw_img = np.repeat(chw_img, cout, axis=0)
        exp = np.ascontiguousarray(rm.resize(chw_img, w, h, rm.F32, scale, bias, flip, "NHWC")).view(np.uint8).reshape(-1)
        assert np.array_equal(arena, exp), (w, cin, cout, flip)


@PITCHES
@pytest.mark.parametrize("ch", [1, 3])
def test_warp_inputs(ch, pitch):
    """the identity, the half turn and a 17-degree rotation about the centre over a 37 x 258 source: taps in every row"""
    import math

    import emu_warp_c as ew
    import resize_model as rm
    import warp_model as wm
    w, h = 37, fc.STAGE_H_HWC
    src = Far(1, h, w * ch, pitch).fill(np.random.default_rng(ch))
    assert fc.crosses(pitch, h)
    scale, bias, s3, b3 = _factors(ch)
    co, si = math.cos(math.radians(17)), math.sin(math.radians(17))
    cx, cy = w / 2, h / 2
    ms = [wm.orientation_matrix(1, w, h), wm.orientation_matrix(3, w, h),
          (co, -si, cx - co * cx + si * cy, si, co, cy - si * cx - co * cy)]
    img = src.rows[0].reshape(h, w, ch)
    for m in ms:
        q = wm.fixed(m)
        assert q is not None
        arena = np.zeros(ch * w * h * 4, np.uint8)
        wmap, outside, bad_loads, loads = ew.warp([src.buf.ctypes.data], [(w, h)], [pitch], ch, [q], w, h, rm.F32, True, s3, b3,
                                                  (7, 130, 255), wm.FILL, arena, 0)
        assert outside == 0 and bad_loads == 0 and loads > 0 and wmap.min() == 1 == wmap.max()
        exp = np.ascontiguousarray(wm.warp(img, q, w, h, rm.F32, scale, bias, wm.FILL, (7, 130, 255), "NHWC")).view(np.uint8).reshape(-1)
        assert np.array_equal(arena, exp), m


# ---- the decode paths: output rows 2^20 bytes apart --------------------------------------------------------------------

MODES = {"444": (1, 1), "420": (2, 2)}
KINDS = ["rgb", "gray", "chw"]
POISON = 0xAA


def out_shape(kind, w):
    """(planes, h, row bytes) of a decode output w wide at the output heights"""
    return {"rgb": (1, fc.OUT_H_HWC, 3 * w), "gray": (1, fc.OUT_H_HWC, w), "chw": (3, fc.OUT_H_CHW, w)}[kind]


def oracle_rows(kind, w, h, hs, vs, qts, planes):
    """the full tight decode as [planes * h, row bytes]"""
    import oracle_c as oc
    f = oc.make_frame(w, h, hs, vs, 3, oc.GRAYSCALE if kind == "gray" else oc.RGB, qts)
    rc, exp = oc.decode_planes(f, planes, plain=True) if kind == "chw" else oc.decode_planes(f, planes)
    assert rc == 0
    if kind == "chw":
        return np.ascontiguousarray(exp.reshape(h, w, 3).transpose(2, 0, 1)).reshape(3 * h, w)
    return exp.reshape(h, -1)


def refused_by_the_reference(kind, w, h, hs, vs, qts, planes):
    """a frame the reference panics on (a ragged gray row under 4:2:0): the paths refuse it too, and no offset is formed"""
    import oracle_c as oc
    f = oc.make_frame(w, h, hs, vs, 3, oc.GRAYSCALE if kind == "gray" else oc.RGB, qts)
    return oc.decode_planes(f, planes)[0] != 0


def far_output(kind, h, row_bytes, pitch):
    """a zero buffer whose image rows alone hold POISON: a row the path must zero and does not, and a byte it must not
    write and does, both show"""
    far = Far(3 if kind == "chw" else 1, h, row_bytes, pitch)
    far.rows[...] = POISON
    return far


def check_far_output(far, want, zero_rows, what):
    """the image's rows equal `want`, the zeroed ones lie past 2^32, and no byte of the padding is anything but zero (where
    the frame call zeroes uncovered rows whole -- Q6, test_gpu_pitch.py -- that is zeros over zeros)"""
    assert_rows(far, want, what)
    got = far.rows.reshape(far.planes * far.h, -1)
    assert zero_rows and not got[zero_rows].any() and not np.asarray(want).reshape(got.shape)[zero_rows].any(), what
    assert max(zero_rows) * far.pitch >= fc.LINE32, f"{what}: no zeroed row lies past 2^32"
    assert int(np.count_nonzero(far.buf)) == int(np.count_nonzero(got)), f"{what}: a padding byte was written"


def uncovered(kind, h, hs, vs):
    """the rows (through the planes) below the last complete strip"""
    mcu_y = -(-h // (8 * vs))
    covered = min(h, (mcu_y // 2 if hs == 2 else mcu_y) * 8 * vs * (2 if hs == 2 else 1))
    return [p * h + r for p in range(3 if kind == "chw" else 1) for r in range(covered, h)]


OUT_PITCH = pytest.mark.parametrize("which", [0, 1], ids=["limit", "below"])


@OUT_PITCH
@pytest.mark.parametrize("w", fc.OUT_WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", list(MODES))
def test_frame_decode(mode, kind, w, which, synth):
    """the three generations of the fused kernel at the limit, the default one below it"""
    import emu_c
    import oracle_c as oc
    hs, vs = MODES[mode]
    npl, h, rb = out_shape(kind, w)
    planes, qts = synth.make_frame(w, h, hs, vs, 3, seed=w + h)
    f = oc.make_frame(w, h, hs, vs, 3, oc.GRAYSCALE if kind == "gray" else oc.RGB, qts)
    pitch = fc.out_pitches(w)[which]
    if refused_by_the_reference(kind, w, h, hs, vs, qts, planes):
        assert emu_c.decode_planes(f, planes, out_pitch=pitch, out=fc.zeros(npl * h * pitch))[0] != 0
        return
    want = oracle_rows(kind, w, h, hs, vs, qts, planes)
    zero_rows = uncovered(kind, h, hs, vs)
    assert bool(zero_rows) == (hs == 2)
    try:
        for variant in (0, 1, 2) if which == 0 else (0,):
            emu_c.set_variant(variant)
            assert fc.crosses(pitch, h, npl)
            far = far_output(kind, h, rb, pitch)
            rc, _ = emu_c.decode_planes(f, planes, out_layout=1 if kind == "chw" else 0, out_pitch=pitch, out=far.buf)
            assert rc == 0
            what = f"frame {mode} {kind} {w}x{h} pitch {pitch} variant {variant}"
            assert_rows(far, want, what)
            if zero_rows:
                check_far_output(far, want, zero_rows, what)
            else:
                assert int(np.count_nonzero(far.buf)) == int(np.count_nonzero(far.rows)), f"{what}: a padding byte was written"
    finally:
        emu_c.set_variant(0)


@OUT_PITCH
@pytest.mark.parametrize("w", fc.OUT_WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", list(MODES))
def test_crop_decode(mode, kind, w, which, synth):
    """a window at the odd origin (3, 5) that ends with the frame.  4:4:4: the copy-out's last strip begins at crop row 4099
    (frame row 4104), so the product row x pitch that places a strip passes 2^32 at both pitches.  4:2:0: strips are 32 rows,
    none can begin that late in a window of 4100, but the crop's last nine rows are the frame's uncovered ones: the zeroed
    rows pass 2^32.  CHW: the third plane begins past 2^32 whatever the rows do."""
    import emu_crop_c as ec
    import oracle_c as oc
    hs, vs = MODES[mode]
    npl, h, rb = out_shape(kind, w)
    x, y = 3, 5
    W, H = 64, y + h
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
    full = oracle_rows(kind, W, H, hs, vs, qts, planes).reshape(npl, H, -1)
    bpp = rb // w
    want = full[:, y:y + h, x * bpp:(x + w) * bpp]
    d = ec.desc(W, H, hs, vs, 3, oc.GRAYSCALE if kind == "gray" else oc.RGB, qts, out_layout=1 if kind == "chw" else 0)
    zero_rows = [r - y + p * h for p in range(npl) for r in [q % H for q in uncovered(kind, H, hs, vs)[:len(uncovered(kind, H, hs, vs)) // npl]]]
    pitch = fc.out_pitches(w)[which]
    assert fc.crosses(pitch, h, npl) and ec.crop_out_len(d, w, h, pitch) == npl * h * pitch
    far = far_output(kind, h, rb, pitch)
    rc, _ = ec.decode_crops(d, [planes], [(x, y)], w, h, out_pitch=pitch, outs=[far.buf])
    assert rc == 0
    what = f"crop {mode} {kind} {w}x{h} at ({x},{y}) pitch {pitch}"
    assert_rows(far, want, what)
    if zero_rows:
        check_far_output(far, want, zero_rows, what)
    else:
        assert int(np.count_nonzero(far.buf)) == int(np.count_nonzero(far.rows)), f"{what}: a padding byte was written"


@OUT_PITCH
@pytest.mark.parametrize("sl", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", list(MODES))
def test_reduced_decode(mode, kind, sl, which, synth):
    """whole reduced frames 48 (1/2) and 12 (1/8) wide, a little taller than the output heights"""
    import emu_scaled_c as es
    import scaled_model as sm
    hs, vs = MODES[mode]
    s = 1 << sl
    h = out_shape(kind, 1)[1] + 3
    W, H = 96, h * s
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
    out_cs = sm.GRAYSCALE if kind == "gray" else sm.RGB
    exp = sm.decode_scaled(W, H, hs, vs, 3, out_cs, qts, planes, sl, chw=kind == "chw", clamp_dc=False)
    rw, rh = sm.scaled_size(W, H, sl)
    assert (rw, rh) == (W // s, h)
    npl, rb = (3, rw) if kind == "chw" else (1, rw * (1 if kind == "gray" else 3))
    d = es.desc(W, H, hs, vs, 3, out_cs, qts, out_layout=1 if kind == "chw" else 0)
    pitch = fc.out_pitches(rw)[which]
    assert fc.crosses(pitch, h, npl) and es.out_len(d, sl, rw, rh, pitch) == npl * h * pitch
    far = far_output(kind, h, rb, pitch)
    rc, _ = es.decode(d, [planes], sl, None, out_pitch=pitch, outs=[far.buf])
    assert rc == 0
    what = f"reduced 1/{s} {mode} {kind} {rw}x{rh} pitch {pitch}"
    assert_rows(far, np.asarray(exp).reshape(npl * h, rb), what)
    assert int(np.count_nonzero(far.buf)) == int(np.count_nonzero(far.rows)), f"{what}: a padding byte was written"
