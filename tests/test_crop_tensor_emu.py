"""CPU: crop windows decoded straight into a normalised tensor (zj_decode_crops_tensor_device) -- the tensor
kernel's tile decode, staging and converting copy-out and the converted-zero kernel, emulated thread by thread
(tests/emu_crop_tensor), against a numpy model: the emulated u8 crop (emu_crop_c.decode_crops, itself checked against the
sliced full decode by test_crop_emu.py) converted by resize_model's conversion at the window's own size.  The whole tensor
is poisoned first and every element compared for equality (bit patterns for the float types); the guard bytes in front of
image 0 and behind the last must stay untouched (emu_crop_tensor_c)."""
import itertools
import zlib

import numpy as np
import pytest

import emu_crop_c as ec
import emu_crop_tensor_c as ect
import oracle_c as oc
import resize_model as rm

MODES = {"none": (1, 1), "h": (2, 1), "v": (1, 2), "hv": (2, 2)}
KINDS = {"rgb": oc.RGB, "gray": oc.GRAYSCALE, "ycbcr": oc.YCBCR}
DTYPES = [rm.F32, rm.F16, rm.BF16, rm.U8]
LAYOUTS = ["NCHW", "NHWC"]
MEAN, STD = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
ERR_UNSUPPORTED = -2


def norm(ch):
    """ImageNet's scale and bias: every row at or below rows_covered converts to a non-zero bias"""
    return (1 / (255 * STD))[:ch].astype(np.float32), (-MEAN / STD)[:ch].astype(np.float32)


def model(crop, ch, w, h, dtype, layout, scale, bias, flip):
    """one u8 crop (h rows of w * ch bytes) -> the image's bytes"""
    chw = crop.reshape(h, w, ch).transpose(2, 0, 1)
    return np.ascontiguousarray(rm.resize(chw, w, h, dtype, scale, bias, bool(flip), layout)).view(np.uint8).reshape(-1)


def check(d, planes, ch, origins, w, h, dtype, layout, flips, normed=True, what=""):
    scale, bias = norm(ch) if normed else (None, None)
    n = len(origins)
    rc0, crops = ec.decode_crops(d, [planes] * n, origins, w, h)
    rc, buf = ect.decode_crops_tensor(d, [planes] * n, origins, w, h, dtype, layout, scale, bias, flips)
    assert rc == rc0, (what, rc, rc0)
    if rc:
        assert (buf == 0xAA).all(), "a refused call wrote"
        return
    ln = ch * w * h * ect.ELEM[dtype]
    assert buf.size == n * ln
    for f, (xy, crop) in enumerate(zip(origins, crops)):
        exp = model(crop, ch, w, h, dtype, layout, scale, bias, flips[f] if flips is not None else 0)
        got = buf[f * ln:(f + 1) * ln]
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            raise AssertionError(f"{what} {d.width}x{d.height} window {w}x{h} at {xy} dtype {dtype} {layout} flips {flips}: "
                                 f"{bad.size} bytes differ, first at {bad[:6].tolist()}")


COMBOS = list(itertools.product(DTYPES, LAYOUTS, [False, True]))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_tensor_equals_converted_crop(mode, kind, synth):
    """the four modes x {RGB, YCbCr, GRAY} x four dtypes x two layouts x flip off / on, over three frames; 1040 x 72 drops an
    MCU row in the v-subsampled modes, so the converted-zero kernel runs with a non-zero bias"""
    hs, vs = MODES[mode]
    ch = 1 if kind == "gray" else 3
    rng = np.random.default_rng(zlib.crc32(f"{mode}-{kind}".encode()))
    for (W, H) in [(13, 9), (517, 40), (1040, 72)]:
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
        d = ec.desc(W, H, hs, vs, 3, KINDS[kind], qts)
        for (dtype, layout, flip) in COMBOS:
            w, h = int(rng.integers(1, min(W, 48) + 1)), int(rng.integers(1, min(H, 9) + 1))
            origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))), (W - w, H - h), (0, 0)]
            check(d, planes, ch, origins, w, h, dtype, layout, [1, 0, 1] if flip else None, what=f"{mode} {kind}")
    # the whole of the smallest frame
    planes, qts = synth.make_frame(13, 9, hs, vs, 3, seed=22)
    d = ec.desc(13, 9, hs, vs, 3, KINDS[kind], qts)
    for (dtype, layout, flip) in COMBOS:
        check(d, planes, ch, [(0, 0)], 13, 9, dtype, layout, [1] if flip else None, what=f"{mode} {kind} whole")


@pytest.mark.parametrize("mode", ["h", "hv"])
@pytest.mark.parametrize("W", [257, 261, 513])
def test_tail_widths(mode, W, synth):
    """widths whose RGB row end has the hole and the early tail (test_gpu_crop.py: TAIL_WIDTHS), flags 0: windows over the
    row's end and the whole row"""
    hs, vs = MODES[mode]
    H = 8 * vs
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W)
    d = ec.desc(W, H, hs, vs, 3, oc.RGB, qts)
    for (dtype, layout) in [(rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NCHW"), (rm.F16, "NHWC")]:
        for w in (21, 70, W):
            check(d, planes, 3, [(W - w, 0), (W - w, H - 3)], w, 3, dtype, layout, [0, 1], what=f"tail {mode}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_window_widths_and_alignments(dtype, layout, synth):
    """w in 1..9, 15, 16, 17 and 255..258 at odd and even x, straight and mirrored, over a tile column's edge (x = 256 in
    4:2:0) and a strip's (row 32): every destination alignment, every head and tail length of a run"""
    W, H, hs, vs = 517, 40, 2, 2
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=5)
    for kind, ch in (("rgb", 3), ("gray", 1)):
        d = ec.desc(W, H, hs, vs, 3, KINDS[kind], qts)
        for w in list(range(1, 10)) + [15, 16, 17, 255, 256, 257, 258]:
            x0 = 256 - w // 2 if w < 255 else 6
            origins = [(x0, 30), (x0 + 1, 30), (x0, 31), (x0 + 1, 29)]
            check(d, planes, ch, origins, w, 3, dtype, layout, [0, 1, 1, 0], what=f"widths {kind}")


@pytest.mark.parametrize("mode", list(MODES))
def test_corrected_flags(mode, synth):
    hs, vs = MODES[mode]
    W, H = 300, 24
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=77)
    d = ec.desc(W, H, hs, vs, 3, oc.RGB, qts, flags=7)
    check(d, planes, 3, [(0, 0), (W - 33, H - 5), (250, 3)], 33, 5, rm.BF16, "NCHW", [0, 1, 0], what=f"corrected {mode}")
    check(d, planes, 3, [(1, 1), (W - 33, H - 5)], 33, 5, rm.F32, "NHWC", [1, 0], normed=False, what=f"corrected {mode}")


def test_descriptors_without_a_tensor(synth):
    """RGBA and CHW planes have no tensor form; a padded frame pitch is not a crop's"""
    planes, qts = synth.make_frame(64, 16, 2, 2, 3, seed=1)
    for cs, layout in ((oc.RGBA, 0), (oc.RGB, 1)):
        d = ec.desc(64, 16, 2, 2, 3, cs, qts, out_layout=layout)
        assert ect.out_len(d, 8, 8, rm.F32) == 0
        rc, buf = ect.decode_crops_tensor(d, [planes], [(0, 0)], 8, 8, rm.F32)
        assert rc == ERR_UNSUPPORTED
    d = ec.desc(64, 16, 2, 2, 3, oc.RGB, qts)
    assert ect.out_len(d, 8, 8, rm.BF16) == 3 * 8 * 8 * 2 and ect.out_len(d, 8, 8, 4) == 0 and ect.out_len(d, 65, 8, rm.F32) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("flip", [False, True])
def test_span_ends_inside_a_pixel(dtype, layout, flip):
    """the copy-out by itself over spans cut anywhere in the row's bytes -- inside a pixel, a span wholly inside one pixel, an
    empty span -- which the real plans never produce: every element written, and right (the poison is no model value)"""
    rng = np.random.default_rng(zlib.crc32(f"spans-{dtype}-{layout}-{flip}".encode()))
    scale, bias = norm(3)
    for (w, h) in [(1, 1), (2, 3), (7, 2), (37, 5), (256, 3)]:
        rows = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if dtype == rm.U8:
            rows[rows == 0xAA] = 0xAB  # (so that an element left out shows)
        exp = model(rows.reshape(-1), 3, w, h, dtype, layout, scale, bias, flip)
        for cuts in ([], [1], [2], [1, 2], [4, 5], [4, 4, 8], [3 * w - 1], sorted(int(c) for c in rng.integers(0, 3 * w + 1, 6))):
            cuts = [c for c in cuts if c <= 3 * w]
            rc, got = ect.copyout_spans(rows, cuts, dtype, layout, scale, bias, flip)
            assert rc == 0
            if not np.array_equal(got, exp):
                bad = np.nonzero(got != exp)[0]
                raise AssertionError(f"{w}x{h} cuts {cuts}: {bad.size} bytes differ, first at {bad[:6].tolist()}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_mixed_geometry_equals_the_one_geometry_call(kind, synth):
    """the mixed kernel body: frames of different sizes, modes, tables and flags, one record each, one window size; image f is
    the one-geometry call's for frame f alone (itself checked against the model above); a frame the plan refuses in the
    middle gives its status and nothing is written"""
    ch = 1 if kind == "gray" else 3
    rng = np.random.default_rng(zlib.crc32(f"mixed-{kind}".encode()))
    w, h = 11, 7
    geos = [(13, 9, "none", 0), (517, 40, "hv", 0), (1040, 72, "h", 7), (300, 24, "v", 0), (261, 16, "hv", 0), (64, 40, "hv", 7),
            (1040, 72, "hv", 0), (100, 33, "none", 7), (257, 16, "h", 0)]
    descs, frames, origins = [], [], []
    for i, (W, H, mode, flags) in enumerate(geos):
        hs, vs = MODES[mode]
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=100 + i)
        descs.append(ec.desc(W, H, hs, vs, 3, KINDS[kind], qts, flags=flags))
        frames.append(planes)
        origins.append((W - w, H - h) if i % 3 == 0 else (int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))))
    scale, bias = norm(ch)
    # (a geometry that is a reference panic -- a narrow one-component frame -- makes the whole call that status: checked, then left out)
    ok = [ect.decode_crops_tensor(descs[f], [frames[f]], [origins[f]], w, h, rm.U8)[0] for f in range(len(geos))]
    if any(ok):
        rc, buf = ect.decode_crops_tensor_mixed(descs, frames, origins, w, h, rm.BF16, "NCHW", scale, bias)
        assert rc == next(r for r in ok if r) and (buf == 0xAA).all()
    keep = [f for f in range(len(geos)) if ok[f] == 0]
    assert len(keep) >= 7
    geos, descs, frames, origins = ([v[f] for f in keep] for v in (geos, descs, frames, origins))
    flips = [i & 1 for i in range(len(geos))]
    for (dtype, layout) in [(rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NCHW"), (rm.F16, "NHWC")]:
        rc, buf = ect.decode_crops_tensor_mixed(descs, frames, origins, w, h, dtype, layout, scale, bias, flips)
        assert rc == 0
        ln = ch * w * h * ect.ELEM[dtype]
        for f in range(len(geos)):
            rc1, one = ect.decode_crops_tensor(descs[f], [frames[f]], [origins[f]], w, h, dtype, layout, scale, bias, [flips[f]])
            assert rc1 == 0 and np.array_equal(buf[f * ln:(f + 1) * ln], one), (kind, dtype, layout, f)
    # a window that leaves frame 4: the call's status is that frame's, nothing written
    bad = list(origins)
    bad[4] = (geos[4][0] - w + 1, 0)
    rc, buf = ect.decode_crops_tensor_mixed(descs, frames, bad, w, h, rm.BF16, "NCHW", scale, bias, flips)
    assert rc == -1 and (buf == 0xAA).all()
