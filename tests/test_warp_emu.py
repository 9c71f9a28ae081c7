"""CPU: the affine-warp kernels' lanes (zune-jpeg_amd/csrc/zj_warp.h) run one by one over the launch's
grid (tests/emu_warp) against warp_model.  Three images a call, each of its own size, misalignment and pitch, so that an odd
C * out_w * out_h shifts the next image's alignment; the tensor's base 0..7 elements off a 64-byte boundary.  For every call:
every tensor byte stored exactly once, no store outside the tensor, no load outside an image's own h rows of w * C bytes,
the values equal the model's bits."""
import math

import numpy as np
import pytest

import emu_warp_c as ew
import resize_model as rm
import warp_model as wm

DTYPES = [rm.F32, rm.F16, rm.BF16, rm.U8]
LAYOUTS = ["NCHW", "NHWC"]
SOURCES = [(1, 1), (2, 1), (7, 5), (53, 37), (258, 3)]
WIDTHS = list(range(1, 10)) + [15, 16, 17, 63, 64, 65]
HEIGHTS = [1, 2, 3]
PADS = [0, 1, 13]
FILLS = [(0, 0, 0), (7, 130, 255)]
MEAN, STD = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
GUARD = 64
POISON = 0xAA


def norm(ch):
    return (1 / (255 * STD))[:ch].astype(np.float32), (-MEAN / STD)[:ch].astype(np.float32)


def aligned(n, to=64):
    buf = np.empty(n + to, np.uint8)
    off = (-buf.ctypes.data) % to
    return buf[off:off + n]


def matrices(w, h, ow, oh):
    """the issue's matrices for a w x h source and an ow x oh output, as doubles"""
    ms = [wm.orientation_matrix(o, w, h) for o in range(1, 9)]
    cx, cy, ox, oy = w / 2, h / 2, ow / 2, oh / 2
    co, si = math.cos(math.radians(17)), math.sin(math.radians(17))
    sx, sy = min(w / ow, 100.0), min(h / oh, 100.0)  # (an entry of 128 or more is refused)
    ms.append((co * sx, -si * sy, cx - co * sx * ox + si * sy * oy, si * sx, co * sy, cy - si * sx * ox - co * sy * oy))  # 17 degrees
    ms.append((sx, 0.3 * sx, -0.3 * sx * oy, 0.0, sy, 0.0))            # shear
    ms.append((3.7, 0.0, 0.0, 0.0, 3.7, 0.0))                            # x 3.7 downscale
    ms.append((1.0, 0.0, float(w + 5), 0.0, 1.0, 0.0))                   # wholly outside
    ms.append((1.0, 0.0, -ow / 2 - 0.25, 0.0, 1.0, -oh / 2 + 0.375))     # half outside
    return ms


def run_call(rng, sources, ms, ch, ow, oh, dtype, layout, base, misalign, pads, edge, fill):
    """sources, ms, misalign, pads: per image (the last three cycled)"""
    n = len(sources)
    E = ew.ELEM[dtype]
    scale, bias = norm(ch)
    s, b = rm.factors(ch, scale, bias)
    s3, b3 = np.ones(3, np.float32), np.zeros(3, np.float32)
    s3[:ch], b3[:ch] = s, b
    offs, pitches, at = [], [], 0
    for i, (w, h) in enumerate(sources):
        at = (at + 3) // 4 * 4 + misalign[i % len(misalign)]
        pitch = w * ch + pads[i % len(pads)]
        offs.append(at); pitches.append(pitch)
        at += pitch * (h - 1) + w * ch  # (the next image begins right behind the last row's last byte)
    src = aligned(at + 8)
    src[:] = rng.integers(0, 256, src.size, dtype=np.uint8)
    imgs = [np.lib.stride_tricks.as_strided(src[o:], (h, w, ch), (p, ch, 1)) for o, p, (w, h) in zip(offs, pitches, sources)]
    ints = [wm.fixed(ms[i % len(ms)]) for i in range(n)]
    assert all(q is not None for q in ints)
    ln = ch * ow * oh * E
    arena = aligned(2 * GUARD + base * E + n * ln)
    arena[:] = POISON
    out_off = GUARD + base * E
    wmap, outside, bad_loads, loads = ew.warp([src.ctypes.data + o for o in offs], sources, pitches, ch, ints, ow, oh, dtype,
                                              layout == "NHWC", s3, b3, fill, edge, arena, out_off)
    what = f"{n} x {sources[:3]} C {ch} -> {ow}x{oh} dtype {dtype} {layout} base {base} misalign {misalign} pads {pads} edge {edge}"
    assert outside == 0, f"{what}: a store fell outside the arena, or was not aligned to its size"
    assert bad_loads == 0, f"{what}: {bad_loads} loads outside their image's rows"
    want = np.zeros(arena.size, np.uint8)
    want[out_off:out_off + n * ln] = 1
    assert np.array_equal(wmap, want), f"{what}: an element not written exactly once, or a byte outside the tensor written"
    assert (arena[:out_off] == POISON).all() and (arena[out_off + n * ln:] == POISON).all()
    for i in range(n):
        exp = np.ascontiguousarray(wm.warp(imgs[i], ints[i], ow, oh, dtype, scale, bias, edge, fill, layout)).view(np.uint8).reshape(-1)
        got = arena[out_off + i * ln:out_off + (i + 1) * ln]
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            raise AssertionError(f"{what}: image {i} matrix {ms[i % len(ms)]}: {bad.size} bytes differ, first at {bad[:6].tolist()}")
    return loads


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_width_alignment_pitch_and_channel_matrix(dtype, layout):
    rng = np.random.default_rng(100 * dtype + len(layout))
    seen_w, seen_h, seen_src = set(), set(), set()
    for ch in (1, 3):
        for wi, ow in enumerate(WIDTHS):
            for base in range(8):
                oh = HEIGHTS[(base + ow) % 3]
                sources = [SOURCES[(wi + base + i) % len(SOURCES)] for i in range(3)]
                all_ms = matrices(*sources[0], ow, oh)
                ms = [all_ms[(3 * (wi + base) + i) % len(all_ms)] for i in range(3)]
                misalign = [(base + i) % 4 for i in range(3)]
                pads = [PADS[(base // 3 + ow + i) % 3] for i in range(3)]
                run_call(rng, sources, ms, ch, ow, oh, dtype, layout, base, misalign, pads, (base + wi) & 1, FILLS[(base >> 1) & 1])
                seen_w.add(ow); seen_h.add(oh); seen_src.update(sources)
    assert seen_w == set(WIDTHS) and seen_h == set(HEIGHTS) and seen_src == set(SOURCES)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("edge", [wm.FILL, wm.REPLICATE])
def test_every_matrix_on_every_source(ch, edge):
    """each of the issue's matrices, built for the source it is applied to, in both edge modes and both fills"""
    rng = np.random.default_rng(17 + ch + 2 * edge)
    combos = [(rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NHWC"), (rm.F16, "NCHW")]
    k = 0
    for (w, h) in SOURCES:
        for (ow, oh) in ((9, 3), (17, 2), (5, 7)):
            for m in matrices(w, h, ow, oh):
                dtype, layout = combos[k % 4]
                run_call(rng, [(w, h)], [m], ch, ow, oh, dtype, layout, k % 8, [k % 4], [PADS[k % 3]], edge, FILLS[(k // 2) % 2])
                k += 1


def test_a_wholly_outside_output_loads_nothing():
    rng = np.random.default_rng(5)
    m = (1.0, 0.0, 60.0, 0.0, 1.0, 0.0)
    assert run_call(rng, [(53, 37)], [m], 3, 17, 9, rm.BF16, "NCHW", 1, [1], [13], wm.FILL, FILLS[1]) == 0
    assert run_call(rng, [(53, 37)], [m], 3, 17, 9, rm.BF16, "NCHW", 1, [1], [13], wm.REPLICATE, FILLS[1]) > 0


@pytest.mark.parametrize("ch", [1, 3])
def test_more_images_than_one_launch_holds(ch):
    rng = np.random.default_rng(49)
    n = ew.batch() + 1
    assert n == 49
    sources = [SOURCES[i % len(SOURCES)] for i in range(n)]
    ms = matrices(7, 5, 5, 3)
    for (dtype, layout) in ((rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NCHW"), (rm.F16, "NHWC")):
        run_call(rng, sources, ms, ch, 5, 3, dtype, layout, 3, [0, 1, 2, 3], PADS, wm.FILL, FILLS[1])


def test_more_than_one_block_each_way():
    """rows across a block's edge and more than 64 pixels a row: several workgroups per image"""
    rng = np.random.default_rng(3)
    rows = ew.block_rows()
    for (ch, dtype, layout, edge) in ((3, rm.BF16, "NCHW", wm.FILL), (1, rm.F32, "NHWC", wm.REPLICATE), (3, rm.U8, "NHWC", wm.FILL)):
        for oh in (rows - 1, rows, rows + 1):
            ms = matrices(53, 37, 131, oh)
            run_call(rng, [(53, 37), (258, 3)], [ms[8], ms[5]], ch, 131, oh, dtype, layout, 5, [3, 0], [1, 0], edge, FILLS[1])


def test_the_group_the_block_and_the_kernel_arguments():
    assert ew.group() == 8 and ew.block_rows() == 32 and ew.params_bytes() <= 4096
