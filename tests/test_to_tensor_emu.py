"""CPU: the u8-images-to-tensor kernel's lanes (zune-jpeg_amd/csrc/zj_to_tensor.h) run one by one over the
launch's grid (tests/emu_to_tensor) against resize_model's conversion at the images' own size.  Three images a call, so that
an odd C * w * h shifts the next image's alignment; the tensor's base 0..7 elements off a 64-byte boundary; the sources 0..3
bytes off a dword, tight and padded by 1 and by 13; channels 1 -> 1, 1 -> 3, 3 -> 3; four dtypes, two layouts, flips mixed
within the call.  For every call: every tensor byte stored exactly once, no store outside the tensor, no load outside an
image's own h rows of w * in_channels bytes, the values equal."""
import numpy as np
import pytest

import emu_to_tensor_c as et
import resize_model as rm

DTYPES = [rm.F32, rm.F16, rm.BF16, rm.U8]
LAYOUTS = ["NCHW", "NHWC"]
CHANNELS = [(1, 1), (1, 3), (3, 3)]
WIDTHS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 255, 256, 257, 258]
HEIGHTS = [1, 2, 3]
PADS = [0, 1, 13]
MEAN, STD = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
GUARD = 64
POISON = 0xAA


def norm(ch):
    return (1 / (255 * STD))[:ch].astype(np.float32), (-MEAN / STD)[:ch].astype(np.float32)


def aligned(n, to=64):
    buf = np.empty(n + to, np.uint8)
    off = (-buf.ctypes.data) % to
    return buf[off:off + n]


def model(img, cout, dtype, layout, scale, bias, flip):
    """img [h, w, cin] u8 -> the image's bytes"""
    h, w, cin = img.shape
    chw = img.transpose(2, 0, 1)
    if cin != cout:
        chw = np.repeat(chw, cout, axis=0)
    return np.ascontiguousarray(rm.resize(chw, w, h, dtype, scale, bias, bool(flip), layout)).view(np.uint8).reshape(-1)


def run_call(rng, n, w, h, cin, cout, dtype, layout, base, misalign, pads, flips):
    """misalign, pads, flips: per image (cycled)"""
    E = et.ELEM[dtype]
    scale, bias = norm(cout)
    s, b = rm.factors(cout, scale, bias)
    s3, b3 = np.ones(3, np.float32), np.zeros(3, np.float32)
    s3[:cout], b3[:cout] = s, b
    # the images side by side in one buffer, each at its own misalignment and pitch, random bytes between them
    offs, pitches, at = [], [], 0
    for i in range(n):
        at = (at + 3) // 4 * 4 + misalign[i % len(misalign)]
        pitch = w * cin + pads[i % len(pads)]
        offs.append(at); pitches.append(pitch)
        at += pitch * (h - 1) + w * cin  # (the next image begins right behind the last row's last byte)
    src = aligned(at + 8)
    src[:] = rng.integers(0, 256, src.size, dtype=np.uint8)
    imgs = [np.lib.stride_tricks.as_strided(src[o:], (h, w, cin), (p, cin, 1)) for o, p in zip(offs, pitches)]
    fl = [flips[i % len(flips)] for i in range(n)]
    ln = cout * w * h * E
    arena = aligned(2 * GUARD + base * E + n * ln)
    arena[:] = POISON
    out_off = GUARD + base * E
    wmap, outside, bad_loads = et.to_tensor([src.ctypes.data + o for o in offs], w, h, pitches, cin, cout, dtype, layout == "NHWC",
                                            s3, b3, fl, arena, out_off)
    what = f"{n} x {w}x{h} {cin}->{cout} dtype {dtype} {layout} base {base} misalign {misalign} pads {pads} flips {flips}"
    assert outside == 0, f"{what}: a store fell outside the arena"
    assert bad_loads == 0, f"{what}: {bad_loads} loads outside their image's rows"
    want = np.zeros(arena.size, np.uint8)
    want[out_off:out_off + n * ln] = 1
    assert np.array_equal(wmap, want), f"{what}: an element not written exactly once, or a byte outside the tensor written"
    assert (arena[:out_off] == POISON).all() and (arena[out_off + n * ln:] == POISON).all()
    for i in range(n):
        exp = model(imgs[i], cout, dtype, layout, scale, bias, fl[i])
        got = arena[out_off + i * ln:out_off + (i + 1) * ln]
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            raise AssertionError(f"{what}: image {i}: {bad.size} bytes differ, first at {bad[:6].tolist()}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_width_alignment_pitch_and_channel_matrix(dtype, layout):
    rng = np.random.default_rng(100 * dtype + len(layout))
    seen = set()
    for (cin, cout) in CHANNELS:
        for w in WIDTHS:
            for base in range(8):
                h = HEIGHTS[(base + w) % 3]
                misalign = [(base + i) % 4 for i in range(3)]
                pads = [PADS[(base // 3 + w + i) % 3] for i in range(3)]
                flips = [(base >> i) & 1 for i in range(3)]
                run_call(rng, 3, w, h, cin, cout, dtype, layout, base, misalign, pads, flips)
                seen.add((w, h))
    assert {w for w, _ in seen} == set(WIDTHS) and {h for _, h in seen} == set(HEIGHTS)


@pytest.mark.parametrize("chans", CHANNELS, ids=["1to1", "1to3", "3to3"])
def test_every_height_misalignment_and_pad_at_the_odd_widths(chans):
    """the full product of heights, source misalignments and pads at widths around a block and a dword, bf16 and f32"""
    rng = np.random.default_rng(7 + chans[1])
    for w in (1, 3, 5, 7, 9, 17, 33):
        for h in HEIGHTS:
            for mis in range(4):
                for pad in PADS:
                    for (dtype, layout) in ((rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NHWC"), (rm.F16, "NCHW")):
                        run_call(rng, 3, w, h, *chans, dtype, layout, (w + mis) % 8, [mis], [pad], [0, 1, 0] if h != 2 else [1, 1, 0])


@pytest.mark.parametrize("chans", CHANNELS, ids=["1to1", "1to3", "3to3"])
def test_129_images_take_two_launches(chans):
    rng = np.random.default_rng(129)
    assert et.batch() == 128
    for (dtype, layout) in ((rm.BF16, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NCHW"), (rm.F16, "NHWC")):
        run_call(rng, 129, 5, 3, *chans, dtype, layout, 3, [0, 1, 2, 3], PADS, [0, 1, 1, 0, 1])


def test_more_than_one_workgroup_per_image():
    rng = np.random.default_rng(3)
    run_call(rng, 2, 258, 40, 3, 3, rm.BF16, "NCHW", 1, [1, 2], [0, 13], [0, 1])
    run_call(rng, 2, 700, 9, 1, 3, rm.F32, "NHWC", 5, [3, 0], [1, 0], [1, 0])


def test_the_block_and_the_kernel_arguments():
    assert et.run() == 8 and et.params_bytes() <= 4096
