"""CPU: the colour-matrix kernel's lanes (zune-jpeg_amd/csrc/zj_color.h) run one by one over the launch's grid
(tests/emu_color) against the definition in numpy (tests/color_model.py): widths around the 16-pixel run and its multiples,
tight and padded pitches, images at every offset from a 16-byte boundary, both layouts, in place and out of place, five
matrices (identity, BGR, saturation 0, a jitter that clamps at both ends, the negative) -- with a write map that shows every
byte of every image written exactly once and no padding or guard byte written, and a read map that shows no byte outside an
image's rows loaded."""
import importlib

import numpy as np
import pytest

import color_cases as cc
import color_model as cm
import emu_color_c as ce


def aligned(n):
    """n bytes that start on a 16-byte boundary"""
    buf = np.empty(n + 16, np.uint8)
    off = (-buf.ctypes.data) % 16
    return buf[off:off + n]


def run_call(rng, cases, chw, in_place, first=0, matrices=cc.MATRICES):
    """one call over `cases`; returns the output arena"""
    lay = cc.Layout(rng, cases, chw, in_place, first, matrices)
    arena = aligned(lay.arena_len)
    arena[:] = lay.arena0
    if in_place:
        src = arena
    else:
        src = aligned(lay.src.size)
        src[:] = lay.src
    rmap, wmap, outside = ce.color(src, lay.in_off, lay.sizes, lay.in_pitch, chw, lay.q, arena, lay.out_off, lay.out_pitch)
    assert outside == 0, "a load or a store fell outside its buffer"
    assert np.array_equal(wmap, lay.inside.astype(np.uint8)), "an image byte not written exactly once, or a padding byte written"
    assert np.array_equal(rmap, lay.src_inside.astype(np.uint8)), "an image byte not read exactly once, or a byte outside the rows read"
    assert np.array_equal(arena, lay.want)
    if not in_place:
        assert np.array_equal(src, lay.src), "an input was written"
    return lay, arena


def images_of(lay, arena):
    bpp, npl = (1, 3) if lay.chw else (3, 1)
    return [arena[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp].copy()
            for (w, h), oo, op in zip(lay.sizes, lay.out_off, lay.out_pitch)]


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_the_size_pitch_and_alignment_matrix_in_place_and_apart(chw):
    cases = cc.matrix()
    assert len(cases) == 23 * 3 * 3 * 16
    B = ce.batch()
    rng = np.random.default_rng(41 + chw)
    for k in range(0, len(cases), B):
        for in_place in (False, True):
            run_call(rng, cases[k:k + B], chw, in_place, first=k)


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_in_place_equals_out_of_place_on_the_same_images(chw, in_place):
    """the same 12 images under the same matrices, once apart and once in place: the same output bytes"""
    rng = np.random.default_rng(3)
    sizes = [(1, 1), (16, 2), (17, 3), (33, 2), (48, 1), (49, 3), (130, 2), (5, 3), (31, 1), (32, 3), (47, 2), (64, 1)]
    bpp, npl = (1, 3) if chw else (3, 1)
    data = [rng.integers(0, 256, (npl, h, w * bpp), dtype=np.uint8) for w, h in sizes]
    outs = []
    for inp in (False, True):
        lay = cc.Layout(np.random.default_rng(4), [(w, h, 1, 13, 3, 5) for w, h in sizes], chw, inp)
        arena = aligned(lay.arena_len)
        arena[:] = cc.SENTINEL
        src = arena if inp else aligned(lay.src.size)
        for a, (w, h), io, ip in zip(data, sizes, lay.in_off, lay.in_pitch):
            src[io:io + ip * h * npl].reshape(npl, h, ip)[:, :, :w * bpp] = a
        _, wmap, outside = ce.color(src, lay.in_off, lay.sizes, lay.in_pitch, chw, lay.q, arena, lay.out_off, lay.out_pitch)
        assert outside == 0 and np.array_equal(wmap, lay.inside.astype(np.uint8))
        outs.append(images_of(lay, arena))
        for a, got, q in zip(data, outs[-1], lay.q):
            img = a if chw else a.reshape(a.shape[1], -1, 3)
            assert np.array_equal(got.reshape(img.shape), cm.apply_fixed(q, img, chw))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_49_images_of_different_sizes_take_a_second_launch(chw, in_place):
    rng = np.random.default_rng(87 + chw)
    assert ce.batch() == 48
    run_call(rng, cc.mixed_49(rng), chw, in_place)


def test_the_run_and_the_kernel_arguments():
    assert ce.run() == 16 and ce.params_bytes() == 76 * 48 + 8 <= 4096


def test_a_tall_and_a_wide_image_share_a_launch():
    """the grid is the image's with the most runs: 1 x 700 beside 700 x 1 beside 257 x 33 (more than one workgroup each)"""
    rng = np.random.default_rng(6)
    for chw in (False, True):
        run_call(rng, [(1, 700, 0, 0, 0, 0), (700, 1, 0, 13, 3, 1), (257, 33, 1, 1, 5, 3), (16, 16, 0, 0, 0, 0)], chw, False)


def test_every_byte_value_under_every_matrix():
    """one 256-pixel row per matrix with every byte value in every channel, and rows where one channel is 0 or 255: the
    24-bit products and the clamp equal the definition"""
    v = np.arange(256, dtype=np.uint8)
    rows = [np.stack([v, v[::-1], np.roll(v, 77)], -1), np.stack([v, np.zeros_like(v), np.full_like(v, 255)], -1),
            np.stack([np.full_like(v, 255), v, v], -1), np.stack([np.zeros_like(v), np.zeros_like(v), v], -1)]
    img = np.stack(rows)                                    # [4, 256, 3]
    for m in list(cc.MATRICES) + list(cc.EXTREMES):
        q = ce.fixed(m)
        assert q == cm.fixed(m)
        src = aligned(img.size)
        src[:] = img.reshape(-1)
        arena = aligned(img.size + 128)
        arena[:] = cc.SENTINEL
        _, wmap, outside = ce.color(src, [0], [(256, 4)], [768], False, [q], arena, [64], [768])
        assert outside == 0 and wmap[64:64 + img.size].min() == 1 == wmap.max() and wmap[:64].max() == 0 == wmap[-64:].max()
        assert np.array_equal(arena[64:64 + img.size].reshape(img.shape), cm.apply_fixed(q, img))


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_the_extreme_matrices_over_the_widths_the_gpu_test_runs(chw, in_place):
    """test_gpu_color.py's layout of color_cases.EXTREMES, lane by lane: both ends of the clamp are reached"""
    cases = [(w, 3, 1, 13, (3 * i + k) % 16, (5 * i + 7 * k) % 16) for i, w in enumerate(cc.EXTREME_WIDTHS) for k in range(3)]
    lay, arena = run_call(np.random.default_rng(112 + chw + 2 * in_place), cases, chw, in_place, matrices=cc.EXTREMES)
    out = arena[lay.inside]
    assert (out == 0).any() and (out == 255).any() and ((out > 0) & (out < 255)).any()


def test_the_host_rule_equals_the_model_and_the_package():
    rng = np.random.default_rng(2)
    for _ in range(200):
        m = rng.uniform(-1, 1, 12) * rng.choice([0.01, 1.0, 16.0, 17.0]) * np.tile([1, 1, 1, 256.0], 3)
        assert ce.fixed(m) == cm.fixed(m)
    assert ce.fixed([float("nan")] + [0.0] * 11) is None and ce.fixed([0.0] * 11 + [float("inf")]) is None
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    assert np.allclose(cc.jitter(), tensors.color_matrix(1.8, 1.6, 2.0, 0.2), atol=1e-12)
    img = cm.noise_image()
    got = cm.apply(cc.jitter(), img)
    assert (got == 0).any() and (got == 255).any()          # it clamps at both ends
