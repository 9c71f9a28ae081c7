"""CPU: the CMYK-to-RGB kernel's lanes (zune-jpeg_amd/csrc/zj_cmyk.h) run one by one over the launch's grid (tests/emu_cmyk)
against (a * k + 127) // 255 in numpy and against Pillow's CMYK -> RGB: widths around the 16-pixel run and its multiples, tight
and padded pitches, images at and off 16-byte boundaries, both layouts, in place and out of place, both values of `inverted`
-- and a write map that shows every byte of every image written exactly once, no padding byte written, and no store outside
the arena."""
import numpy as np
import pytest

import cmyk_stage_cases as sc
import emu_cmyk_c as ck


def aligned(n):
    """n bytes that start on a 16-byte boundary"""
    buf = np.empty(n + 16, np.uint8)
    off = (-buf.ctypes.data) % 16
    return buf[off:off + n]


def run_call(rng, cases, chw, in_place):
    lay = sc.Layout(rng, cases, chw, in_place)
    src = aligned(lay.src.size)
    src[:] = lay.src
    arena = aligned(lay.arena_len)
    arena[:] = lay.arena0
    a_addrs = [(arena if in_place else src).ctypes.data + o for o in lay.a_off]
    wmap, outside = ck.combine(a_addrs, [src.ctypes.data + o for o in lay.k_off], lay.sizes, lay.a_pitch, lay.k_pitch, chw,
                               lay.inverted, arena, lay.out_off, lay.out_pitch)
    assert outside == 0, "a store fell outside the arena"
    assert np.array_equal(wmap, lay.inside.astype(np.uint8)), "an image byte not written exactly once, or a padding byte written"
    assert np.array_equal(arena, lay.want)
    assert np.array_equal(src, lay.src), "an input was written"


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_the_size_pitch_and_alignment_matrix(chw, in_place):
    rng = np.random.default_rng(41 + chw + 2 * in_place)
    cases = sc.matrix()
    assert len(cases) == 12 * 4 * 2 * 4 * 3
    B = ck.batch()
    for k in range(0, len(cases), B):
        run_call(rng, cases[k:k + B], chw, in_place)


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_129_images_of_mixed_sizes_take_a_second_launch(chw, in_place):
    rng = np.random.default_rng(87 + chw)
    assert ck.batch() < 129
    run_call(rng, sc.mixed_129(rng), chw, in_place)


def test_the_run_and_the_kernel_arguments():
    assert ck.run() == 16 and ck.params_bytes() <= 4096


def test_a_tall_and_a_wide_image_share_a_launch():
    """the grid is the image's with the most runs: 1 x 700 beside 700 x 1 beside 257 x 33 (more than one workgroup each)"""
    rng = np.random.default_rng(6)
    for chw in (False, True):
        run_call(rng, [(1, 700, 0, 0, 0), (700, 1, 0, 3, 1), (257, 33, 5, 1, 3), (16, 16, 0, 0, 0)], chw, False)


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_every_pair_of_bytes_against_the_formula_and_pillow(chw):
    """one 256 x 256 image pair that holds every (a, k): the kernel's packed arithmetic equals (a * k + 127) // 255 on all
    65 536 pairs, and that is Pillow's CMYK -> RGB on its (complemented) samples"""
    from PIL import Image
    kv, av = np.mgrid[0:256, 0:256].astype(np.uint8)        # k = the row, a = the column
    a3 = np.stack([av, av[:, ::-1], av], axis=0 if chw else 2)
    for inverted in (0, 1):
        src = aligned(4 * 65536)
        src[:65536] = kv.reshape(-1)
        src[65536:] = a3.reshape(-1)
        arena = aligned(3 * 65536 + 128)
        arena[:] = sc.SENTINEL
        wmap, outside = ck.combine([src.ctypes.data + 65536], [src.ctypes.data], [(256, 256)], [256 if chw else 768], [256], chw,
                                   [inverted], arena, [64], [256 if chw else 768])
        assert outside == 0 and wmap[64:64 + 3 * 65536].min() == 1 == wmap.max() and wmap[:64].max() == 0 == wmap[-64:].max()
        got = arena[64:64 + 3 * 65536].reshape(a3.shape)
        k3 = kv[None] if chw else kv[:, :, None]
        assert np.array_equal(got, sc.combine(a3, k3, inverted))
        # Pillow takes CMYK samples "ink": 0 = none.  inverted (an Adobe file's stored samples are 255 - ink): ink = 255 - x
        hwc = (lambda x: np.ascontiguousarray(x.transpose(1, 2, 0))) if chw else (lambda x: x)
        ink = np.concatenate([hwc(a3), kv[:, :, None]], axis=2)
        if inverted:
            ink = 255 - ink
        pil = np.asarray(Image.fromarray(np.ascontiguousarray(ink), "CMYK").convert("RGB"))
        assert np.array_equal(hwc(got), pil)
