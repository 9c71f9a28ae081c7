"""CPU: the tone stages' kernels (zune-jpeg_amd/csrc/zj_tone.h) run lane by lane and workgroup by workgroup, phase by phase,
with poisoned LDS (tests/emu_tone) against the definition in numpy (tests/tone_model.py):
- the histogram for widths around the 16-pixel run, heights 1 and 3 and an image one run larger than a workgroup's share, in
  both layouts and for one channel, sources at byte offsets 0..3 from a dword, padded pitches whose padding holds a value the
  images never use -- with a read map that shows every image byte loaded exactly once and nothing else;
- the table build over synthetic histograms: every (lo, hi) pair of autocontrast, the equalize cases with the 65535^2 total;
- the lookup under a random permutation table per image, in place and apart, with a write map that shows every image byte
  stored exactly once and no padding or guard byte, for one image more than a launch takes."""
import numpy as np
import pytest

import emu_tone_c as et
import tone_model as tm
from tone_cases import HEIGHTS, WIDTHS, Arena, permutations, stretches

POISON, PAD = 0xA5, 250
LAYOUTS = pytest.mark.parametrize("channels,chw", [(3, False), (3, True), (1, False)], ids=["HWC", "CHW", "L"])


def test_the_constants_and_the_kernel_arguments():
    assert et.const("run") == 16 and et.const("nt") == 256
    assert et.const("hist_batch") == 128 and et.const("tone_lut_batch") == 256 and et.const("lut_batch") == 128
    assert et.const("hist_params") == 24 * 128 + 8 and et.const("tone_lut_params") == 8 * 256 + 24 and et.const("lut_params") == 28 * 128 + 16
    assert max(et.const(k) for k in ("hist_params", "tone_lut_params", "lut_params")) <= 4096
    for op in range(-2, 8):
        for param in range(-2, 260):
            assert et.op_valid(op, param) == tm.valid(op, param), (op, param)


@LAYOUTS
def test_histogram_equals_the_model_and_reads_each_byte_once(channels, chw):
    share = et.const("nt") * et.const("hist_runs")                    # runs of one workgroup
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(16 * (share + 1), 1), (16 * (share // 3 + 1), 3), (16 * share, 1)]
    ar = Arena(sizes, channels, chw, np.random.default_rng(3 + channels + chw), PAD, 0, 200)
    assert {o % 4 for o in ar.off} == {0, 1, 2, 3} and any(p > w * ar.bpp for p, (w, _) in zip(ar.pitch, sizes))
    got, rmap, outside = et.hist(ar.buf, ar.off, sizes, ar.pitch, channels, chw)
    assert outside == 0
    assert np.array_equal(rmap, ar.inside.astype(np.uint8)), "an image byte not loaded exactly once, or a byte outside the rows loaded"
    for i in range(len(sizes)):
        assert np.array_equal(got[i], tm.histogram(ar.image(i), chw)), (i, sizes[i])
    assert got[:, :, 200:].sum() == 0, "padding was counted"


@LAYOUTS
def test_histogram_of_stretches_of_equal_neighbours(channels, chw):
    """rows made of stretches of one value, 1 to 40 pixels long, and flat images: a stretch is one add of its length"""
    rng = np.random.default_rng(31 + channels + chw)
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(300, 7), (4097, 2)]
    ar = stretches(rng, Arena(sizes, channels, chw, rng, PAD, 0, 200))
    flat = Arena([(16, 1), (33, 3), (700, 5)], channels, chw, rng, PAD, 77, 78)
    for a in (ar, flat):
        got, rmap, outside = et.hist(a.buf, a.off, a.sizes, a.pitch, channels, chw)
        assert outside == 0 and np.array_equal(rmap, a.inside.astype(np.uint8))
        for i in range(len(a.sizes)):
            assert np.array_equal(got[i], tm.histogram(a.image(i), chw)), (i, a.sizes[i])
    assert got[2].sum() == 700 * 5 * channels and got[2][:, 77].sum() == got[2].sum()


def test_histogram_of_one_image_more_than_a_launch_takes():
    rng = np.random.default_rng(9)
    n = et.const("hist_batch") + 1
    sizes = [(int(rng.integers(1, 70)), int(rng.integers(1, 6))) for _ in range(n)]
    ar = Arena(sizes, 3, False, rng, PAD, 0, 200)
    got, rmap, outside = et.hist(ar.buf, ar.off, sizes, ar.pitch, 3, False)
    assert outside == 0 and np.array_equal(rmap, ar.inside.astype(np.uint8))
    for i in range(n):
        assert np.array_equal(got[i], tm.histogram(ar.image(i))), i


def test_every_lo_hi_pair_of_autocontrast():
    pairs = tm.autocontrast_pairs()
    hist = np.zeros((len(pairs), 1, 256), np.uint32)
    for k, (lo, hi) in enumerate(pairs):
        hist[k, 0, lo], hist[k, 0, hi] = 3, 5
    got = et.luts([(tm.AUTOCONTRAST, 0)] * len(pairs), 1, hist)
    bad = [(lo, hi) for k, (lo, hi) in enumerate(pairs) if not np.array_equal(got[k, 0], tm.autocontrast_table(hist[k, 0]))]
    assert not bad, (len(bad), bad[:5])
    # lo == hi and no bin at all: the identity
    one = np.zeros((2, 1, 256), np.uint32)
    one[0, 0, 99] = 7
    got = et.luts([(tm.AUTOCONTRAST, 0)] * 2, 1, one)
    assert np.array_equal(got[0, 0], np.arange(256)) and np.array_equal(got[1, 0], np.arange(256))


def test_the_equalize_cases_and_the_64_bit_sum():
    cases = tm.equalize_cases()
    names = sorted(cases)
    hist = np.array([[cases[names[(k + c) % len(names)]] for c in range(3)] for k in range(len(names))], np.uint64)
    for op in (tm.EQUALIZE, tm.AUTOCONTRAST):
        got = et.luts([(op, 0)] * len(names), 3, hist)
        for k, name in enumerate(names):
            for c in range(3):
                other = names[(k + c) % len(names)]
                assert np.array_equal(got[k, c], tm.table(op, 0, cases[other])), (op, name, c, other)
    rng = np.random.default_rng(8)
    for _ in range(40):   # random bins of every density
        h = rng.integers(0, 1 << int(rng.integers(1, 32)), 256) * (rng.random(256) < rng.random())
        got = et.luts([(tm.EQUALIZE, 0)], 1, h.reshape(1, 1, 256))
        assert np.array_equal(got[0, 0], tm.table(tm.EQUALIZE, 0, h))


def test_the_ops_without_a_histogram_and_the_refusals():
    ops = [(tm.IDENTITY, 0), (tm.INVERT, 0)] + [(tm.POSTERIZE, b) for b in range(1, 9)] + [(tm.SOLARIZE, t) for t in (0, 1, 128, 255, 256)]
    ops = ops * 18   # (a second launch)
    for channels in (1, 3):
        got = et.luts(ops, channels, None)
        for k, (op, param) in enumerate(ops):
            assert np.array_equal(got[k], tm.tables(op, param, None, channels)), (k, op, param)
    assert et.luts([(tm.INVERT, 0), (tm.EQUALIZE, 0)], 1, None) is None
    assert et.luts([(tm.POSTERIZE, 9)], 1, None) is None and et.luts([(6, 0)], 1, None) is None


def lookup(sizes, channels, chw, in_place, seed):
    rng = np.random.default_rng(seed)
    src = Arena(sizes, channels, chw, rng, POISON)
    dst = src if in_place else Arena(sizes, channels, chw, rng, POISON, pads=(13, 0, 1, 5), data=False)
    tables = permutations(rng, len(sizes), channels)
    before = src.buf.copy()
    arena = src.buf if in_place else dst.buf
    rmap, wmap, outside = et.lut(src.buf, src.off, sizes, src.pitch, channels, chw, tables, arena, dst.off, dst.pitch)
    assert outside == 0, "a load or a store fell outside its buffer"
    assert np.array_equal(wmap, dst.inside.astype(np.uint8)), "an image byte not stored exactly once, or a padding byte stored"
    assert np.array_equal(rmap, src.inside.astype(np.uint8)), "an image byte not loaded exactly once, or a byte outside the rows loaded"
    assert (arena[~dst.inside] == POISON).all()
    outs = []
    for i in range(len(sizes)):
        a = Arena.image(src, i, before)
        want = tm.apply_luts(a, tables[i], chw)
        assert np.array_equal(dst.image(i, arena), want), (i, sizes[i])
        outs.append(want)
    if not in_place:
        assert np.array_equal(src.buf, before), "an input was written"
    return outs


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
@LAYOUTS
def test_lookup_under_permutation_tables(channels, chw, in_place):
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(300, 20), (4097, 1)]
    lookup(sizes, channels, chw, in_place, 21 + channels + 2 * chw)


@LAYOUTS
def test_in_place_equals_apart(channels, chw):
    sizes = [(1, 1), (16, 2), (17, 3), (33, 2), (48, 1), (49, 3), (130, 2), (5, 3), (31, 1), (32, 3), (47, 2), (64, 1)]
    a = lookup(sizes, channels, chw, False, 77)
    b = lookup(sizes, channels, chw, True, 77)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in_place"])
def test_lookup_of_one_image_more_than_a_launch_takes(in_place):
    rng = np.random.default_rng(87)
    n = et.const("lut_batch") + 1
    sizes = [(int(rng.integers(1, 70)), int(rng.integers(1, 6))) for _ in range(n)]
    lookup(sizes, 3, False, in_place, 88)


def test_the_whole_op_through_the_three_kernels_equals_the_model():
    """histogram -> tables -> lookup, as zj_tone_device chains them, for every op"""
    rng = np.random.default_rng(12)
    ops = [(tm.IDENTITY, 0), (tm.INVERT, 0), (tm.POSTERIZE, 3), (tm.SOLARIZE, 100), (tm.AUTOCONTRAST, 0), (tm.EQUALIZE, 0)]
    for channels, chw in ((3, False), (3, True), (1, False)):
        sizes = [(37, 3), (130, 5), (61, 40)] * 2
        src = Arena(sizes, channels, chw, rng, POISON, 30, 220)
        bins, _, outside = et.hist(src.buf, src.off, sizes, src.pitch, channels, chw)
        tables = et.luts(ops, channels, bins)
        before = src.buf.copy()
        _, _, out2 = et.lut(src.buf, src.off, sizes, src.pitch, channels, chw, tables, src.buf, src.off, src.pitch)
        assert outside == 0 and out2 == 0
        for i, (op, param) in enumerate(ops):
            assert np.array_equal(src.image(i, src.buf), tm.apply(op, param, Arena.image(src, i, before), chw)), (i, op)
