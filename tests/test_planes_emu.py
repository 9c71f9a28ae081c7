"""CPU: the planes-to-RGB kernel's lanes (zune-jpeg_amd/csrc/zj_planes.h) run one by one over the launch's grid
(tests/emu_planes) against box replication and the oracle's colour arithmetic in numpy: widths around the 16-pixel run and its
multiples, every ratio pair and phase per component, tight and padded pitches, planes and images at and off 4- and 16-byte
boundaries, both layouts, both colour modes -- with a write map that shows every byte of every image written exactly once, no
padding byte written, no store outside the arena, and a read map that shows no byte read but the samples an image shows."""
import numpy as np
import pytest

import emu_planes_c as pk
import oracle_np as onp
import planes_cases as pc


def aligned(n):
    """n bytes that start on a 16-byte boundary"""
    buf = np.empty(n + 16, np.uint8)
    off = (-buf.ctypes.data) % 16
    return buf[off:off + n]


def run_call(rng, cases, chw, stored_rgb):
    lay = pc.Layout(rng, cases, chw, stored_rgb)
    src = aligned(lay.src.size)
    src[:] = lay.src
    arena = aligned(lay.arena_len)
    arena[:] = pc.SENTINEL
    wmap, outside, bad_reads = pk.combine(src, lay.needed, lay.p_off, lay.p_pitch, lay.sizes, lay.geos, stored_rgb, chw, arena,
                                          lay.out_off, lay.out_pitch)
    assert outside == 0, "a store fell outside the arena"
    assert bad_reads == 0, "a byte was read that is no sample the image shows"
    assert np.array_equal(wmap, lay.inside.astype(np.uint8)), "an image byte not written exactly once, or a padding byte written"
    assert np.array_equal(arena, lay.want)
    assert np.array_equal(src, lay.src), "an input was written"


@pytest.mark.parametrize("stored_rgb", [False, True], ids=["ycbcr", "stored_rgb"])
@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_the_size_pitch_alignment_ratio_and_phase_matrix(chw, stored_rgb):
    rng = np.random.default_rng(43 + chw + 2 * stored_rgb)
    cases = pc.matrix()
    assert len(cases) == 12 * 4 * 2 * 4 * 3
    # every width meets every (rx, px) and every height every (ry, py), in every component
    for c in range(3):
        assert {(k[0], k[5][c][0], k[5][c][2]) for k in cases} == {(w, rx, px) for w in pc.ec.WIDTHS for rx in (1, 2, 4) for px in range(rx)}
        assert {(k[1], k[5][c][1], k[5][c][3]) for k in cases} == {(h, ry, py) for h in pc.ec.HEIGHTS for ry in (1, 2, 4) for py in range(ry)}
    step = 2 * pk.batch() + 5  # (calls of three launches, the last one short)
    for k in range(0, len(cases), step):
        run_call(rng, cases[k:k + step], chw, stored_rgb)


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_129_images_of_mixed_sizes_take_a_second_launch(chw):
    rng = np.random.default_rng(89 + chw)
    assert pk.batch() < 129
    run_call(rng, pc.mixed_129(rng), chw, False)


def test_the_run_and_the_kernel_arguments():
    assert pk.run() == 16 and pk.params_bytes() <= 4096


def test_a_tall_and_a_wide_image_share_a_launch():
    """the grid is the image's with the most runs: 1 x 700 beside 700 x 1 beside 257 x 33 (more than one workgroup each)"""
    rng = np.random.default_rng(7)
    cases = pc.with_geos([(1, 700, 0, 0, 0), (700, 1, 0, 3, 1), (257, 33, 5, 1, 3), (16, 16, 0, 0, 0)], start=17)
    for chw in (False, True):
        run_call(rng, cases, chw, False)


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
def test_every_triple_of_bytes_against_the_oracle(chw):
    """all 2^24 (y, cb, cr): 64 images of 256 x 1024 -- four values of y each, cb and cr the position -- at ratio 1: the
    packed 16-bit arithmetic equals ycbcr_to_rgb_px everywhere"""
    cbv, crv = np.mgrid[0:256, 0:256].astype(np.uint8)
    bpp, npl = (1, 3) if chw else (3, 1)
    geo = ((1, 1, 0, 0),) * 3
    for y0 in range(0, 256, 4):
        src = aligned(3 * 4 * 65536)
        ys = np.repeat(np.arange(y0, y0 + 4, dtype=np.uint8), 65536)
        src[:4 * 65536] = ys
        src[4 * 65536:8 * 65536] = np.tile(cbv.reshape(-1), 4)
        src[8 * 65536:] = np.tile(crv.reshape(-1), 4)
        arena = aligned(3 * 4 * 65536 + 128)
        arena[:] = pc.SENTINEL
        wmap, outside, bad = pk.combine(src, np.ones(src.size, np.uint8), [(0, 4 * 65536, 8 * 65536)], [(256, 256, 256)],
                                        [(256, 1024)], [geo], False, chw, arena, [64], [256 * bpp])
        assert outside == 0 and bad == 0
        assert wmap[64:-64].min() == 1 == wmap.max() and wmap[:64].max() == 0 == wmap[-64:].max()
        want = onp.ycbcr_to_rgb_px(ys.astype(np.int16), src[4 * 65536:8 * 65536].astype(np.int16), src[8 * 65536:].astype(np.int16))
        got = arena[64:-64].reshape(npl, 1024, 256 * bpp)
        got = got.transpose(1, 2, 0).reshape(-1, 3) if chw else got.reshape(-1, 3)
        assert np.array_equal(got, want), y0
