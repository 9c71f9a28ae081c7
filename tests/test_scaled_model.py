"""CPU: the definition of the reduced-size decode (tests/scaled_model.py) against three yardsticks:
 1. its integer form against its float64 form (IEEE 1180's accuracy requirement: peak error 1),
 2. against the oracle's full decode, box-averaged (a gain or phase error of the definition would show as >= 2 levels),
 3. against libjpeg-turbo's reduced IDCTs through Pillow's Image.draft, with a one-pixel shift as the control."""
import importlib
import os

import numpy as np
import pytest

import oracle_c as oc
import scaled_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# (N_x, N_y) a sampling mode can produce: luma and unsampled chroma (4,4) (2,2) (1,1); 4:2:0 chroma (8,8)* (4,4) (2,2);
# 4:2:2 chroma (8,4) (4,2) (2,1); 4:4:0 chroma (4,8) (2,4) (1,2).  (*: the full transform, not the reduced one.)
SHAPES = [(4, 4), (2, 2), (1, 1), (8, 4), (4, 2), (2, 1), (4, 8), (2, 4), (1, 2)]
FILES = ["test-baseline.jpg", "ref/medium_no_samp_2500x1786.jpg", "ref/medium_horiz_samp_2500x1786.jpg",
         "ref/medium_vertical_samp_2500x1786.jpg", "ref/speed_bench_hv_subsampling.jpg"]


def zj_mod():
    return importlib.import_module("zune-jpeg_amd")


_COEF = {}


def file_coefficients(name):
    """the front-end's planes of a fixture file, the values the file codes (ZJ_FLAG_FULL_AC_VALUES)"""
    if name not in _COEF:
        zj = zj_mod()
        o = zj.ZuneJpegOptions()
        o.flags = zj.FLAG_FULL_AC_VALUES
        desc, planes, info = zj.Decoder(o).decode_coefficients(open(os.path.join(GOLDEN, name), "rb").read())
        _COEF[name] = ([np.array(p) for p in planes], [np.array(q) for q in np.ctypeslib.as_array(desc.qt)], info)
    return _COEF[name]


def test_matrices_symmetry_and_fold():
    """A_N[N-1-m][k] = (-1)^k A_N[m][k]; the fold: A_4's column 4 is zero and its columns 5, 6, 7 are multiples of 3, 2, 1;
    A_1 is DC / 8 in two dimensions"""
    for n in (1, 2, 4, 8):
        a = sm.float_matrix(n)
        assert np.allclose(a[::-1], a * np.array([1, -1] * 4)[None, :])
        assert np.allclose(a.sum(axis=0)[1:], 0) and np.isclose(a[:, 0].mean(), 1 / (2 * np.sqrt(2)))
    a4 = sm.float_matrix(4)
    assert np.allclose(a4[:, 4], 0)
    for k in (5, 6, 7):
        ratio = a4[:, k] / a4[:, 8 - k]
        assert np.allclose(ratio, ratio[0])
    assert np.isclose(sm.float_matrix(1)[0, 0] ** 2, 1 / 8)
    # the mean of the 8-point IDCT's outputs, directly
    a8 = sm.float_matrix(8)
    for n in (1, 2, 4):
        assert np.allclose(sm.float_matrix(n), a8.reshape(n, 8 // n, 8).mean(axis=1))


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_integer_form_meets_ieee1180_peak_error(nx, ny):
    """random blocks in the standard's three ranges (-256..255, -5..5, -300..300: the IDCT's INPUT, i.e. the dequantised
    values, here products of a coefficient and a table entry of up to 255) against the float64 definition, rounded: peak
    error at most 1"""
    rng = np.random.default_rng(1180 + 8 * nx + ny)
    for (lo, hi) in ((-256, 255), (-5, 5), (-300, 300)):
        for sign in (1, -1):
            for qmax in (1, 16, 255):
                q = rng.integers(1, qmax + 1, 64)
                q[rng.integers(64)] = qmax
                v = sign * rng.integers(lo, hi + 1, (10000, 64))
                c = np.trunc(v / q[None, :]).astype(np.int16)  # c x q stays inside the range
                deq = (c.astype(np.int64) * q[None, :]).reshape(-1, 8, 8)
                got = sm.int_samples(c, q, nx, ny).astype(np.int32)
                err = np.abs(got - sm.float_rounded(deq, nx, ny))
                print(f"N {nx}x{ny} range {lo}..{hi} sign {sign} q<={qmax}: peak {err.max()}, differing {np.mean(err != 0):.4f}")
                assert err.max() <= 1


@pytest.mark.parametrize("name", FILES)
def test_integer_form_on_fixture_coefficients(name):
    planes, qts, info = file_coefficients(name)
    for c, (plane, qt) in enumerate(zip(planes, qts)):
        blocks = plane.reshape(-1, 64)[:: max(1, plane.size // 64 // 20000)]
        deq = (blocks.astype(np.int64) * qt[None, :].astype(np.int64)).reshape(-1, 8, 8)
        for (nx, ny) in SHAPES:
            err = np.abs(sm.int_samples(blocks, qt, nx, ny).astype(np.int32) - sm.float_rounded(deq, nx, ny))
            assert err.max() <= 1, (name, c, nx, ny)


# ---- 2. the oracle's full decode, box-averaged ------------------------------------------------------------------
# What separates a reduced sample from the mean of the s x s full-decode bytes under it: the rounding of the mean itself
# (<= 0.5), the mean of up to 64 roundings of the full decode (each <= 0.5 + its fixed-point error), and this model's
# fixed-point error.  MEASURED over the 48 frames below: 1.000, which is a half grey level's multiple
# already: that is the bound.  (2 or more would be a gain or phase error of the definition.)
ORACLE_BOUND = 1.0


def tame_frame(synth, W, H, ncomp, seed):
    """a synth.py frame with its DC walk compressed into the middle of the range, so that nothing saturates"""
    planes, qts = synth.make_frame(W, H, 1, 1, ncomp, seed=seed)
    out = []
    for p in planes:
        b = np.array(p, np.int16).reshape(-1, 64)
        b[:, 0] = b[:, 0] // 8
        b[:, 1:] = b[:, 1:] // 2
        out.append(b.reshape(-1))
    return out, qts


def test_model_against_box_averaged_oracle(synth):
    """4:4:4 and grayscale frames on which the oracle (corrected flags) produces no byte at 0 or 255.  W or H not a
    multiple of s: the reduced frame's last column / row stands for pixels of the edge blocks beyond the frame; the oracle
    decodes the same planes at the padded size (the blocks' own 8 x 8 pixels), and the reduced frame is compared on the
    pixels the full frame has -- its ceil(W / s) x ceil(H / s) cells."""
    worst = 0.0
    used = 0
    for ncomp in (1, 3):
        for (W, H) in [(96, 64), (100, 50), (203, 77), (64, 121)]:
            Wp, Hp = (W + 7) // 8 * 8, (H + 7) // 8 * 8
            for seed in range(6):
                planes, qts = tame_frame(synth, W, H, ncomp, seed)
                out_cs = oc.GRAYSCALE if ncomp == 1 else oc.YCBCR
                rc, full = oc.decode_planes(oc.make_frame(Wp, Hp, 1, 1, ncomp, out_cs, qts), planes, ext=oc.EXT_CLAMP_DC | oc.EXT_EDGE_REP)
                assert rc == 0
                luma = full.reshape(Hp, Wp, -1)[:, :, 0].astype(np.float64)
                if luma.min() <= 0 or luma.max() >= 255:
                    continue
                used += 1
                for sl in (1, 2, 3):
                    s = 1 << sl
                    red = sm.decode_scaled_ycc(W, H, 1, 1, ncomp, qts, planes, sl)[0].astype(np.float64)
                    rw, rh = sm.scaled_size(W, H, sl)
                    assert red.shape == (rh, rw)
                    box = luma[:rh * s, :rw * s].reshape(rh, s, rw, s).mean(axis=(1, 3))
                    d = np.abs(red - box).max()
                    worst = max(worst, d)
                    assert d <= ORACLE_BOUND, (ncomp, W, H, seed, sl, d)
    print(f"model vs box-averaged oracle: worst {worst:.3f} over {used} frames")
    assert used >= 24


# ---- 3. libjpeg-turbo through Pillow ------------------------------------------------------------------------------
# mean absolute difference per channel, MEASURED on the build machine (Pillow 12.2, libjpeg-turbo) and asserted with a
# quarter grey level of margin for other builds' IDCT rounding; see DESIGN.md 3.7 for the table and for why the
# sub-sampled chroma of some modes differs more (libjpeg-turbo scales the chroma IDCT by the same factor as luma's and
# up-samples the result, where this definition lands every component on the reduced grid directly).
PILLOW_MEASURED = {
    ("test-baseline.jpg", 1): (0.001, 0.0, 0.0),  # shifted by one pixel: luma 2.03
    ("test-baseline.jpg", 2): (0.001, 0.0, 0.0),  # 3.99
    ("test-baseline.jpg", 3): (0.0, 0.0, 0.0),  # 7.49
    ("ref/medium_no_samp_2500x1786.jpg", 1): (0.03, 0.011, 0.026),  # 2.79
    ("ref/medium_no_samp_2500x1786.jpg", 2): (0.024, 0.006, 0.02),  # 2.56
    ("ref/medium_no_samp_2500x1786.jpg", 3): (0.0, 0.0, 0.0),  # 3.26
    ("ref/medium_horiz_samp_2500x1786.jpg", 1): (0.03, 0.107, 0.221),  # 2.79
    ("ref/medium_horiz_samp_2500x1786.jpg", 2): (0.024, 0.208, 0.432),  # 2.56
    ("ref/medium_horiz_samp_2500x1786.jpg", 3): (0.0, 0.289, 0.549),  # 3.26
    ("ref/medium_vertical_samp_2500x1786.jpg", 1): (0.03, 0.109, 0.23),  # 2.79
    ("ref/medium_vertical_samp_2500x1786.jpg", 2): (0.024, 0.217, 0.454),  # 2.56
    ("ref/medium_vertical_samp_2500x1786.jpg", 3): (0.0, 0.291, 0.566),  # 3.26
    ("ref/speed_bench_hv_subsampling.jpg", 1): (0.019, 0.303, 0.288),  # 0.41 (a smooth image: little detail to shift)
    ("ref/speed_bench_hv_subsampling.jpg", 2): (0.022, 0.002, 0.004),  # 0.40
    ("ref/speed_bench_hv_subsampling.jpg", 3): (0.0, 0.001, 0.002),  # 0.35
}


def pillow_draft(name, sl):
    from PIL import Image, features
    if not features.check("jpg"):
        pytest.skip("Pillow without JPEG support")
    im = Image.open(os.path.join(GOLDEN, name))
    W, H = im.size
    s = 1 << sl
    im.draft("YCbCr", (W // s, H // s))  # the floor: asked for the ceiling Pillow picks the next smaller scale for odd sizes
    assert im.mode == "YCbCr" and im.size == (-(-W // s), -(-H // s)), (im.mode, im.size)
    return np.asarray(im, np.int32)


def model_ycc(name, sl):
    planes, qts, info = file_coefficients(name)
    ycc = sm.decode_scaled_ycc(info.width, info.height, info.h_max, info.v_max, 3, qts, planes, sl, clamp_dc=True)
    return np.stack([np.clip(c, 0, 255) for c in ycc], axis=-1).astype(np.int32)


def mad_per_channel(a, b, name, sl):
    d = np.abs(a - b).astype(np.float64)
    if name == "test-baseline.jpg":  # the reference never decodes the file's last 7 MCUs (test_jpeg_frontend.py): mid grey
        s = 1 << sl
        d[134 * 8 // s:, 233 * 8 // s:] = 0
    return d.reshape(-1, 3).mean(axis=0)


@pytest.mark.parametrize("sl", [1, 2, 3])
@pytest.mark.parametrize("name", FILES)
def test_model_against_libjpeg_turbo_draft(name, sl):
    pytest.importorskip("PIL")
    pil = pillow_draft(name, sl)
    ours = model_ycc(name, sl)
    assert ours.shape == pil.shape
    aligned = mad_per_channel(ours, pil, name, sl)
    shifted = mad_per_channel(ours[:, 1:], pil[:, :-1], name, sl)  # the model's image one reduced pixel to the left
    print(f"{name} 1/{1 << sl}: aligned {np.round(aligned, 3).tolist()} shifted {np.round(shifted, 3).tolist()}")
    measured = PILLOW_MEASURED[(name, sl)]
    for ch in range(3):
        bound = measured[ch] + 0.25
        assert aligned[ch] <= bound, (name, sl, ch, aligned[ch], bound)
    # The test's power: shifted by one reduced pixel, the comparison must fail.  This is asserted for LUMA, which carries
    # the detail; its margin is smallest on speed_bench_hv_subsampling.jpg, a smooth image (0.35-0.41 against 0.27).  The
    # CHROMA numbers of the sub-sampled modes (up to 0.57 + 0.25) are recorded, not discriminating: libjpeg-turbo
    # up-samples those components, and bounds of that size would also admit a truncated transform.  What
    # pins chroma's transform is that it is luma's code at the same N (4:4:4 chroma, 0.03 here) and test 1.
    assert shifted[0] > PILLOW_MEASURED[(name, sl)][0] + 0.25, (name, sl, shifted[0])
