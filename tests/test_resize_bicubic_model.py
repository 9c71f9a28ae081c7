"""CPU: the numpy model of the bicubic antialiased resize (tests/resize_bicubic_model.py) against its own
properties, torch's F.interpolate(mode="bicubic", antialias=True) in float64 and, where it is installed, Pillow's BICUBIC."""
import numpy as np
import pytest

import resize_bicubic_model as bm
import resize_model as rm

AXES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 5), (8, 4), (9, 4), (64, 224), (224, 64), (500, 224), (4096, 224),
        (65535, 1), (65535, 8192), (1, 8192)]
# measured over REFERENCE_CASES (profiles/resize_bicubic.txt): the largest |model - torch float64| in grey levels; the
# share of u8 pixels two or more levels from Pillow's.  The tests assert twice each (Pillow: capped at 1 % of the pixels).
TORCH_MEASURED = 0.0277
PILLOW_GE2_MEASURED = 183 / 434816  # (0.042 %; 98.26 % equal, 1.70 % one level)


@pytest.mark.parametrize("n,m", AXES)
def test_weights_sum_to_2_14_over_a_positive_S(n, m):
    j, w, S = bm.taps(n, m)  # (asserts S > 0, the tap count, |C_j| 2^14 < 2^63, sum |w| <= 2^15 and |w| < 2^15 itself)
    assert (w.sum(axis=1) == 1 << 14).all() and (S > 0).all()
    assert (j >= 0).all() and (j < n).all()
    if n == m:  # the identity: one tap of 2^14 on j = i, K(T) = 0 on its neighbours
        assert np.array_equal(j[w != 0], np.arange(n)) and (w[w != 0] == 1 << 14).all()
    if n == 2 * m and m >= 5:  # an interior output: its taps mirror about the centre
        i = m // 2
        dense = np.zeros(n, np.int64)
        np.add.at(dense, j[i], w[i])
        lo, hi = 2 * i - 3, 2 * i + 4  # 8 taps, the centre between source pixels 2i and 2i + 1
        assert dense[:lo].sum() == 0 and dense[hi + 1:].sum() == 0
        assert np.array_equal(dense[lo:hi + 1], dense[lo:hi + 1][::-1]) and (dense[lo:hi + 1] != 0).all()


def test_a_symmetric_interior_output_of_a_halving():
    """n = 2m: (8, 4) has no interior output (every output is cut by an edge), (224, 112) has"""
    j, w, _ = bm.taps(224, 112)
    for i in (2, 56, 109):
        dense = np.zeros(224, np.int64)
        np.add.at(dense, j[i], w[i])
        seg = dense[2 * i - 3:2 * i + 5]
        assert dense.sum() == seg.sum() == 1 << 14 and np.array_equal(seg, seg[::-1]) and seg[0] < 0 and seg[3] > 0


def test_kernel_is_keys_cubic():
    T = bm.T
    q = np.array([0, 1, T // 2, T - 1, T, T + 1, 3 * T // 2, 2 * T - 1], np.int64)
    K = bm.kernel(q)
    assert K[0] == 2 * T ** 3 and K[4] == 0 and (K[:4] > 0).all() and (K[5:] < 0).all()
    x = q / T  # a = -1/2: 1.5 x^3 - 2.5 x^2 + 1, and -0.5 x^3 + 2.5 x^2 - 4 x + 2
    f = np.where(x < 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2)
    assert np.allclose(K / (2 * T ** 3), f, atol=1e-12)


@pytest.mark.parametrize("kind", ["white", "black", "checker"])
def test_stated_ranges_hold(kind):
    """|t| <= T_MAX and |horizontal sum| <= H_MAX (asserted inside passes()); all-255 and all-0 stay exact"""
    for (w, h, ow, oh) in [(37, 29, 8, 8), (16, 16, 40, 24), (9, 8, 4, 4), (64, 3, 224, 7), (500, 2, 224, 1)]:
        if kind == "checker":
            yy, xx = np.mgrid[0:h, 0:w]
            img = (((xx + yy) & 1) * 255).astype(np.uint8)[None]
        else:
            img = np.full((1, h, w), 255 if kind == "white" else 0, np.uint8)
        t, hs, v = bm.passes(img, ow, oh)
        assert np.abs(t).max() <= bm.T_MAX and np.abs(hs).max() <= bm.H_MAX
        if kind != "checker":  # weights that sum to 2^14: a flat image stays flat, to the bit
            assert (t == (255 * 256 if kind == "white" else 0)).all() and (v == (bm.V_MAX if kind == "white" else 0)).all()


def test_the_final_clamp_engages_under_the_negative_lobes():
    img = np.zeros((1, 4, 64), np.uint8)
    img[:, :, 1::2] = 255  # alternating 0 / 255 columns, enlarged: the outputs over the extreme pixels overshoot both ways
    v = bm.passes(img, 224, 4)[2]
    assert v.min() < 0 and v.max() > bm.V_MAX
    out = bm.resize(img, 224, 4, rm.U8)
    assert out.min() == 0 and out.max() == 255


def test_identity_windows_give_the_crop():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (3, 33, 57), dtype=np.uint8)
    assert np.array_equal(bm.resize(img, 57, 33, rm.U8), img)
    for dt in (rm.F32, rm.F16, rm.BF16):
        exp = np.ascontiguousarray(rm.resize(img, 57, 33, dt, [0.01] * 3, [-1.0] * 3))
        assert np.array_equal(bm.resize(img, 57, 33, dt, [0.01] * 3, [-1.0] * 3).view(np.uint8), exp.view(np.uint8))


REFERENCE_SIZES = [((37, 29), (8, 8)), ((37, 29), (64, 48)), ((200, 160), (10, 8)), ((16, 16), (40, 24)), ((224, 224), (224, 224))]
REFERENCE_CASES = [(s, d, k, c) for (s, d) in REFERENCE_SIZES for k in ("noise", "smooth") for c in (1, 3)]


def reference_image(src, kind, channels):
    rng = np.random.default_rng(src[0] * 7 + src[1] + channels)
    if kind == "noise":
        return rng.integers(0, 256, (channels, src[1], src[0]), dtype=np.uint8)
    yy, xx = np.mgrid[0:src[1], 0:src[0]]
    return np.stack([127.5 + 127 * np.sin(xx / (7.0 + 5 * c) + yy / (9.0 + 3 * c)) for c in range(channels)]).astype(np.uint8)


def torch_error(src, dst, kind, channels):
    import torch
    import torch.nn.functional as F
    img = reference_image(src, kind, channels)
    got = bm.values(img, dst[0], dst[1]).astype(np.float64) / 65536
    ref = F.interpolate(torch.from_numpy(img.astype(np.float64))[None], size=(dst[1], dst[0]), mode="bicubic",
                        align_corners=False, antialias=True)[0].clamp(0, 255).numpy()
    return np.abs(got - ref).max()


@pytest.mark.parametrize("src,dst,kind,channels", REFERENCE_CASES)
def test_model_is_torch_antialiased_bicubic(src, dst, kind, channels):
    pytest.importorskip("torch")
    err = torch_error(src, dst, kind, channels)
    print(f"{src} -> {dst} {kind} x{channels}: {err:.5f} grey levels")
    assert err <= 2 * TORCH_MEASURED, err
    if src == dst:
        assert err == 0


def pillow_differences(src, dst, kind, channels):
    """the counts of u8 pixels 0, 1 and >= 2 levels from Pillow's BICUBIC resize of the same image"""
    from PIL import Image
    img = reference_image(src, kind, channels)
    got = bm.resize(img, dst[0], dst[1], rm.U8)
    ref = np.stack([np.asarray(Image.fromarray(p).resize(dst, Image.BICUBIC)) for p in img])
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    return int((d == 0).sum()), int((d == 1).sum()), int((d >= 2).sum())


def test_model_against_pillow_bicubic():
    """Pillow rounds its intermediate to u8, so single levels differ; two or more is what the bound is on"""
    pytest.importorskip("PIL")
    tot = np.zeros(3, np.int64)
    for case in REFERENCE_CASES:
        tot += pillow_differences(*case)
    share = tot / tot.sum()
    print(f"Pillow BICUBIC: {share[0]:.4%} equal, {share[1]:.4%} one level, {share[2]:.4%} two or more, of {tot.sum()} pixels")
    assert share[2] <= min(2 * PILLOW_GE2_MEASURED, 0.01)
    assert share[0] >= 0.5  # (measured: see profiles/resize_bicubic.txt)
