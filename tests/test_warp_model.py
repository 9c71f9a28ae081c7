"""CPU: the affine warp's definition (tests/warp_model.py) against what it must reduce to -- the to-tensor
stage at the identity, the displayed image at the eight EXIF orientations, the bilinear resize at power-of-two scales -- against
float64 grid_sample within the derived bound, its source window by brute force, and the library's host-side rules
(zune-jpeg_amd/csrc/zj_warp_fixed.h, through tests/emu_warp) against the model's."""
import math

import numpy as np
import pytest

import emu_warp_c as ew
import orient_model as om
import resize_model as rm
import warp_model as wm


def noise(rng, w, h, ch):
    return rng.integers(0, 256, (h, w, ch), dtype=np.uint8)


def smooth(w, h, ch):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    planes = [127.5 + 127.5 * np.sin(0.19 * x + 0.11 * y + c) * np.cos(0.07 * x - 0.13 * y + 2 * c) for c in range(ch)]
    return np.clip(np.rint(np.stack(planes, -1)), 0, 255).astype(np.uint8)


def random_matrix(rng, w, h, ow, oh):
    """rotation + scale + shear + translate about the centres, output pixel centre -> source coordinates"""
    t = rng.uniform(-math.pi, math.pi)
    sx, sy = rng.uniform(0.4, 2.5, 2) * (w / ow, h / oh)
    sh = rng.uniform(-0.4, 0.4)
    lin = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]]) @ np.array([[1, sh], [0, 1]]) @ np.diag([sx, sy])
    off = np.array([w / 2, h / 2]) + rng.uniform(-0.3, 0.3, 2) * (w, h) - lin @ np.array([ow / 2, oh / 2])
    return (lin[0, 0], lin[0, 1], off[0], lin[1, 0], lin[1, 1], off[1])


# ---- what the definition reduces to ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
def test_the_identity_is_the_to_tensor_stage(ch):
    rng = np.random.default_rng(ch)
    img = noise(rng, 13, 7, ch)
    q = wm.fixed((1, 0, 0, 0, 1, 0))
    assert q == [1 << 24, 0, 0, 0, 1 << 24, 0]
    for edge in (wm.FILL, wm.REPLICATE):
        v = wm.values(img, q, 13, 7, edge, (9, 9, 9))
        assert np.array_equal(v, img.transpose(2, 0, 1).astype(np.int64) << 16)
    mean, std = np.float32([0.485, 0.456, 0.406])[:ch], np.float32([0.229, 0.224, 0.225])[:ch]
    scale, bias = (1 / (255 * std)).astype(np.float32), (-mean / std).astype(np.float32)
    for dtype in (rm.F32, rm.F16, rm.BF16, rm.U8):
        for layout in ("NCHW", "NHWC"):
            got = wm.warp(img, q, 13, 7, dtype, scale, bias, wm.FILL, None, layout)
            exp = rm.resize(img.transpose(2, 0, 1), 13, 7, dtype, scale, bias, False, layout)  # (the to-tensor stage's model)
            assert got.dtype == exp.dtype and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(exp).view(np.uint8))


@pytest.mark.parametrize("o", range(1, 9))
def test_an_orientation_is_an_integer_matrix(o):
    rng = np.random.default_rng(o)
    W, H = 11, 6
    img = noise(rng, W, H, 3)
    dw, dh = om.oriented_size(o, W, H)
    m = wm.orientation_matrix(o, W, H)
    if o == 6:
        assert m == (0, 1, 0, -1, 0, H)
    q = wm.fixed(m)
    assert all(v % (1 << 24) == 0 for v in q)
    for edge in (wm.FILL, wm.REPLICATE):
        v = wm.values(img, q, dw, dh, edge, (200, 100, 50))
        assert np.array_equal(v, om.orient(img, o).transpose(2, 0, 1).astype(np.int64) << 16)


@pytest.mark.parametrize("kx", [-2, -1, 1, 2])
@pytest.mark.parametrize("ky", [-2, -1, 1, 2])
def test_a_power_of_two_scale_is_the_bilinear_resize(kx, ky):
    """out = in x 2^k per axis, REPLICATE: resize_model's values, element for element"""
    rng = np.random.default_rng(100 + 10 * kx + ky)
    w, h = 24, 12
    img = noise(rng, w, h, 3)
    ow, oh = (w << kx if kx > 0 else w >> -kx), (h << ky if ky > 0 else h >> -ky)
    q = wm.fixed((2.0 ** -kx, 0, 0, 0, 2.0 ** -ky, 0))
    assert np.array_equal(wm.values(img, q, ow, oh, wm.REPLICATE), rm.values(img.transpose(2, 0, 1), ow, oh))


def test_another_ratio_is_close_to_the_resize_but_not_equal():
    rng = np.random.default_rng(4)
    img = noise(rng, 30, 20, 1)
    q = wm.fixed((30 / 13, 0, 0, 0, 20 / 7, 0))
    d = np.abs(wm.values(img, q, 13, 7, wm.REPLICATE) - rm.values(img.transpose(2, 0, 1), 13, 7))
    assert d.max() < 65536  # (under one grey level; no equality is claimed)


# ---- the float reference ---------------------------------------------------------------------------------------------
def grid_sample_ref(img, m, ow, oh, edge):
    import torch
    import torch.nn.functional as F
    h, w, ch = img.shape
    Y, X = np.meshgrid(np.arange(oh) + 0.5, np.arange(ow) + 0.5, indexing="ij")
    sx = m[0] * X + m[1] * Y + m[2]
    sy = m[3] * X + m[4] * Y + m[5]
    grid = torch.from_numpy(np.stack([2 * sx / w - 1, 2 * sy / h - 1], -1)[None]).double()
    src = torch.from_numpy(img.transpose(2, 0, 1)[None].astype(np.float64))
    out = F.grid_sample(src, grid, mode="bilinear", padding_mode="border" if edge == wm.REPLICATE else "zeros", align_corners=False)
    return out[0].numpy()


@pytest.mark.parametrize("edge", [wm.FILL, wm.REPLICATE], ids=["fill", "replicate"])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_the_bound_against_float64_grid_sample(edge, kind):
    """|v / 65536 - ref| < 2 . 255 / 256 + 255 . 2 (out_w + out_h + 1) 2^-25 < 2.0 grey levels: each axis is low by less than
    1/256 pixel (truncation), the matrix's rounding adds at most (out_w + out_h + 1) 2^-25 pixel, and bilinear u8 data is
    255-Lipschitz per axis.  Asserted at 2.0, as derived."""
    rng = np.random.default_rng(40 + edge + (7 if kind == "smooth" else 0))
    worst = 0.0
    for i in range(40):
        w, h = int(rng.integers(5, 80)), int(rng.integers(5, 60))
        ow, oh = int(rng.integers(1, 65)), int(rng.integers(1, 49))
        img = noise(rng, w, h, 3) if kind == "noise" else smooth(w, h, 3)
        m = random_matrix(rng, w, h, ow, oh)
        q = wm.fixed(m)
        assert q is not None
        v = wm.values(img, q, ow, oh, edge) / 65536.0
        err = np.abs(v - grid_sample_ref(img, m, ow, oh, edge)).max()
        worst = max(worst, err)
        assert err < 2.0, (i, m, err)
    print(f"largest error over 40 matrices, {kind}, edge {edge}: {worst:.3f} grey levels")


# ---- the source window -----------------------------------------------------------------------------------------------
def window_matrices(rng, fw, fh, ow, oh):
    ms = [random_matrix(rng, fw, fh, ow, oh) for _ in range(6)]
    ms += [wm.orientation_matrix(o, fw, fh) for o in range(1, 9)]
    ms += [(1, 0, fw + 3, 0, 1, 0), (1, 0, 0, 0, 1, -(oh + 2)), (1, 0, -ow / 2, 0, 1, fh - 0.5), (0.25, 0, fw - 1, 0, 0.25, 0),
           (1, 0, -ow - 5, 0, 1, fh + 5)]
    return ms


@pytest.mark.parametrize("edge", [wm.FILL, wm.REPLICATE], ids=["fill", "replicate"])
def test_the_window_holds_every_tap_and_warps_the_same(edge):
    rng = np.random.default_rng(90 + edge)
    fill = (7, 130, 255)
    seen_empty = seen_part = 0
    for (fw, fh) in ((1, 1), (2, 1), (3, 4), (9, 7), (5, 7)):
        frame = noise(rng, fw, fh, 3)
        for (ow, oh) in ((1, 1), (4, 3), (7, 5)):
            for m in window_matrices(rng, fw, fh, ow, oh):
                q = wm.fixed(m)
                (x, y, w, h), sh = wm.source_window(q, fw, fh, ow, oh, edge)
                assert ew.window(q, fw, fh, ow, oh, edge) == ((x, y, w, h), sh), (m, fw, fh, ow, oh)
                full = wm.values(frame, q, ow, oh, edge, fill)
                if w == 0:
                    assert edge == wm.FILL and h == 0
                    assert np.array_equal(full, np.broadcast_to((np.array(fill, np.int64) << 16)[:, None, None], full.shape))
                    seen_empty += 1
                    continue
                assert 0 <= x and 0 <= y and x + w <= fw and y + h <= fh
                # every tap, one by one: inside the frame -> inside the window (fill); clamped into the frame -> there (replicate)
                x0, _, y0, _ = wm.positions(q, ow, oh)
                for tx, ty in ((x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)):
                    if edge == wm.REPLICATE:
                        tx, ty = np.clip(tx, 0, fw - 1), np.clip(ty, 0, fh - 1)
                        assert ((tx >= x) & (tx < x + w) & (ty >= y) & (ty < y + h)).all()
                    else:
                        inx, iny = (tx >= 0) & (tx < fw), (ty >= 0) & (ty < fh)
                        assert (~inx | ((tx >= x) & (tx < x + w))).all() and (~iny | ((ty >= y) & (ty < y + h))).all()
                assert sh[2] == q[2] - (x << 24) and sh[5] == q[5] - (y << 24) and sh[:2] + sh[3:5] == q[:2] + q[3:5]
                assert np.array_equal(wm.values(frame[y:y + h, x:x + w], sh, ow, oh, edge, fill), full), (m, fw, fh, ow, oh)
                seen_part += (w, h) != (fw, fh)
    assert seen_part > 20 and (edge == wm.REPLICATE or seen_empty > 5)


# ---- zj_warp_fixed ---------------------------------------------------------------------------------------------------
def test_the_fixed_point_rounding():
    e = 2.0 ** -25  # half a unit
    assert wm.fixed((e, -e, 0, 3 * e, -3 * e, 0))[:2] == [1, 0] and wm.fixed((e, -e, 0, 3 * e, -3 * e, 0))[3:5] == [2, -1]
    assert wm.fixed((1, 0, 0, 0, 1, 0)) == [1 << 24, 0, 0, 0, 1 << 24, 0]
    assert wm.fixed((0, 0, 0.5 + e, 0, 0, 0.5 - 2 * e))[2::3] == [1, -1]  # (C0 = round((c - 1/2) 2^24): ties go up)
    assert wm.fixed((2, 1, 10, -1, 0.5, -3))[2::3] == [(1 + 0.5 + 10) * 2 ** 24 - (1 << 23), int((-0.5 + 0.25 - 3 - 0.5) * 2 ** 24)]
    rng = np.random.default_rng(8)
    ms = [tuple(rng.uniform(-127.9, 127.9, 6) * (1, 1, 1e4, 1, 1, 1e4)) for _ in range(200)]
    ms += [(127.99999999, -127.99999999, 2.0 ** 31 - 1, 1e-300, -1e-300, -(2.0 ** 31 - 1)), (0, 0, 0, 0, 0, 0)]
    for m in ms:
        assert ew.fixed(m) == wm.fixed(m) is not None, m


@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), "limit", "-limit"])
def test_the_refusals(k, bad):
    lim = 2.0 ** 31 if k % 3 == 2 else 128.0
    v = {"limit": lim, "-limit": -lim}.get(bad, bad)
    m = [0.5, 0.25, 3.0, -0.5, 1.0, -7.0]
    m[k] = v
    assert wm.fixed(m) is None and ew.fixed(m) is None
    if isinstance(bad, str):
        m[k] = math.nextafter(v, 0.0)
        assert wm.fixed(m) is not None and ew.fixed(m) == wm.fixed(m)


# ---- tensors.warp_matrix, by its properties --------------------------------------------------------------------------
def tensors():
    import importlib
    return importlib.import_module("zune-jpeg_amd.tensors")


def test_warp_matrix_identity_rot90_and_letterbox():
    T = tensors()
    rng = np.random.default_rng(12)
    W, H = 10, 6
    img = noise(rng, W, H, 3)
    assert T.warp_matrix((W, H), (W / 2, H / 2)) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    # 90 degrees, counter-clockwise as displayed: numpy's rot90, exactly (the matrix is integral up to rounding of cos 90)
    q = wm.fixed(T.warp_matrix((H, W), (W / 2, H / 2), angle=90))
    v = wm.values(img, q, H, W, wm.REPLICATE)
    # (cos 90 degrees is 6e-17 in doubles: a position may be one step of 1/256 off per axis, 255 x 256 units each)
    assert np.abs(v - (np.rot90(img).transpose(2, 0, 1).astype(np.int64) << 16)).max() <= 2 * 255 * 256
    assert np.array_equal((v + 32768) >> 16, np.rot90(img).transpose(2, 0, 1))
    # the mirror
    v = wm.values(img, wm.fixed(T.warp_matrix((W, H), (W / 2, H / 2), hflip=True)), W, H, wm.FILL)
    assert np.array_equal(v, img[:, ::-1].transpose(2, 0, 1).astype(np.int64) << 16)
    # a translate moves the content by whole output pixels
    v = wm.values(img, wm.fixed(T.warp_matrix((W, H), (W / 2, H / 2), translate=(2, -1))), W, H, wm.FILL, (5, 5, 5))
    assert np.array_equal(v[:, :H - 1, 2:], img[1:, :W - 2].transpose(2, 0, 1).astype(np.int64) << 16)
    assert (v[:, H - 1] == 5 << 16).all() and (v[:, :, :2] == 5 << 16).all()
    # the letterbox: a 10 x 6 image into 20 x 20 is scaled by 2 to 20 x 12, centred, rows 4 .. 15; fill above and below
    S = 20
    m = T.warp_matrix((S, S), (W / 2, H / 2), scale=min(S / W, S / H))
    assert m == (0.5, 0.0, 0.0, 0.0, 0.5, -2.0)
    v = wm.values(img, wm.fixed(m), S, S, wm.FILL, (114, 114, 114))
    assert (v[:, :3] == 114 << 16).all() and (v[:, 17:] == 114 << 16).all()
    assert np.array_equal(v[:, 5:15, 1:19], rm.values(img.transpose(2, 0, 1), S, 12)[:, 1:11, 1:19])
    with pytest.raises(ValueError):
        T.warp_matrix((S, S), (0, 0), scale=0)
