"""CPU: the reduced-size decode (zj_decode_crops_scaled_device) -- the kernel's phases emulated thread by
thread (tests/emu_scaled) equal the numpy definition (tests/scaled_model.py) bit for bit, and the plans (reduced frame,
windows, the prescaled resize's scale choice and reduced window) equal brute-force statements."""
import zlib

import numpy as np
import pytest

import emu_scaled_c as es
import scaled_model as sm

MODES = {"none": (1, 1), "h": (2, 1), "v": (1, 2), "hv": (2, 2)}
KINDS = {"rgb": (sm.RGB, 0), "gray": (sm.GRAYSCALE, 0), "ycbcr": (sm.YCBCR, 0), "chw": (sm.RGB, 1)}
ERR_ARG, ERR_UNSUPPORTED = -1, -2
# full-resolution pixels of a tile row (zj_scaled.h: ScaledCfg::TM x 8 x HS)
TILE_PX = {("none", False): 512, ("h", False): 1024, ("v", False): 512, ("hv", False): 512,
           ("none", True): 2048, ("h", True): 2048, ("v", True): 1024, ("hv", True): 1024}


def model_frame(W, H, hs, vs, qts, planes, sl, kind, flags=0):
    out_cs, layout = KINDS[kind]
    return sm.decode_scaled(W, H, hs, vs, 3, out_cs, qts, planes, sl, chw=layout == 1, clamp_dc=bool(flags & 2))


def check(d, planes, sl, kind, exp, windows, out_pitch=0, nframes=None):
    """windows: None = the whole reduced frame, else a list of (x, y, w, h), one frame each"""
    chw = kind == "chw"
    bpp = 1 if chw or kind == "gray" else 3
    n = nframes or (len(windows) if windows is not None else 1)
    rc, outs = es.decode(d, [planes] * n, sl, windows, out_pitch=out_pitch)
    assert rc == 0, (kind, sl, windows, rc)
    rh, rw = exp.shape[-2:] if chw else exp.shape[:2]
    for i, got in enumerate(outs):
        x, y, w, h = windows[i] if windows is not None else (0, 0, rw, rh)
        pitch = out_pitch or w * bpp
        rows = got.reshape(3, h, pitch) if chw else got.reshape(h, pitch)
        want = exp[:, y:y + h, x:x + w] if chw else exp[y:y + h, x:x + w].reshape(h, w * bpp)
        body = rows[..., :w * bpp]
        if not np.array_equal(body, want):
            bad = np.argwhere(body != want)
            raise AssertionError(f"{kind} 1/{1 << sl} {d.width}x{d.height} window {(x, y, w, h)}: {len(bad)} bytes differ, "
                                 f"first {bad[:4].tolist()}: got {body[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
        assert (rows[..., w * bpp:] == 0xAA).all(), "pitch padding written"


def windows_of(rw, rh, rng):
    """windows touching each edge and each corner, a one-pixel window, windows inside"""
    w2, h2 = max(1, rw // 2), max(1, rh // 2)
    wins = [(0, 0, rw, rh), (0, 0, 1, 1), (rw - 1, rh - 1, 1, 1), (rw - 1, 0, 1, 1), (0, rh - 1, 1, 1),
            (0, 0, w2, h2), (rw - w2, 0, w2, h2), (0, rh - h2, w2, h2), (rw - w2, rh - h2, w2, h2),
            (0, rh // 3, rw, 1), (rw // 3, 0, 1, rh)]
    for _ in range(3):
        w, h = int(rng.integers(1, rw + 1)), int(rng.integers(1, rh + 1))
        wins.append((int(rng.integers(rw - w + 1)), int(rng.integers(rh - h + 1)), w, h))
    return wins


@pytest.mark.parametrize("sl", [1, 2, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_small_frames_every_size(mode, sl, synth):
    """widths and heights 1..40, whole reduced frames, every output kind"""
    hs, vs = MODES[mode]
    sizes = [(W, (7 * W) % 40 + 1) for W in range(1, 41)] + [((11 * H) % 40 + 1, H) for H in range(1, 41)]
    for (W, H) in sizes:
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W * 41 + H)
        for kind, (out_cs, layout) in KINDS.items():
            d = es.desc(W, H, hs, vs, 3, out_cs, qts, out_layout=layout)
            assert es.scaled_size(d, sl) == (0,) + sm.scaled_size(W, H, sl)
            check(d, planes, sl, kind, model_frame(W, H, hs, vs, qts, planes, sl, kind), None)


@pytest.mark.parametrize("sl", [1, 2, 3])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mode", list(MODES))
def test_windows_and_tile_seams(mode, kind, sl, synth):
    """frames around multiples of the tile width; windows at every edge and corner, of one pixel, across the tile seams;
    every window a frame of one scattered launch"""
    hs, vs = MODES[mode]
    out_cs, layout = KINDS[kind]
    rng = np.random.default_rng(zlib.crc32(f"{mode}-{kind}-{sl}".encode()))
    T = TILE_PX[(mode, kind == "gray")]
    for (W, H) in [(T - 1, 19), (T, 9), (T + 1, 33), (2 * T + 5, 17), (37, 40), (100, 70)]:
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
        d = es.desc(W, H, hs, vs, 3, out_cs, qts, out_layout=layout)
        exp = model_frame(W, H, hs, vs, qts, planes, sl, kind)
        rw, rh = sm.scaled_size(W, H, sl)
        wins = windows_of(rw, rh, rng)
        s = 1 << sl
        if rw > T // s:  # across the first tile seam
            wins += [(T // s - 1, 0, 2, rh), (T // s, rh - 1, rw - T // s, 1), (T // s - 3, 0, min(7, rw - T // s + 3), 1)]
        check(d, planes, sl, kind, exp, wins)


@pytest.mark.parametrize("kind", list(KINDS))
def test_wide_pitch_keeps_padding(kind, synth):
    out_cs, layout = KINDS[kind]
    for (W, H, hs, vs, sl) in [(2500, 40, 2, 2, 1), (272, 33, 2, 1, 2), (13, 9, 1, 1, 1), (600, 70, 1, 2, 3)]:
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=3)
        d = es.desc(W, H, hs, vs, 3, out_cs, qts, out_layout=layout)
        exp = model_frame(W, H, hs, vs, qts, planes, sl, kind)
        rw, rh = sm.scaled_size(W, H, sl)
        w, h = min(rw, 37), min(rh, 11)
        bpp = 1 if kind in ("chw", "gray") else 3
        pitch = (w * bpp + 127) // 128 * 128 + 3
        check(d, planes, sl, kind, exp, [(0, 0, w, h), (rw - w, rh - h, w, h), ((rw - w) // 2, (rh - h) // 2, w, h)], out_pitch=pitch)


def test_batches_split_at_scatter_max(synth):
    """33 frames of their own planes and windows: two launches"""
    W, H, hs, vs, sl = 100, 50, 2, 2, 1
    frames, exps = [], []
    rng = np.random.default_rng(5)
    for i in range(33):
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=17, frame_index=i)
        frames.append(planes)
        exps.append(sm.decode_scaled(W, H, hs, vs, 3, sm.RGB, qts, planes, sl))
    d = es.desc(W, H, hs, vs, 3, sm.RGB, qts)
    rw, rh = sm.scaled_size(W, H, sl)
    wins = []
    for i in range(33):
        w, h = int(rng.integers(1, rw + 1)), int(rng.integers(1, rh + 1))
        wins.append((int(rng.integers(rw - w + 1)), int(rng.integers(rh - h + 1)), w, h))
    rc, outs = es.decode(d, frames, sl, wins)
    assert rc == 0
    for (x, y, w, h), got, exp in zip(wins, outs, exps):
        assert np.array_equal(got.reshape(h, w, 3), exp[y:y + h, x:x + w])


def test_flags_adversarial_and_single_component(synth):
    """ZJ_FLAG_CLAMP_DC acts on the components that take the full transform (4:2:0 chroma at 1/2), the other flags on
    nothing; unclamped DC-only chroma (Q1) passes through the colour arithmetic as in the full path; a single-component
    frame decodes to its luma, or to zeros for a colour output"""
    for (W, H, hs, vs) in [(100, 40, 2, 2), (70, 16, 1, 1)]:
        planes, qts = synth.make_adversarial_frame(W, H, hs, vs, 3, seed=99)
        for sl in (1, 2, 3):
            for kind, (out_cs, layout) in KINDS.items():
                for flags in (0, 2, 7):
                    d = es.desc(W, H, hs, vs, 3, out_cs, qts, flags=flags, out_layout=layout)
                    check(d, planes, sl, kind, model_frame(W, H, hs, vs, qts, planes, sl, kind, flags), None)
    planes, qts = synth.make_frame(45, 23, 1, 1, 1, seed=4)
    for sl in (1, 2, 3):
        rw, rh = sm.scaled_size(45, 23, sl)
        d = es.desc(45, 23, 1, 1, 1, sm.GRAYSCALE, qts)
        rc, outs = es.decode(d, [planes], sl)
        assert rc == 0 and np.array_equal(outs[0].reshape(rh, rw, 1), sm.decode_scaled(45, 23, 1, 1, 1, sm.GRAYSCALE, qts, planes, sl))
        for layout in (0, 1):
            d = es.desc(45, 23, 1, 1, 1, sm.RGB, qts, out_layout=layout)
            assert es.out_len(d, sl, rw, rh) == 3 * rw * rh
            rc, outs = es.decode(d, [planes], sl, [(1, 1, rw - 1, rh - 1)], out_pitch=3 * rw + 5)
            assert rc == 0
            rows = outs[0].reshape(-1, 3 * rw + 5)
            w = (rw - 1) * (1 if layout else 3)
            assert (rows[:, :w] == 0).all() and (rows[:, w:] == 0xAA).all()


def test_argument_errors(synth):
    planes, qts = synth.make_frame(100, 50, 2, 2, 3, seed=1)
    d = es.desc(100, 50, 2, 2, 3, sm.RGB, qts)
    assert es.decode(d, [planes], 0)[0] == ERR_ARG and es.decode(d, [planes], 4)[0] == ERR_ARG
    for win in [(0, 0, 0, 5), (0, 0, 5, 0), (46, 0, 5, 5), (0, 21, 5, 5), (50, 0, 1, 1)]:
        assert es.out_len(d, 1, win[2], win[3]) == 0 or es.decode(d, [planes], 1, [win])[0] == ERR_ARG, win
    assert es.out_len(d, 1, 10, 10, out_pitch=29) == 0 and es.out_len(d, 1, 10, 10, out_pitch=30) == 300
    dp = es.desc(100, 50, 2, 2, 3, sm.RGB, qts)
    dp.out_pitch = 384
    assert es.scaled_size(dp, 1)[0] == ERR_ARG
    for cs in (5, 6):  # RGBA, RGBX
        assert es.scaled_size(es.desc(100, 50, 2, 2, 3, cs, qts), 1)[0] == ERR_UNSUPPORTED


def test_prescale_plan_brute_force():
    """the per-image scale and the reduced window of the prescaled resize against their statements: every w in 1..4096 x
    out_w in {1, 224, 8192} x max_prescale"""
    W = 4096
    for out_w in (1, 224, 8192):
        for max_log2 in (0, 1, 2, 3):
            for w in range(1, W + 1):
                h = max(1, (w * 3) // 4)
                out_h = out_w
                # the largest power of two s <= 2^max with floor(w / s) >= out_w and floor(h / s) >= out_h, by trying all
                best = 0
                for k in range(0, max_log2 + 1):
                    if k == 0 or (w // (1 << k) >= out_w and h // (1 << k) >= out_h):
                        best = max(best, k)
                k = es.prescale_pick(w, h, out_w, out_h, max_log2)
                assert k == best == sm.prescale_log2(w, h, out_w, out_h, max_log2), (w, out_w, max_log2)
                if w % 7 and w > 64:
                    continue  # the window: a seventh of the widths, and all the small ones
                s = 1 << k
                for (x, y, H) in ((0, 0, 4096), (W - w, 4096 - h, 4096), ((W - w) // 2, 5, 4093)):
                    Wf = W - (3 if H == 4093 and x + w <= W - 3 else 0)
                    rx, ry, rw, rh = es.prescale_window(x, y, w, h, k, Wf, H)
                    assert (rx, ry, rw, rh) == sm.reduced_window(x, y, w, h, k, Wf, H)
                    fw, fh = -(-Wf // s), -(-H // s)
                    assert rw >= 1 and rh >= 1 and rx + rw <= fw and ry + rh <= fh          # inside the reduced frame
                    assert rx * s <= x and ry * s <= y                                      # covers the requested window
                    assert min((rx + rw) * s, Wf) >= x + w and min((ry + rh) * s, H) >= y + h
                    assert x - rx * s < s and (rx + rw) * s - (x + w) < s                  # by less than s per side
                    assert y - ry * s < s and (ry + rh) * s - (y + h) < s
                    if k:
                        assert rw >= out_w and rh >= out_h                                  # the resize never enlarges
