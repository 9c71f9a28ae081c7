"""CPU: crop-window decode (zj_decode_crops_device) -- the crop kernel's tile decode, staging and copy-out
and the crop plan, emulated thread by thread (tests/emu_crop), against the full-frame decode sliced with numpy: the
emulated full kernel (tests/emu, itself checked against the oracle by test_emu.py) and, for the reference's own
outputs, the oracle directly."""
import zlib

import numpy as np
import pytest

import emu_c
import emu_crop_c as ec
import oracle_c as oc

MODES = {"none": (1, 1), "h": (2, 1), "v": (1, 2), "hv": (2, 2)}
KINDS = {"rgb": (oc.RGB, 0), "gray": (oc.GRAYSCALE, 0), "ycbcr": (oc.YCBCR, 0), "rgba": (oc.RGBA, 0), "chw": (oc.RGB, 1)}
ERR_ARG = -1


def one_group_width(hs, vs, kind):
    """a width whose last tile column holds a single 16-pixel group (tile widths of zj_device.h: TileWidth)"""
    twy = {(1, 1): 512, (2, 1): 256, (1, 2): 256, (2, 2): 256}[(hs, vs)] if kind != "gray" else \
        {(1, 1): 1024, (2, 1): 1024, (1, 2): 1024, (2, 2): 512}[(hs, vs)]
    return twy + 16


def full_frame(d, planes, kind, flags):
    """the full decode as [H, row] (HWC) or [3, H, W] (CHW)"""
    f = oc.make_frame(d.width, d.height, d.h_max, d.v_max, 3, d.out_colorspace, [list(d.qt[c]) for c in range(3)])
    rc, out = emu_c.decode_planes(f, planes, flags=flags, out_layout=d.out_layout)
    if rc == 0 and flags == 0 and kind in ("rgb", "gray", "ycbcr"):
        rco, exp = oc.decode_planes(f, planes)
        assert rco == 0 and np.array_equal(out, exp), "emulated full decode != oracle"
    if rc:
        return rc, None
    if kind == "chw":
        return 0, out.reshape(3, d.height, d.width)
    return 0, out.reshape(d.height, -1)


def expect(full, kind, bpp, x, y, w, h):
    if kind == "chw":
        return full[:, y:y + h, x:x + w]
    return full[y:y + h, x * bpp:(x + w) * bpp]


def check_windows(d, planes, kind, flags, full, windows, out_pitch=0):
    """windows: list of (w, h, [origins]); every origin of one size in one call (frames of a scattered batch)"""
    ncomp = {oc.RGB: 3, oc.GRAYSCALE: 1, oc.YCBCR: 3, oc.RGBA: 4}[d.out_colorspace]
    bpp = 1 if kind == "chw" else ncomp
    for (w, h, origins) in windows:
        rc, outs = ec.decode_crops(d, [planes] * len(origins), origins, w, h, out_pitch=out_pitch)
        assert rc == 0, (w, h, origins, rc)
        pitch = out_pitch or w * bpp
        for (x, y), got in zip(origins, outs):
            rows = got.reshape(3, h, pitch) if kind == "chw" else got.reshape(h, pitch)
            body = rows[..., :w * bpp]
            exp = expect(full, kind, bpp, x, y, w, h)
            if not np.array_equal(body, exp):
                bad = np.argwhere(body != exp)
                raise AssertionError(f"{kind} {d.width}x{d.height} window {w}x{h} at ({x},{y}): {len(bad)} bytes differ, first {bad[:4].tolist()}")
            assert (rows[..., w * bpp:] == 0xAA).all(), "pitch padding written"


def windows_for(W, H, hs, rng, rows_covered):
    wins = [(W, H, [(0, 0)]),
            (1, 1, [(0, 0), (W - 1, H - 1), (int(rng.integers(W)), int(rng.integers(H)))]),
            # right edge inside the row's last 64 bytes (the early RGB tail, Q5)
            (min(W, 5), min(H, 3), [(W - min(W, 5), 0), (W - min(W, 5), H - min(H, 3))]),
            (min(W, 21), min(H, 7), [(W - min(W, 21), int(rng.integers(H - min(H, 7) + 1)))])]
    # windows that start and end mid-tile and mid-strip
    w, h = max(1, W // 3 + 1), max(1, H // 2 + 1)
    wins.append((w, h, [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for _ in range(4)]))
    w2 = max(1, min(W, 300))
    wins.append((w2, min(H, 9), [(int(rng.integers(W - w2 + 1)), int(rng.integers(H - min(H, 9) + 1))) for _ in range(3)]))
    if rows_covered < H:  # wholly below the last complete strip: zeros (Q6)
        wins.append((min(W, 17), H - rows_covered, [(0, rows_covered), (W - min(W, 17), rows_covered)]))
    return wins


def rows_covered_of(W, H, hs, vs):
    mcu_y = -(-H // (8 * vs))
    sh = {(1, 1): 8, (2, 1): 16, (1, 2): 16, (2, 2): 32}[(hs, vs)]
    return (mcu_y // 2 if hs == 2 else mcu_y) * sh


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("flags", [0, 7])
def test_crop_equals_sliced_full_decode(mode, kind, flags, synth):
    hs, vs = MODES[mode]
    out_cs, layout = KINDS[kind]
    rng = np.random.default_rng(zlib.crc32(f"{mode}-{kind}-{flags}".encode()))
    sizes = [(64, 40), (one_group_width(hs, vs, kind), 40), (2500, 40), (4090, 17), (13, 9), (100, 33)]
    for (W, H) in sizes:
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
        d = ec.desc(W, H, hs, vs, 3, out_cs, qts, flags=flags, out_layout=layout)
        rc, full = full_frame(d, planes, kind, flags)
        if rc:  # (a reference panic: the crop reports the plan's error too)
            assert ec.decode_crops(d, [planes], [(0, 0)], 1, 1)[0] == rc
            continue
        check_windows(d, planes, kind, flags, full, windows_for(W, H, hs, rng, rows_covered_of(W, H, hs, vs)))


@pytest.mark.parametrize("kind", list(KINDS))
def test_crop_wide_pitch_keeps_padding(kind, synth):
    """out_pitch wider than the crop's row: the rows land at the pitch, the poisoned padding between them survives"""
    out_cs, layout = KINDS[kind]
    for (W, H, hs, vs) in [(2500, 40, 2, 2), (272, 33, 2, 1), (13, 9, 1, 1)]:
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=3)
        d = ec.desc(W, H, hs, vs, 3, out_cs, qts, out_layout=layout)
        rc, full = full_frame(d, planes, kind, 0)
        if rc:
            continue
        w, h = min(W, 37), min(H, 11)
        ncomp = {oc.RGB: 3, oc.GRAYSCALE: 1, oc.YCBCR: 3, oc.RGBA: 4}[out_cs]
        pitch = (w * (1 if kind == "chw" else ncomp) + 127) // 128 * 128 + 3
        check_windows(d, planes, kind, 0, full, [(w, h, [(0, 0), (W - w, H - h), (W // 2 - w // 2, (H - h) // 2)])], out_pitch=pitch)


def test_crop_adversarial_frames_redo_wide(synth):
    """frames whose DC-only blocks decode outside a byte (Q1) make the crop kernel redo tiles with the wide code"""
    for (W, H, hs, vs) in [(100, 40, 2, 2), (528, 16, 1, 1)]:
        planes, qts = synth.make_adversarial_frame(W, H, hs, vs, 3, seed=99)
        for kind in ("rgb", "chw", "rgba"):
            out_cs, layout = KINDS[kind]
            d = ec.desc(W, H, hs, vs, 3, out_cs, qts, out_layout=layout)
            rc, full = full_frame(d, planes, kind, 0)
            assert rc == 0
            check_windows(d, planes, kind, 0, full, [(W, H, [(0, 0)]), (W // 2, H // 2, [(3, 5), (W // 2, H // 2)])])


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mode", list(MODES))
def test_plan_columns_equal_brute_force_writers(kind, mode, synth):
    """the plan's tile columns of a window == the columns that write a byte inside it, from the full-frame write map;
    every byte of a row has exactly one writer, and the plan's owned ranges are exactly those writers' bytes"""
    hs, vs = MODES[mode]
    out_cs, layout = KINDS[kind]
    rng = np.random.default_rng(11)
    for W in (64, one_group_width(hs, vs, kind), one_group_width(hs, vs, kind) - 8, 2500, 4090, 13, 520, 1032):
        planes, qts = synth.make_frame(W, 16 * vs, hs, vs, 3, seed=1)
        d = ec.desc(W, 16 * vs, hs, vs, 3, out_cs, qts, out_layout=layout)
        ntiles, owner = ec.row_owners(d, planes)
        if ntiles < 0:
            continue
        assert (owner >= 0).all(), (W, np.nonzero(owner < 0)[0][:8])
        bpp = len(owner) // W
        rc, _, own = ec.crop_window(d, 0, 0, W, 1)
        assert rc == ntiles and own[0] == 0 and own[-1] == len(owner)
        for k in range(ntiles):
            assert (owner[own[k]:own[k + 1]] == k).all(), (W, k)
        for _ in range(40):
            w = int(rng.integers(1, W + 1))
            x = int(rng.integers(0, W - w + 1))
            rc, (s0, s1, k0, k1), _ = ec.crop_window(d, x, 0, w, 1)
            brute = sorted(set(owner[x * bpp:(x + w) * bpp].tolist()))
            assert list(range(k0, k1)) == brute, (W, x, w, k0, k1, brute)


def test_strip_range(synth):
    planes, qts = synth.make_frame(64, 200, 2, 2, 3, seed=1)
    d = ec.desc(64, 200, 2, 2, 3, oc.RGB, qts)
    # 4:2:0: 32-row strips, mcu_y = 13 -> 6 strips (the odd MCU row is dropped: rows 192..199 stay 0)
    assert ec.crop_window(d, 0, 0, 64, 200)[1][:2] == (0, 6)
    assert ec.crop_window(d, 0, 31, 8, 2)[1][:2] == (0, 2)
    assert ec.crop_window(d, 0, 32, 8, 32)[1][:2] == (1, 2)
    assert ec.crop_window(d, 0, 192, 8, 8)[1][:2] == (6, 6)


def test_crop_out_len_and_argument_errors(synth):
    planes, qts = synth.make_frame(100, 40, 2, 2, 3, seed=1)
    d = ec.desc(100, 40, 2, 2, 3, oc.RGB, qts)
    assert ec.crop_out_len(d, 10, 4) == 120
    assert ec.crop_out_len(d, 10, 4, 64) == 256
    assert ec.crop_out_len(d, 100, 40) == 12000
    assert ec.crop_out_len(d, 10, 4, 29) == 0       # pitch below the row
    assert ec.crop_out_len(d, 0, 4) == 0 and ec.crop_out_len(d, 4, 0) == 0
    assert ec.crop_out_len(d, 101, 4) == 0 and ec.crop_out_len(d, 4, 41) == 0
    dc = ec.desc(100, 40, 2, 2, 3, oc.RGB, qts, out_layout=1)
    assert ec.crop_out_len(dc, 10, 4) == 120 and ec.crop_out_len(dc, 10, 4, 16) == 3 * 16 * 4
    dg = ec.desc(100, 40, 1, 1, 3, oc.GRAYSCALE, qts)
    assert ec.crop_out_len(dg, 10, 4) == 40
    da = ec.desc(100, 40, 2, 2, 3, oc.RGBA, qts)
    assert ec.crop_out_len(da, 10, 4) == 160
    dp = ec.desc(100, 40, 2, 2, 3, oc.RGB, qts)
    dp.out_pitch = 384
    assert ec.crop_out_len(dp, 10, 4) == 0           # the frame's own pitch must be 0
    assert ec.decode_crops(dp, [planes], [(0, 0)], 10, 4)[0] == ERR_ARG
    for (x, y, w, h, pitch) in [(91, 0, 10, 4, 0), (0, 37, 10, 4, 0), (0, 0, 0, 4, 0), (0, 0, 4, 0, 0), (0, 0, 10, 4, 29)]:
        assert ec.decode_crops(d, [planes], [(x, y)], w, h, out_pitch=pitch)[0] == ERR_ARG, (x, y, w, h, pitch)
    # one bad window of a batch: nothing is written at all
    rc, outs = ec.decode_crops(d, [planes, planes], [(0, 0), (95, 0)], 10, 4)
    assert rc == ERR_ARG and all((o == 0xAA).all() for o in outs)


def test_scattered_batches_cross_launch_splits(synth):
    """more frames than one launch carries (32): every frame its own planes and origin"""
    W, H = 272, 40
    frames = [synth.make_frame(W, H, 2, 2, 3, seed=5, frame_index=i)[0] for i in range(33)]
    qts = synth.make_frame(W, H, 2, 2, 3, seed=5)[1]
    d = ec.desc(W, H, 2, 2, 3, oc.RGB, qts)
    rng = np.random.default_rng(5)
    w, h = 40, 12
    origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for _ in frames]
    rc, outs = ec.decode_crops(d, frames, origins, w, h)
    assert rc == 0
    for i, ((x, y), got) in enumerate(zip(origins, outs)):
        _, full = full_frame(d, frames[i], "rgb", 0)
        assert np.array_equal(got.reshape(h, 3 * w), expect(full, "rgb", 3, x, y, w, h)), i


def test_crop_out_len_of_an_all_zero_output(synth):
    """a single-component frame asked for a colour output is all zeros (worker.rs:131) of zj_out_len's size: its crops
    are sized the same way, by the output's components (RGBA / RGBX 4, RGB 3, CHW RGB 3 planes), not refused"""
    import importlib
    import ctypes as C
    zj = importlib.import_module("zune-jpeg_amd")
    _, qts = synth.make_frame(64, 40, 1, 1, 1, seed=1)
    for cs, layout, per_px, planes in [(zj.ColorSpace.RGBA, 0, 4, 1), (zj.ColorSpace.RGBX, 0, 4, 1), (zj.ColorSpace.RGB, 0, 3, 1),
                                       (zj.ColorSpace.RGB, 1, 1, 3), (zj.ColorSpace.YCbCr, 0, 3, 1)]:
        d = zj.FrameDesc.make(100, 40, 1, 1, 1, cs, qts, out_layout=layout)
        assert zj.lib().zj_out_len(C.byref(d)) == 100 * 40 * per_px * planes
        assert zj.crop_out_len(d, 10, 4) == 10 * 4 * per_px * planes, (cs, layout)
        assert zj.crop_out_len(d, 10, 4, 64) == 64 * 4 * planes
        assert zj.crop_out_len(d, 101, 4) == 0 and zj.crop_out_len(d, 10, 4, 10 * per_px - 1) == 0
    dg = zj.FrameDesc.make(100, 40, 1, 1, 1, zj.ColorSpace.GRAYSCALE, qts)
    assert zj.crop_out_len(dg, 10, 4) == 40


# ---- ownership at every row-end width ---------------------------------------------------------------------------------
# The early RGB tail (Q5, zj_device.h: store_unit_generic) writes the row's last two 8-pixel units at p' = position - diff.
# Where 3W - position is 1..15 the tail ends BEFORE position, and the bytes [p' + 48, position) between them belong to the
# column of the ordinary unit they lie in: with 4:2:2 / 4:2:0 and the tail starting on a column boundary (W = 1..5 mod 256,
# W > 256) that is the PREVIOUS column, which then owns two pieces of the row.

def tail_geometry(W, hs):
    """(p', position) of an RGB row of width W (store_unit_generic)"""
    P = -(-W // (8 * hs)) * 8 * hs
    position = 48 * max(P // 16 - 1, 0)
    diff = max(64 - (3 * W - position), 0)
    return (position - diff if position > diff else 0), position


def tile_width(hs, vs, kind):
    return one_group_width(hs, vs, kind) - 16


def zero_planes(W, H, hs, vs):
    """all-zero coefficients: which bytes a column writes does not depend on the pixels"""
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    return [np.zeros(mx * my * 64 * hs * vs, np.int16), np.zeros(mx * my * 64, np.int16), np.zeros(mx * my * 64, np.int16)]


def sweep_widths():
    """every width up to 1100; the row ends at each tile width T: W = kT + r, r in 0..17 and T-17..T-1, up to ~16400 for
    T = 512 and 1024, up to ~4400 for T = 256 (beyond that its even k are T = 512's and its odd k differ from them only in
    the row's end: r = 0..6 there, where the tail starts on a column boundary); the same at the last column below 65535"""
    ws = set(range(1, 1101))
    for T, top in ((256, 4400), (512, 16400), (1024, 16400)):
        for k in range(1, top // T + 1):
            ws.update(k * T + r for r in list(range(18)) + list(range(T - 17, T)))
    ws.update(k * 256 + r for k in range(1, 16400 // 256 + 1) for r in range(7))
    ws.update([65280 + r for r in range(18)] + list(range(65519, 65536)))
    return sorted(ws)


SWEEP_FLAGS = [0, 1, 6, 7]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_plan_owner_of_every_byte_equals_brute_force_writer(kind, mode, synth):
    """every byte of a row has exactly one writer, and the crop plan's owner of it is that writer, at every width of
    sweep_widths().  Rows wider than 1100 pixels are examined from their last two columns on (their first columns are
    those of the narrower rows).  RGB HWC, whose row end depends on ZJ_FLAG_PLAIN_TAIL, runs every width with and without
    it: flags 0 and 1, or 6 and 7, in turn; the other kinds, whose writes the flags do not move, take one of 0, 1, 6, 7."""
    hs, vs = MODES[mode]
    out_cs, layout = KINDS[kind]
    _, qts = synth.make_frame(16, 16, 1, 1, 3, seed=1)
    H = 16 * vs
    descs = {f: ec.desc(16, H, hs, vs, 3, out_cs, qts, flags=f, out_layout=layout) for f in SWEEP_FLAGS}
    bad = []
    for i, W in enumerate(sweep_widths()):
        planes = zero_planes(W, H, hs, vs)
        for flags in (SWEEP_FLAGS[2 * (i % 2):2 * (i % 2) + 2] if kind == "rgb" else [SWEEP_FLAGS[i % 4]]):
            d = descs[flags]
            d.width = W
            ntiles, plan = ec.plan_owners(d)
            k_lo = max(ntiles - 2, 0) if W > 1100 else 0
            nt, brute = ec.row_owners(d, planes, k_lo)
            assert nt == ntiles, (W, flags, nt, ntiles)  # (both refuse a frame the reference panics on, ZJ_ERR_PANIC)
            if nt < 0:
                continue
            seen = brute != -3
            assert seen.sum() == len(brute) - k_lo * tile_width(hs, vs, kind) * (len(brute) // W), (W, k_lo)
            assert (brute[seen] >= 0).all(), (W, flags, "bytes with no writer or two", np.nonzero(seen & (brute < 0))[0][:8])
            if not np.array_equal(plan[seen], brute[seen]):
                b = np.nonzero(seen & (plan != brute))[0]
                bad.append((W, flags, len(b), int(b[0]), int(plan[b[0]]), int(brute[b[0]])))
    assert not bad, f"{len(bad)} (width, flags) where the plan's owner != the writer: (W, flags, bytes, first, plan, writer) {bad[:12]}"


def affected_widths():
    return [k * 256 + r for k in (1, 2, 3) for r in range(1, 6)] + [1029, 1281, 2053, 4101, 65281, 65285]


@pytest.mark.parametrize("mode", ["h", "hv"])
@pytest.mark.parametrize("flags", [0, 6, 1])
def test_window_columns_equal_brute_force_writers_at_the_tail(mode, flags, synth):
    """crop_window's [k0, k1) == the columns that write a byte of the window, for windows at the row's end of the widths
    whose tail starts on a column boundary: random ones, windows wholly inside [p' + 48, position) (only the previous
    column writes them), and windows that start or end at p' - 1, p', p' + 48, position and the row's last byte"""
    hs, vs = MODES[mode]
    _, qts = synth.make_frame(16, 16, 1, 1, 3, seed=1)
    rng = np.random.default_rng(flags + 10 * hs * vs)
    for W in affected_widths():
        d = ec.desc(W, 16 * vs, hs, vs, 3, oc.RGB, qts, flags=flags)
        ntiles = ec.plan_owners(d)[0]
        k_lo = max(ntiles - 3, 0)
        nt, owner = ec.row_owners(d, zero_planes(W, 16 * vs, hs, vs), k_lo)
        assert nt == ntiles and (owner[owner != -3] >= 0).all()
        pp, position = tail_geometry(W, hs)
        x_lo = 3 * tile_width(hs, vs, "rgb") * k_lo // 3 + 1  # windows right of the bytes not examined
        wins = []
        for _ in range(40):
            x = int(rng.integers(x_lo, W))
            wins.append((x, int(rng.integers(1, W - x + 1))))
        hole = [x for x in range(x_lo, W) if pp + 48 <= 3 * x and 3 * x + 3 <= position]
        if flags == 0 or flags == 6:
            assert len(hole) == (position - pp - 48) // 3, (W, pp, position)
        wins += [(x, n) for x in hole for n in range(1, len(hole) + 1) if x + n - 1 <= hole[-1]]
        for b in (pp - 1, pp, pp + 48, position, 3 * W - 1):
            q = min(max(b // 3, x_lo), W - 1)
            wins += [(q, W - q), (q, 1), (q, min(W - q, 16)), (x_lo, q - x_lo + 1), (max(q - 15, x_lo), min(q, 15) + 1)]
        for (x, w) in wins:
            rc, (s0, s1, k0, k1), _ = ec.crop_window(d, x, 0, w, 1)
            assert rc == ntiles
            brute = sorted(set(owner[3 * x:3 * (x + w)].tolist()))
            assert list(range(k0, k1)) == brute, (W, flags, x, w, k0, k1, brute, pp, position)


@pytest.mark.parametrize("W", [256, 257, 258, 261, 262, 513, 517, 1029, 1281, 2053, 4101])
@pytest.mark.parametrize("mode", ["h", "hv"])
def test_crop_at_the_tail_widths_equals_sliced_full_decode(W, mode, synth):
    """the emulated crop (over poisoned staging: a byte the copy-out takes from a column that never wrote it shows) == the
    sliced full decode, at the widths whose tail starts on a column boundary and their unaffected neighbours: the whole
    frame, every right-aligned window 1 to 48 pixels wide, windows that start or end at p' - 1, p', p' + 48, position and
    the row's last byte, and a batch of origins"""
    hs, vs = MODES[mode]
    H = 16 * vs
    planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W)
    pp, position = tail_geometry(W, hs)
    rng = np.random.default_rng(W * hs * vs)
    for kind in ("rgb", "rgba", "chw"):
        out_cs, layout = KINDS[kind]
        for flags in (0, 6, 7):
            d = ec.desc(W, H, hs, vs, 3, out_cs, qts, flags=flags, out_layout=layout)
            rc, full = full_frame(d, planes, kind, flags)
            assert rc == 0
            wins = [(W, H, [(0, 0)])]
            wins += [(w, H, [(W - w, 0)]) for w in range(1, min(W, 48) + 1)]
            for b in (pp - 1, pp, pp + 48, position, 3 * W - 1):
                q = min(max(b // 3, 0), W - 1)
                wins += [(W - q, H, [(q, 0)]), (q + 1, H, [(0, 0)]), (min(W - q, 20), 3, [(q, 5)]), (min(q + 1, 20), 2, [(max(q - 19, 0), 7)])]
            w = 40
            wins.append((w, H // 2, [(W - w, 0), (W - w - 1, H // 2), (W - w - 5, 3)] +
                         [(int(rng.integers(W - w + 1)), int(rng.integers(H // 2 + 1))) for _ in range(5)]))
            check_windows(d, planes, kind, flags, full, wins)
