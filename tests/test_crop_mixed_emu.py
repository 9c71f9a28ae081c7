"""CPU: the mixed-geometry crop stage (zj_decode_crops_resized_mixed_device) -- the kernels' bodies run
over a table of per-frame records (tests/emu_crop_mixed), every frame's bytes against the emulated ONE-geometry kernel for
that frame alone (tests/emu_crop, tests/emu_scaled: zj_fused_crop_kernel + zj_crop_zero_kernel, zj_scaled_kernel), and the
argument rules of the planes entry point on the host."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import emu_crop_c as ec
import emu_crop_mixed_c as em
import emu_scaled_c as es

synth = importlib.import_module("zune-jpeg_amd.synth")

RGB, GRAY, YCBCR = 0, 1, 2
MODES = {"444": (1, 1), "422": (2, 1), "440": (1, 2), "420": (2, 2)}
ERR_ARG, ERR_UNSUPPORTED = -1, -2
CORRECTED = 7  # ZJ_FLAG_CORRECTED: CLAMP_DC | EDGE_REPLICATE | PLAIN_TAIL
OUT = (8, 8)   # the resize target the scale is picked against


def frame(w, h, mode, cs=RGB, layout=0, flags=0, seed=1, quality=90, in_comp=3):
    hs, vs = MODES[mode] if in_comp == 3 else (1, 1)
    assert cs != GRAY or w % 16 == 0, "grayscale widths off the MCU grid are ZJ_ERR_PANIC (zj_plan.h: make_plan)"
    planes, qts = synth.make_frame(w, h, hs, vs, in_comp, seed=seed, quality=quality)
    return ec.desc(w, h, hs, vs, in_comp, cs, qts, flags=flags, out_layout=layout), [np.array(p) for p in planes]


def single(d, planes, k, cwin):
    """frame alone through the emulated one-geometry kernels: the bytes of its tight crop"""
    x, y, w, h = cwin
    if k == 0:
        rc, outs = ec.decode_crops(d, [planes], [(x, y)], w, h)
    else:
        rc, outs = es.decode(d, [planes], k, [cwin])
    assert rc == 0, (rc, k, cwin)
    return outs[0]


def check_group(frames, windows, max_k=0, orientations=None, want_counts=None):
    descs = [f[0] for f in frames]
    rc, outs, plan, counts = em.crops(descs, [f[1] for f in frames], windows, OUT[0], OUT[1], max_k, orientations)
    assert rc == 0, rc
    for i, ((d, planes), (k, cwin, _), got) in enumerate(zip(frames, plan, outs)):
        exp = single(d, planes, k, cwin)
        assert got.size == exp.size and np.array_equal(got, exp), f"frame {i} ({d.width}x{d.height}, scale {k}, window {cwin})"
    if want_counts is not None:
        assert counts == want_counts, counts
    return plan, counts


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["rgb", "chw", "gray", "ycbcr"])
def test_one_launch_over_mixed_frames_equals_each_frame_alone(mode, kind):
    """frames of different width, height, tables, flags and windows in ONE emulated crop launch of a sampling mode"""
    cs, layout = {"rgb": (RGB, 0), "chw": (RGB, 1), "gray": (GRAY, 0), "ycbcr": (YCBCR, 0)}[kind]
    sizes = [(17, 9), (33, 40), (257, 16), (272, 24), (300, 72)] if kind == "rgb" else [(17, 9), (261, 40), (300, 33)]
    if kind == "gray":
        sizes = [(16, 9), (272, 40), (304, 33)]
    frames, windows = [], []
    for i, (w, h) in enumerate(sizes):
        frames.append(frame(w, h, mode, cs, layout, flags=CORRECTED if i % 2 else 0, seed=10 + i, quality=(50, 75, 90, 95, 30)[i]))
        windows.append([(0, 0, w, h), (w - 1, h - 1, 1, 1), (w // 3, h // 2, w - w // 3, h - h // 2), (0, 0, min(w, 8), min(h, 8)),
                        (w - min(w, 20), 0, min(w, 20), h)][i])
    _, counts = check_group(frames, windows)
    assert counts[0] == 1 and counts[1] == 0  # one crop launch for the mode, whatever the frames' sizes


def test_every_mode_in_one_group():
    """4:4:4, 4:2:2, 4:4:0 and 4:2:0 frames in one group: one crop launch per mode present, one zero launch"""
    frames = [frame(40 + 13 * i, 24 + 16 * (i % 3), m, flags=CORRECTED if i & 1 else 0, seed=30 + i, quality=40 + 10 * i)
              for i, m in enumerate(["420", "444", "422", "440", "420", "444"])]
    windows = [(0, 0, d.width, d.height) for d, _ in frames]
    _, counts = check_group(frames, windows)
    assert counts[0] == 4


def test_gray_frames_of_one_and_three_components():
    frames = [frame(48, 20, "444", GRAY, in_comp=1, seed=3), frame(32, 48, "420", GRAY, seed=4), frame(304, 16, "422", GRAY, seed=5)]
    check_group(frames, [(0, 0, 48, 20), (5, 7, 27, 40), (250, 1, 54, 15)])


@pytest.mark.parametrize("mode", ["420", "440"])
def test_rows_below_the_last_complete_strip_per_frame(mode):
    """heights 40 and 72 drop an MCU row or lie below rows_covered; 32 and 64 do not: each frame's zeros by its own
    rows_covered, in one zero launch"""
    frames = [frame(48, h, mode, seed=40 + h) for h in (40, 32, 72, 64)]
    windows = [(0, 0, 48, 40), (0, 0, 48, 32), (3, 60, 20, 12), (0, 50, 48, 14)]
    plan, counts = check_group(frames, windows)
    if mode == "420":  # (4:4:0 strips are one MCU row: none is dropped)
        assert counts[2] == 1
    d, planes = frames[0]
    got = em.crops([d], [planes], [windows[0]], *OUT)[1][0].reshape(40, -1)
    if mode == "420":
        assert (got[32:] == 0).all() and got[:32].any()


@pytest.mark.parametrize("kind", ["rgb", "chw", "gray"])
def test_every_scale_in_one_group(kind):
    """max_prescale_log2 3 with windows that land on scale 0, 1, 2 and 3: one reduced launch per (mode, scale) present"""
    cs, layout = {"rgb": (RGB, 0), "chw": (RGB, 1), "gray": (GRAY, 0)}[kind]
    frames, windows = [], []
    for i, (mode, w, h, win) in enumerate([("420", 100, 80, (0, 0, 12, 12)), ("420", 90, 70, (1, 3, 17, 30)), ("420", 130, 90, (7, 9, 40, 33)),
                                           ("420", 200, 150, (11, 5, 180, 140)), ("444", 70, 66, (3, 1, 65, 64)), ("422", 150, 40, (20, 4, 100, 35)),
                                           ("440", 64, 200, (0, 30, 64, 170)), ("420", 133, 77, (0, 0, 133, 77))]):
        if kind == "gray":
            w = (w + 15) // 16 * 16
        frames.append(frame(w, h, mode, cs, layout, flags=CORRECTED if i % 3 == 0 else 0, seed=60 + i, quality=35 + 8 * i))
        windows.append(win)
    plan, counts = check_group(frames, windows, max_k=3)
    ks = [p[0] for p in plan]
    assert set(ks) == {0, 1, 2, 3}, ks
    assert counts[1] == len({(f[0].h_max, f[0].v_max, k) for f, k in zip(frames, ks) if k})


def test_orientations_map_each_window_to_its_own_frame():
    frames = [frame(40 + 7 * o, 30 + 5 * o, "420" if o & 1 else "422", seed=80 + o) for o in range(1, 9)]
    windows = []
    for o, (d, _) in zip(range(1, 9), frames):
        dw, dh = (d.height, d.width) if o >= 5 else (d.width, d.height)
        windows.append((2, 3, dw - 5, dh - 4))
    plan, _ = check_group(frames, windows, orientations=list(range(1, 9)))
    zj = importlib.import_module("zune-jpeg_amd")
    if os.path.exists(zj.lib_path()):
        for o, (d, _), w, p in zip(range(1, 9), frames, windows, plan):
            assert tuple(zj.orient_window(o, d.width, d.height, w)) == p[1] and p[2] == o


def test_more_frames_than_a_scattered_launch_holds():
    """40 frames (ZJ_SCATTER_MAX is 32) in one launch"""
    frames = [frame(16 + (5 * i) % 48, 16 + (3 * i) % 32, "420", seed=100 + i) for i in range(40)]
    windows = [(i % 5, i % 3, d.width - i % 5, d.height - i % 3) for i, (d, _) in enumerate(frames)]
    _, counts = check_group(frames, windows)
    assert counts[0] == 1


def test_record_sizes_fit_the_table_alignment():
    assert em.lib().zjem_record_bytes(0) % 8 == 0 and em.lib().zjem_record_bytes(1) % 8 == 0
    assert em.lib().zjem_record_bytes(2) == 32


# ---- argument rules of the planes entry point, on the host ------------------------------------------------------------
def five():
    return [frame(40 + 8 * i, 32 + 8 * i, "420", seed=i)[0] for i in range(5)]


def test_mismatched_colorspace_or_layout_is_an_argument_error():
    descs = five()
    wins = [(0, 0, 8, 8)] * 5
    assert em.plan(descs, wins, *OUT)[0] == 0
    descs[2].out_colorspace = YCBCR
    assert em.plan(descs, wins, *OUT)[0] == ERR_ARG
    descs = five()
    descs[4].out_layout = 1
    assert em.plan(descs, wins, *OUT)[0] == ERR_ARG


def test_a_window_leaving_frame_3_of_5_is_an_argument_error_and_nothing_runs():
    descs = five()
    wins = [(0, 0, d.width, d.height) for d in descs]
    wins[3] = (1, 0, descs[3].width, descs[3].height)
    assert em.plan(descs, wins, *OUT)[0] == ERR_ARG
    planes = [frame(d.width, d.height, "420", seed=i)[1] for i, d in enumerate(descs)]
    rc, outs, _, _ = em.crops(descs, planes, wins, *OUT)
    assert rc == ERR_ARG and all((o == 0xAA).all() for o in outs)


def test_orientation_9_is_an_argument_error():
    descs = five()
    wins = [(0, 0, 8, 8)] * 5
    assert em.plan(descs, wins, *OUT, orientations=[1, 2, 3, 4, 5])[0] == 0
    assert em.plan(descs, wins, *OUT, orientations=[1, 2, 9, 4, 5])[0] == ERR_ARG
    assert em.plan(descs, wins, *OUT, orientations=[1, 2, 0, 4, 5])[0] == ERR_ARG


def test_the_first_failing_frames_status_is_returned():
    """frame 1 is unsupported (a single component asked for RGB), frame 3's window leaves it: the status is frame 1's"""
    descs = five()
    descs[1].in_components = 1
    descs[1].h_max = descs[1].v_max = 1
    wins = [(0, 0, 8, 8)] * 5
    wins[3] = (0, 0, 1000, 8)
    assert em.plan(descs, wins, *OUT)[0] == ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def zj():
    m = importlib.import_module("zune-jpeg_amd")
    if not os.path.exists(m.lib_path()):
        import __graft_entry__ as g
        g.build()
    return m


def test_library_entry_points_reject_bad_arguments_without_a_gpu(zj):
    """the exported calls with no context: ZJ_ERR_ARG before anything touches a device"""
    L = zj.lib()
    assert "zj_decode_crops_resized_mixed_device" in zj.abi_symbols()
    assert "zj_decoder_finish_pixels_resized_crop_batch_device" in zj.abi_symbols()
    qt = np.ones((3, 64), np.int32)
    descs = (zj.FrameDesc * 2)(zj.FrameDesc.make(64, 32, 2, 2, 3, zj.ColorSpace.RGB, list(qt)),
                               zj.FrameDesc.make(48, 40, 1, 1, 3, zj.ColorSpace.RGB, list(qt)))
    buf = np.zeros(64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    ptrs = (C.c_void_p * 2)(p, p)
    win = (C.c_uint * 8)(0, 0, 8, 8, 0, 0, 8, 8)
    sc = (C.c_float * 3)(1.0, 1.0, 1.0)
    ori = (C.c_uint8 * 2)(1, 1)
    for f in (0, 1, 4, 2, -1):
        assert L.zj_decode_crops_resized_mixed_device(None, descs, 2, ptrs, ptrs, ptrs, win, 4, 4, 2, 0, sc, sc, None, f, 0, ori,
                                                      p, None) == ERR_ARG
    rcs = (C.c_int * 2)()
    assert L.zj_decoder_finish_pixels_resized_crop_batch_device(None, 2, None, win, 4, 4, 2, 0, sc, sc, None, 0, 0, 0, p,
                                                                1 << 20, rcs) == ERR_ARG
