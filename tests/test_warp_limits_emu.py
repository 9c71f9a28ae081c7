"""CPU: the affine warp's position arithmetic at its matrix limits (tests/warp_limit_cases.py; zune-jpeg_amd/csrc/zj_warp.h and
zj_warp_fixed.h).  What the cases reach and which wrong variants of the arithmetic they catch is asserted first,
from numpy and Python integers alone.  Then every case goes through the kernels' lanes (tests/emu_warp) with the checks of
test_warp_emu.run_call -- every tensor byte stored once, no store outside the tensor, no load outside an image's rows, the
model's bits -- and the host's rules (the six integers, the source window) are compared with their Python-integer
restatements."""
import numpy as np
import pytest

import emu_warp_c as ew
import warp_limit_cases as wl
import warp_model as wm
from test_warp_emu import run_call

NAMES = wl.names()


def test_the_cases_reach_what_they_claim():
    rep = wl.assert_cases()
    assert rep["cases"] == len(NAMES) and rep["surviving mutants"] == 0


@pytest.mark.parametrize("mutant", list(wl.MUTANTS))
def test_every_wrong_variant_is_caught_by_a_named_case(mutant):
    caught, alive = wl.surviving_mutants()
    for edge in wl.MUTANTS[mutant][1]:
        assert (mutant, edge) not in alive and caught[(mutant, edge)] in NAMES, (mutant, edge)
        c = wl.by_name(caught[(mutant, edge)])
        assert not np.array_equal(wl.values(c, edge, wl.MUTANTS[mutant][0]), wl.values(c, edge))


@pytest.mark.parametrize("name", NAMES)
def test_the_lanes_equal_the_model(name):
    c = wl.by_name(name)
    k = NAMES.index(name)
    combos, pad, base = wl.rotation(k)
    rng = np.random.default_rng(k)
    for edge in c["edges"]:
        for j, (dtype, layout) in enumerate(combos):
            run_call(rng, [c["src"]], [c["m"]], c["ch"], *c["out"], dtype, layout, (base + j) % 8, [(k + j) % 4], [pad], edge,
                     wl.FILLS[(k + j) % 2])


def test_the_rotation_covers_every_dtype_layout_pad_and_base():
    seen = [wl.rotation(k) for k in range(len(NAMES))]
    assert {cb for r in seen for cb in r[0]} == {(d, l) for d in range(4) for l in ("NCHW", "NHWC")}
    assert {r[1] for r in seen} == {0, 1, 13} and {r[2] for r in seen} == set(range(8))


@pytest.mark.parametrize("ch", [1, 3])
def test_a_second_launch_packs_the_limit_matrices(ch):
    """49 images, one more than a launch holds, the limit matrices in turn"""
    import resize_model as rm
    n = ew.batch() + 1
    ms = wl.cycle_matrices()
    assert n == 49 and len(ms) >= 12
    sources = [[(1, 1), (2, 1), (5, 3), (7, 5), (258, 3)][i % 5] for i in range(n)]
    rng = np.random.default_rng(490 + ch)
    for (dtype, layout, edge) in ((rm.F32, "NHWC", wm.REPLICATE), (rm.U8, "NCHW", wm.FILL)):
        run_call(rng, sources, ms, ch, 65, 33, dtype, layout, 3, [0, 1, 2, 3], [0, 1, 13], edge, wl.FILLS[1])


@pytest.mark.parametrize("frame", [(96, 80), (48, 64)])
def test_the_frame_matrices_have_the_windows_they_claim(frame):
    """the matrices of the GPU test's plane and file calls: a few pixels, the whole frame, nothing (FILL) or one corner, edge
    column or edge row (REPLICATE); the library's window is the restatement's"""
    wl.assert_frame_cases(*frame)
    for name, (ow, oh), m, _ in wl.frame_cases(*frame):
        q = ew.fixed(m)
        assert q == wl.fixed_ints(m), name
        for edge in wl.BOTH:
            win, sh = wl.window_ints(q, *frame, ow, oh, edge)
            assert ew.window(q, *frame, ow, oh, edge) == (win, sh), (name, edge)
            # what the plane and file calls rely on: the window's crop under the shifted integers is the frame under the matrix's
            img = np.random.default_rng(len(name)).integers(0, 256, (frame[1], frame[0], 3), dtype=np.uint8)
            whole = wm.values(img, q, ow, oh, edge, wl.FILLS[1])
            if win[2] == 0:
                assert edge == wm.FILL and bool((whole == np.array(wl.FILLS[1])[:, None, None] << 16).all()), name
            else:
                crop = img[win[1]:win[1] + win[3], win[0]:win[0] + win[2]]
                assert np.array_equal(wm.values(crop, sh, ow, oh, edge, wl.FILLS[1]), whole), (name, edge)


def test_the_integers_are_the_models():
    for c in wl.cases():
        assert ew.fixed(c["m"]) == wm.fixed(c["m"]) == list(c["ints"]), c["name"]
    # the refusals the definition promises, at the first double it refuses
    for bad in ((128.0, 0, 0, 0, 1, 0), (1, -128.0, 0, 0, 1, 0), (1, 0, 2.0 ** 31, 0, 1, 0), (1, 0, 0, 0, 1, -2.0 ** 31)):
        assert ew.fixed(bad) is None and wm.fixed(bad) is None


@pytest.mark.parametrize("group", sorted({n.split("/")[0] for n in NAMES}))
def test_the_window_is_the_models_and_holds_every_tap(group):
    """emu_warp_c.window == warp_model.source_window == the Python-integer restatement for frames 96 x 80, 1 x 1 and
    65535 x 65535 in both edge modes; wl.windows checks the shifted integers' bound and, by brute force over the case's output
    pixels, that every tap inside the frame (FILL) and every clamped tap (REPLICATE) lies in the window"""
    for c in wl.cases():
        if c["group"] != group:
            continue
        for (fw, fh), edge, win, sh in wl.windows(c):
            assert ew.window(c["ints"], fw, fh, *c["out"], edge) == (win, sh), (c["name"], fw, fh, edge)
            assert wm.source_window(list(c["ints"]), fw, fh, *c["out"], edge) == (win, sh), (c["name"], fw, fh, edge)
