"""CPU: the frames of tests/guard_cases.py -- every arm of classify_block at its limit, the tile redo, tables per component --
through the emulations of the kernels that classify: the fused kernels in every variant (tests/emu), the crop, crop-tensor and
mixed-geometry crop kernels (tests/emu_crop, emu_crop_tensor, emu_crop_mixed) and the reduced decode of 4:2:0 at 1/2
(tests/emu_scaled), against the expectations test_gpu_guard.py uses on the device: the oracle's bytes, and
scaled_model.decode_scaled for the reduced decode.  emu_c.stats() must count the classes and the redone tiles that
guard_cases predicts from the coefficients alone."""
import numpy as np
import pytest

import emu_c
import emu_crop_c as ec
import emu_crop_mixed_c as em
import emu_crop_tensor_c as ect
import emu_scaled_c as es
import guard_cases as gc
import resize_model as rm
import scaled_model as sm
from test_gpu_crop_tensor import convert

CASES = [(name, mode) for name in gc.TABLE_NAMES for mode in gc.MODES]
CASE_IDS = [f"{n}-{m}" for n, m in CASES]


@pytest.fixture(autouse=True)
def _variant_zero():
    yield
    emu_c.set_variant(0)


def kinds_for(w):
    """a GRAYSCALE output of a width off the 16-pixel grid is a reference panic (zj_plan.h: make_plan)"""
    return [k for k in gc.KINDS if k != "gray" or w % 16 == 0]


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} values differ, first {bad[:4].tolist()}")


def test_cases_state_what_they_reach(capsys):
    with capsys.disabled():
        report = gc.assert_cases()
    assert len(report["tables"]) == 8 and len(report["mix"]) == 2 * len(gc.TABLE_NAMES) * sum(len(s) for s in gc.SHAPES.values())


def fused(name, mode, w, h, kind, flags, variant, seed=0):
    hs, vs = gc.MODES[mode]
    planes, qts = gc.frame(name, mode, w, h, seed)
    cs, _, dflags, layout = gc.kind_of(kind)
    emu_c.set_variant(variant)
    rc, out = emu_c.decode_planes(ec.desc(w, h, hs, vs, 3, cs, qts), planes, flags=flags | dflags, out_layout=layout)
    assert rc == 0, (name, mode, w, h, kind, flags, variant, rc)
    return out.reshape(3, h, w) if kind == "chw" else out.reshape(h, -1)


@pytest.mark.parametrize("name,mode", CASES, ids=CASE_IDS)
def test_fused_emulation_matches_oracle(name, mode):
    """every kind under every flag set in the packed generation; RGB under every variant as well, with the class counts and
    the redone tiles of the packed variants; the other kinds once more with direct stores"""
    for (w, h) in gc.SHAPES[mode]:
        for kind in kinds_for(w):
            if kind == "rgb":
                continue
            for flags in gc.FLAG_SETS:
                same(fused(name, mode, w, h, kind, flags, 0), gc.expected(name, mode, w, h, kind, flags), (name, mode, w, h, kind, flags))
            same(fused(name, mode, w, h, kind, 0, 2), gc.expected(name, mode, w, h, kind, 0), (name, mode, w, h, kind, "direct"))
        for flags in gc.FLAG_SETS:
            for variant in (0, 1, 2):
                for seed in ((0, 1) if flags == 0 and variant == 0 else (0,)):
                    same(fused(name, mode, w, h, "rgb", flags, variant, seed), gc.expected(name, mode, w, h, "rgb", flags, seed),
                         (name, mode, w, h, flags, variant, seed))
                    if variant != 1:
                        want = gc.predicted_stats(name, mode, w, h, seed)
                        if flags & gc.FLAG_CLAMP_DC:
                            want = want[:3] + (0,)           # a clamped shortcut value is a byte: nothing is redone
                        assert emu_c.stats() == want, (name, mode, w, h, flags, variant, emu_c.stats(), want)


@pytest.mark.parametrize("name,mode", CASES, ids=CASE_IDS)
def test_crop_emulation_matches_oracle(name, mode):
    hs, vs = gc.MODES[mode]
    for (w, h) in gc.SHAPES[mode]:
        planes, qts = gc.frame(name, mode, w, h)
        for kind in ("rgb", "gray", "chw"):
            if kind not in kinds_for(w):
                continue
            cs, _, _, layout = gc.kind_of(kind)
            d = ec.desc(w, h, hs, vs, 3, cs, qts, out_layout=layout)
            exp = gc.expected(name, mode, w, h, kind)
            for (x, y, ww, hh) in gc.windows(name, mode, w, h):
                rc, outs = ec.decode_crops(d, [planes], [(x, y)], ww, hh)
                assert rc == 0, (name, mode, w, h, kind, rc)
                got = outs[0].reshape(3, hh, ww) if kind == "chw" else outs[0].reshape(hh, -1)
                same(got, gc.crop_of(exp, kind, x, y, ww, hh), (name, mode, w, h, kind, (x, y, ww, hh)))


def crop_hwc(name, mode, w, h, kind, win, seed=0):
    """the oracle's crop as [1, h, w, C] uint8"""
    x, y, ww, hh = win
    exp = gc.crop_of(gc.expected(name, mode, w, h, kind, 0, seed), kind, x, y, ww, hh)
    return np.ascontiguousarray(exp).reshape(1, hh, ww, -1)


@pytest.mark.parametrize("name,mode", CASES, ids=CASE_IDS)
def test_crop_tensor_emulation_matches_oracle(name, mode):
    """u8 and f32 (scale 1, bias 0), NCHW and NHWC: the conversion of the oracle's crop"""
    hs, vs = gc.MODES[mode]
    for (w, h) in gc.SHAPES[mode]:
        planes, qts = gc.frame(name, mode, w, h)
        for kind in ("rgb", "gray"):
            if kind not in kinds_for(w):
                continue
            d = ec.desc(w, h, hs, vs, 3, gc.kind_of(kind)[0], qts)
            for i, win in enumerate(gc.windows(name, mode, w, h)):
                dtype, layout = [(rm.U8, "NCHW"), (rm.F32, "NHWC"), (rm.U8, "NHWC"), (rm.F32, "NCHW")][(i + (kind == "gray")) % 4]
                rc, got = ect.decode_crops_tensor(d, [planes], [win[:2]], win[2], win[3], dtype, layout)
                assert rc == 0, (name, mode, w, h, kind, win, rc)
                same(got, convert(crop_hwc(name, mode, w, h, kind, win), dtype, layout, None, None, None), (name, mode, w, h, kind, win, dtype, layout))


def mixed_frames(names=("q50", "cross", "flat16", "q10")):
    """the first shape of every mode, each under another table set: (name, mode, w, h, descriptor, planes)"""
    out = []
    for name, mode in zip(names, ("420", "444", "422", "440")):
        w, h = gc.SHAPES[mode][0]
        hs, vs = gc.MODES[mode]
        planes, qts = gc.frame(name, mode, w, h)
        out.append((name, mode, w, h, ec.desc(w, h, hs, vs, 3, 0, qts), planes))
    return out


@pytest.mark.parametrize("dtype,layout", [(rm.U8, "NHWC"), (rm.F32, "NCHW")])
def test_crop_tensor_mixed_emulation_matches_oracle(dtype, layout):
    """4:2:0 and 4:4:4 frames (and the two other modes) with different tables in one mixed call, one window size: inside a
    redone tile, inside one that is not, across their seam"""
    fr = mixed_frames()
    for pick in (1, 2, 3):
        wins = [gc.windows(n, m, w, h)[pick] for (n, m, w, h, _, _) in fr]
        ww, hh = min(v[2] for v in wins), min(v[3] for v in wins)
        rc, got = ect.decode_crops_tensor_mixed([f[4] for f in fr], [f[5] for f in fr], [v[:2] for v in wins], ww, hh, dtype, layout)
        assert rc == 0
        exp = np.concatenate([convert(crop_hwc(n, m, w, h, "rgb", (v[0], v[1], ww, hh)), dtype, layout, None, None, None)
                              for (n, m, w, h, _, _), v in zip(fr, wins)])
        same(got, exp, (pick, dtype, layout))


def test_crop_mixed_emulation_matches_oracle():
    """the mixed-geometry crop stage (zj_crop_mixed.hip's body) at scale 1: every window of every frame"""
    fr = mixed_frames()
    for pick in range(5):
        wins = [gc.windows(n, m, w, h)[pick] for (n, m, w, h, _, _) in fr]
        rc, outs, plan, _ = em.crops([f[4] for f in fr], [f[5] for f in fr], wins, 1, 1)
        assert rc == 0 and all(p[0] == 0 and tuple(p[1]) == tuple(v) for p, v in zip(plan, wins)), plan
        for (n, m, w, h, _, _), v, got in zip(fr, wins, outs):
            same(got.reshape(v[3], -1), gc.crop_of(gc.expected(n, m, w, h, "rgb"), "rgb", *v), (n, m, v))


SCALED_KINDS = {"rgb": (sm.RGB, 0), "ycbcr": (sm.YCBCR, 0), "chw": (sm.RGB, 1)}


def scaled_expect(name, w, h, sl, kind, seed=0):
    planes, qts = gc.frame(name, "420", w, h, seed)
    cs, layout = SCALED_KINDS[kind]
    return sm.decode_scaled(w, h, 2, 2, 3, cs, qts, planes, sl, chw=layout == 1)


@pytest.mark.parametrize("name", gc.TABLE_NAMES)
def test_scaled_emulation_matches_the_model(name):
    """4:2:0 at 1/2: the chroma blocks take the full transform behind classify_block (scaled_finish); at 1/4 nothing does"""
    for (w, h) in gc.SHAPES["420"]:
        planes, qts = gc.frame(name, "420", w, h)
        for kind, (cs, layout) in SCALED_KINDS.items():
            d = es.desc(w, h, 2, 2, 3, cs, qts, out_layout=layout)
            for sl in (1, 2):
                rc, outs = es.decode(d, [planes], sl)
                assert rc == 0
                exp = scaled_expect(name, w, h, sl, kind)
                same(outs[0].reshape(exp.shape), exp, (name, w, h, kind, sl))


def test_scaled_mixed_emulation_matches_the_model():
    """the mixed-geometry reduced path: 4:2:0 frames of two sizes and table sets at scale 1/2 in one group"""
    specs = [("cross", 528, 64), ("q50", 272, 48), ("flat1", 530, 64)]
    descs, planes, wins = [], [], []
    for (name, w, h) in specs:
        p, qts = gc.frame(name, "420", w, h)
        descs.append(ec.desc(w, h, 2, 2, 3, 0, qts))
        planes.append(p)
        wins.append((0, 0, w - w % 2, h))
    for (name, w, h), d, p, win in zip(specs, descs, planes, wins):
        rc, outs, plan, _ = em.crops([d], [p], [win], win[2] // 2, win[3] // 2, 1)
        assert rc == 0 and plan[0][0] == 1, plan
        x, y, ww, hh = plan[0][1]
        same(outs[0].reshape(hh, ww, 3), scaled_expect(name, w, h, 1, "rgb")[y:y + hh, x:x + ww], (name, w, h))
    rc, outs, plan, _ = em.crops(descs[:2], planes[:2], [(0, 0, 264, 48), (0, 0, 264, 48)], 132, 24, 1)
    assert rc == 0 and [p[0] for p in plan] == [1, 1]
    for (name, w, h), got in zip(specs[:2], outs):
        same(got.reshape(24, 132, 3), scaled_expect(name, w, h, 1, "rgb")[:24, :132], (name, "group"))
