"""CPU: the interior form of the fused kernel's colour rounds (Cfg::INTERIOR, interior_tile in zune-jpeg_amd/csrc/zj_device.h)
in the emulation build, with the knob on and off (-DZJ_INTERIOR=1 / 0): whole frames byte for byte against the oracle at
the smallest shapes where the form can go wrong (tests/interior_cases.py), and for every tile which rounds it ran, against
the predicate stated on its own."""
import numpy as np
import pytest

import emu_interior_c as emu
import interior_cases as cases
import oracle_c as oc


def test_predicate_on_the_shapes_of_the_cases():
    """what the cases are there for, before anything is decoded"""
    def admitted(name):
        _, mode, w, h, flags, _, _ = cases.CASES[cases.CASE_IDS.index(name)]
        tiles, strips, _ = cases.geometry(w, h, mode)
        return {(s, t) for s in range(strips) for t in range(tiles) if cases.interior(w, h, mode, flags, s, t)}
    assert admitted("768x64") == {(0, 1), (1, 1)}
    assert admitted("512x64") == set()
    assert admitted("768x48") == {(0, 1)}               # (the cut second strip is not even launched)
    assert admitted("768x56") == {(0, 1)}               # the clipped second strip is launched, and is out
    assert cases.geometry(768, 48, "hv")[1] == 1 and cases.geometry(768, 56, "hv")[1] == 2
    assert admitted("752x64") == {(0, 1), (1, 1)}
    assert admitted("1024x32-edge-rep") == set()
    assert admitted("1024x32") == {(0, 1), (0, 2)}
    assert admitted("768x32-422") == set()              # 256 items on 192 threads: the second round is not full


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_emulated_interior_rounds_match_oracle(case, kind):
    name, mode, w, h, flags, padded, plant = case
    hs, vs = cases.MODES[mode]
    planes, qts = cases.frame(w, h, mode, plant)
    exp = cases.expected(w, h, mode, kind, flags, plant)
    f = oc.make_frame(w, h, hs, vs, 3, cases.colorspace(kind), qts)
    tiles, strips, _ = cases.geometry(w, h, mode)
    redo = cases.redo_tiles(w, h, mode, plant)
    pitch = cases.out_pitch(w, kind) if padded else 0
    row = exp.shape[1]
    for knob in (1, 0):
        rc, out, ways = emu.decode_planes(knob, f, planes, flags=cases.desc_flags(kind, flags), out_pitch=pitch)
        assert rc == 0, (name, kind, knob, rc)
        # which rounds every tile ran
        assert set(ways) == {(s, t) for s in range(strips) for t in range(tiles)}
        for (s, t), way in sorted(ways.items()):
            if (s, t) in redo:
                want = emu.REDO      # the branch to the interior rounds comes after the redo test: the wide code does the tile
            elif knob and cases.interior(w, h, mode, flags, s, t):
                want = emu.INTERIOR
            else:
                want = emu.GENERAL
            assert way == want, (name, kind, knob, s, t, way, want)
        if plant is not None:
            assert any(cases.interior(w, h, mode, flags, s, t) for (s, t) in redo), "the redone tile is one the predicate admits"
        # the bytes
        bad = np.argwhere(out[:, :row] != exp)
        assert bad.size == 0, (name, kind, knob, len(bad), bad[:8].tolist())
        assert (out[:, row:] == 0xAA).all(), (name, kind, knob, "the padding of a row was written")
