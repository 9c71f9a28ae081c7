"""CPU: the byte formulation of the chroma up-sampling filters (Cfg::CBYTE, tri_b in zune-jpeg_amd/csrc/zj_device.h) in the
emulation build -- the filter by itself over every pair of bytes, and whole frames against the oracle at the smallest shapes
where the byte code can go wrong, with planted coefficient content (tests/chroma_bytes_cases.py)."""
import numpy as np
import pytest

import chroma_bytes_cases as cases
import emu_cbyte_c as emu
import oracle_c as oc


@pytest.fixture(autouse=True)
def _default_variant():
    yield
    emu.set_variant(0)


def test_byte_filter_equals_the_oracles_triangle_filter_for_every_pair_of_bytes():
    """tri_b(near, far) == (3 * near + far + 2) >> 2 for all 65 536 (near, far): both roundings of both averages occur"""
    near, far = [a.reshape(-1).astype(np.uint8) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij")]
    exp = ((3 * near.astype(np.int32) + far.astype(np.int32) + 2) >> 2).astype(np.uint8)
    assert np.array_equal(emu.tri_b(near, far), exp)
    # the same numbers from the oracle's own horizontal up-sampler (upsampler/scalar.rs:5-60): in a row ... far, near, far ...
    # both outputs of `near` are (3 * near + far + 2) >> 2
    n = near.size
    inp = np.empty((n, 3), np.int16)
    inp[:, 0], inp[:, 1], inp[:, 2] = far, near, far
    rc, up = oc.upsample_h(inp.reshape(-1), 6 * n)
    assert rc == 0
    up = up.reshape(n, 6)
    assert np.array_equal(up[:, 2], exp.astype(np.int16)) and np.array_equal(up[:, 3], exp.astype(np.int16))


@pytest.mark.parametrize("mode", list(cases.MODES))
@pytest.mark.parametrize("wh", cases.ALIGNED + cases.RAGGED)
def test_planted_blocks_are_in_the_input(mode, wh):
    cases.assert_planted(*wh, mode)


@pytest.mark.parametrize("mode", list(cases.MODES))
@pytest.mark.parametrize("kind", cases.OUT_KINDS)
@pytest.mark.parametrize("wh", cases.ALIGNED + cases.RAGGED)
def test_emulated_byte_chroma_matches_oracle(mode, kind, wh):
    """Whole frames: dense low-quality blocks (chroma saturating at 0 and 255), DC-only chroma inside 0..255, and DC-only
    chroma whose shortcut value is 256 / -1 in a block wave and in a halo column -- those tiles must take the redo, exactly
    those, and still equal the oracle.  Staged and direct stores; ZJ_FLAG_CLAMP_DC / ZJ_FLAG_EDGE_REPLICATE on and off."""
    w, h = wh
    hs, vs = cases.MODES[mode]
    planes, qts = cases.frame(w, h, mode)
    cases.assert_planted(w, h, mode)
    cs = {"rgb": oc.RGB, "ycbcr": oc.YCBCR, "rgba": oc.RGBA, "chw": oc.RGB}[kind]
    f = oc.make_frame(w, h, hs, vs, 3, cs, qts)
    for flags in cases.FLAG_SETS:
        exp = cases.expected(w, h, mode, kind, flags)
        for variant in (0, 2):
            emu.set_variant(variant)
            rc, out = emu.decode_planes(f, planes, flags=flags, out_layout=1 if kind == "chw" else 0)
            assert rc == 0, (mode, kind, wh, flags, variant, rc)
            tiles, redo, byte_tiles = emu.stats()
            assert tiles > 0 and byte_tiles == tiles, "this instantiation did not stage its chroma as bytes"
            # clamped, the planted values are bytes: nothing to redo; otherwise exactly the tiles that see a planted block
            want = 0 if flags & cases.FLAG_CLAMP_DC else len(cases.redo_tiles(w, h, hs, vs))
            assert redo == want, (mode, kind, wh, flags, variant, redo, want)
            bad = np.nonzero(out != exp)[0]
            assert bad.size == 0, (mode, kind, wh, flags, variant, bad.size, bad[:8])
