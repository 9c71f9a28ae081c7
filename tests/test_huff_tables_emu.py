"""CPU: the device Huffman stage (zune-jpeg_amd/csrc/zj_huff_device.h, run thread by thread by tests/emu) and the table
the host builds for it (zj_jpeg.cpp gpu_table / prepare_scan) over the code-table shapes of tests/huff_table_cases.py.

Yardsticks: the planes handed to the encoder are the truth wherever oracle/ref_walk.py -- the line-by-line model of the
reference's reader -- returns them without a short read; where it does not (symbols the reference reads its own way, an
interval it does not close) its planes are.  The CPU walker, the emulated device stage and (tests/test_gpu_huff_tables.py)
the GPU must equal that truth; a scan the device hands back must carry the status bit its group expects (long DC symbols:
the device may also keep the scan -- then with the truth's planes).  In the groups
deep, straddle (but its LEFT_OVER case), budget, three and minimal NO case may be handed back: a handed-back case reaches
the right pixels through the CPU walker and says nothing about the device."""
import importlib
import os

import numpy as np
import pytest

import emu_c
import huff_table_cases as H


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


def options(zj, c, entropy=None):
    o = zj.ZuneJpegOptions()
    o.flags = c.flags
    if entropy is not None:
        o.entropy = entropy
    return o


def prepared(zj, c, sub):
    """the blob prepare_scan leaves under ENTROPY_GPU_ALWAYS at sub-sequences of `sub` bytes, or None"""
    old = os.environ.get("ZJ_HUFF_SUB")
    os.environ["ZJ_HUFF_SUB"] = str(sub)
    try:
        d = zj.Decoder(options(zj, c, zj.ENTROPY_GPU_ALWAYS))
    finally:
        if old is None:
            del os.environ["ZJ_HUFF_SUB"]
        else:
            os.environ["ZJ_HUFF_SUB"] = old
    d.prepare(c.data)
    return d.scan_blob()


def assert_planes(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a[: b.size], b), (what, k, np.nonzero(a[: b.size] != b)[0][:8])


@pytest.mark.parametrize("name", H.NAMES)
def test_truth_and_cpu_walker(zj, name):
    """ref_walk decodes every case (a case it cannot read is a broken input); it returns the encoder's planes in every
    group that must be kept; the CPU walker equals the truth."""
    c = H.case(name)
    want, same = H.truth(name)
    if c.expect in (H.KEEP, H.CPU):
        assert same, "the reference's reader does not return the planes this case encodes"
    if name in ("straddle-left-over", "walker-cut"):   # (walker-skip is written the reference's way: it reads it back)
        assert not same, "the reference reads this case like any decoder: it does not test what it is meant to"
    _, got, _ = zj.Decoder(options(zj, c)).decode_coefficients(c.data)
    assert_planes(got, want, "CPU walker")


@pytest.mark.parametrize("sub", H.SUBS)
@pytest.mark.parametrize("name", H.NAMES)
def test_emulated_device_stage(zj, name, sub):
    c = H.case(name)
    want, _ = H.truth(name)
    blob = prepared(zj, c, sub)
    if c.expect == H.CPU:
        assert blob is None
        return
    assert blob is not None, "the front-end did not prepare the scan for the device"
    hdr = H.blob_header(blob)
    assert hdr["sub_bytes"] == sub and hdr["tab_entries"] == c.entries()
    got, status, st = emu_c.huff_decode(blob, c.plane_lens())
    print(name, sub, "status", status, st)
    if c.expect == H.KEEP or (c.may_keep and status == 0):
        assert status == 0, (status, st)
        assert_planes(got, want, "device stage")
    else:
        assert status & c.expect, (status, st)


@pytest.mark.parametrize("name", ["hv", "hv_rst", "none", "h_rst", "gray"])
def test_encoder_bytes_have_not_changed(synth, name):
    """tools/jpeg_enc.py with tables=None writes the bytes stored in tests/golden/entropy_*.npz (tools/make_golden.py); the
    one-pair form writes what the per-component form writes when ids 0 and 1 hold that pair"""
    import jpeg_enc
    z = np.load(os.path.join(H.ROOT, "tests", "golden", f"entropy_{name}.npz"))
    ncomp, w, h, hs, vs, restart = (int(z[k]) for k in ("components", "width", "height", "h_max", "v_max", "restart"))
    planes = [z[c] for c in ("y", "cb", "cr")[:ncomp]]
    args = (planes, synth.quant_tables(85), w, h, hs, vs, ncomp)
    assert jpeg_enc.encode_baseline(*args, restart=restart) == z["jpeg"].tobytes()
    pair = jpeg_enc.canonical_tables({s: 4 if s < 8 else 5 for s in range(12)}, {s: 9 for s in range(255)})
    per = {"dc": {0: pair["dc"], 1: pair["dc"]}, "ac": {0: pair["ac"], 1: pair["ac"]}, "sel": [(0, 0), (1, 1), (1, 1)][:ncomp]}
    assert jpeg_enc.encode_baseline(*args, restart=restart, tables=pair) == jpeg_enc.encode_baseline(*args, restart=restart, tables=per)


def test_every_deep_lookup_goes_through_a_second_level():
    """the lengths themselves: no symbol the deep cases' data uses has a code that fits the first level"""
    for name in ("deep-links-gray", "deep-420-big", "deep-444-ri"):
        c = H.case(name)
        used = H.used_symbols(c.planes, c.w, c.h, c.hs, c.vs, c.ncomp, c.restart)
        for comp, (td, ta) in enumerate(c.sel):
            assert all(c.dc[td][s] > H.L1_DC for s in used[comp][0]), name
            assert all(c.ac[ta][s] > H.L1_AC for s in used[comp][1]), name
            assert len(used[comp][1]) > 20
    c = H.case("deep-ac-420")
    used = H.used_symbols(c.planes, c.w, c.h, c.hs, c.vs, c.ncomp, c.restart)
    assert all(c.ac[ta][s] > H.L1_AC for comp, (_, ta) in enumerate(c.sel) for s in used[comp][1])


def test_deep_tables_hold_several_links(zj):
    c = H.case("deep-links-gray")
    blob = prepared(zj, c, 16)
    hdr = H.blob_header(blob)
    ac, dc = H.blob_links(blob, hdr["ac_off"][0], True), H.blob_links(blob, hdr["dc_off"][0], False)
    assert len(ac) >= 3 and ac == list(range(len(ac))) == list(range(H.links(c.ac[0], True)))
    assert dc == list(range(H.links(c.dc[0], False))) and dc
    assert hdr["nsub"] > 1024                     # more than one prefix-sum workgroup, more than four decode workgroups
    c = H.case("deep-420-big")                    # chroma: DC sizes 0..4 hang off the second link
    blob = prepared(zj, c, 16)
    hdr = H.blob_header(blob)
    assert H.blob_links(blob, hdr["dc_off"][1], False) == [0, 1] and H.blob_links(blob, hdr["dc_off"][0], False) == [0]
    assert len(H.blob_links(blob, hdr["ac_off"][1], True)) >= 3


def test_sub_sequence_counts_cross_the_workgroups(zj):
    assert H.blob_header(prepared(zj, H.case("deep-420-big"), 16))["nsub"] > 1024
    assert H.blob_header(prepared(zj, H.case("deep-ac-420"), 16))["nsub"] > 256


def test_budget_pair(zj, monkeypatch, capfd):
    """7424 entries are prepared and kept; one AC link more (7456) is refused with reason 12 and decodes on the CPU"""
    fits, over = H.case("budget-exact"), H.case("budget-over")
    assert fits.entries() == H.TAB_BUDGET and over.entries() == H.TAB_BUDGET + 32
    blob = prepared(zj, fits, 32)
    hdr = H.blob_header(blob)
    assert hdr["tab_entries"] == 7424
    assert [len(H.blob_links(blob, hdr["dc_off"][k], False)) for k in (0, 1)] == [2, 0]
    assert [len(H.blob_links(blob, hdr["ac_off"][k], True)) for k in (0, 1)] == [40, 24]
    monkeypatch.setenv("ZJ_HUFF_DEBUG", "1")
    capfd.readouterr()
    assert prepared(zj, over, 32) is None
    assert "reason 12" in capfd.readouterr().err
    _, got, _ = zj.Decoder(options(zj, over, zj.ENTROPY_GPU_ALWAYS)).decode_coefficients(over.data)
    assert_planes(got, over.planes, "CPU path")


def test_three_ac_tables_have_offsets_of_their_own(zj):
    c = H.case("three-ac")
    hdr = H.blob_header(prepared(zj, c, 32))
    assert hdr["tab_entries"] == 7424
    assert len(set(hdr["ac_off"][:3])) == 3 and len(set(hdr["dc_off"][:3])) == 2 and hdr["dc_off"][1] == hdr["dc_off"][2]
    assert not set(hdr["ac_off"][:3]) & set(hdr["dc_off"][:3])
    assert H.blob_header(prepared(zj, H.case("min-all-ones"), 32))["tab_entries"] == H.case("min-all-ones").entries()


def test_straddling_symbols_are_where_the_cases_say():
    """the 26-bit symbols begin 1..8 bits in front of a multiple of 1024 bits of their segment -- checked on the file's
    own bytes: the bits at that place are the 16-bit code of a size-10 symbol"""
    for name in ("straddle-gray", "straddle-gray-ri", "straddle-420-ri", "straddle-left-over"):
        c = H.case(name)
        assert {d for _, _, d, last in c.placed if not last} == ({3, 7} if name == "straddle-left-over" else set(range(1, 9)))
        assert (c.restart == 60) == any(last for *_, last in c.placed)   # (4:2:0 intervals end with a chroma block)
        sos = c.data.index(b"\xff\xda")
        body = c.data[sos + 2 + int.from_bytes(c.data[sos + 2:sos + 4], "big"):-2]
        segs, cur, k = [], bytearray(), 0
        while k < len(body):
            if body[k] == 0xFF and body[k + 1] == 0:
                cur.append(0xFF)
                k += 2
            elif body[k] == 0xFF:
                segs.append(bytes(cur))
                cur = bytearray()
                k += 2
            else:
                cur.append(body[k])
                k += 1
        segs.append(bytes(cur))
        codes16 = {code for sym, (code, n) in H.canon(c.ac[0])["codes"].items() if n == 16 and sym & 15 == 10}
        for seg, limit, d, last in c.placed:
            bits = int.from_bytes(segs[seg], "big") >> (8 * len(segs[seg]) - (limit - d) - 16) & 0xFFFF
            assert bits in codes16, (name, seg, limit, d)
            if last:
                assert 8 * len(segs[seg]) - (limit - d + 26) < 8    # ... and the interval ends with it
