"""GPU: the entropy stage on the device (zune-jpeg_amd/csrc/zj_huff.hip) over the code-table shapes of
tests/huff_table_cases.py, in the two layers of tests/test_gpu_entropy.py: the planes zj_decode_scan leaves in HBM against
the truth (the encoder's planes, or oracle/ref_walk.py's where the reference reads the file its own way), and
decode_buffer under ENTROPY_GPU_ALWAYS against the same call with the CPU entropy stage.  The yardsticks and the condition
that no case of the kept groups may come back from the device are those of tests/test_huff_tables_emu.py, which runs
every case at every sub-sequence size on the CPU; here every case runs at one size, rotating through 16, 32 and 128 within
its group, and the straddle group at all three (huff_table_cases.subs_of)."""
import importlib
import os

import numpy as np
import pytest

import huff_table_cases as H

pytestmark = pytest.mark.gpu

RUNS = [(n, s) for n in H.NAMES for s in H.subs_of(n)]


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)
    yield c
    c.close()


def decoder(zj, ctx, c, entropy, sub):
    old = os.environ.get("ZJ_HUFF_SUB")
    os.environ["ZJ_HUFF_SUB"] = str(sub)
    try:
        o = zj.ZuneJpegOptions()
        o.flags, o.entropy = c.flags, entropy
        return zj.Decoder(o, ctx)
    finally:
        if old is None:
            del os.environ["ZJ_HUFF_SUB"]
        else:
            os.environ["ZJ_HUFF_SUB"] = old


def test_every_size_serves_every_group():
    for g in set(H.GROUP.values()):
        assert {s for n, s in RUNS if H.GROUP[n] == g and n not in H.CPU_NAMES} == set(H.SUBS), g
    assert {(n, s) for n, s in RUNS if H.GROUP[n] == "straddle"} == {(n, s) for n in H.NAMES if H.GROUP[n] == "straddle" for s in H.SUBS}


@pytest.mark.parametrize("name,sub", RUNS)
def test_planes_in_hbm(zj, ctx, name, sub):
    c = H.case(name)
    want, _ = H.truth(name)
    g = decoder(zj, ctx, c, zj.ENTROPY_GPU_ALWAYS, sub)
    desc, _ = g.prepare(c.data)
    blob = g.scan_blob()
    if c.expect == H.CPU:
        assert blob is None
        return
    assert blob is not None and H.blob_header(blob)["tab_entries"] == c.entries()
    out, rc, st = ctx.decode_scan(desc, blob)
    if c.expect != H.KEEP and not (c.may_keep and st == 0):
        assert rc == zj.RETRY_CPU and st & c.expect, (rc, st)
        return
    assert rc == 0 and st == 0, (rc, [v for k, v in zj.HUFF_ST.items() if st & k])
    for k, (a, b) in enumerate(zip(ctx.scan_planes(), want)):
        assert np.array_equal(a, b), (name, sub, k, np.nonzero(a != b)[0][:8])


@pytest.mark.parametrize("name,sub", RUNS)
def test_pixels_equal_the_cpu_entropy_stage(zj, ctx, name, sub):
    c = H.case(name)
    g = decoder(zj, ctx, c, zj.ENTROPY_GPU_ALWAYS, sub)
    got = g.decode_buffer(c.data)
    st = g.gpu_status()
    if c.expect in (H.KEEP, H.CPU):
        assert st == 0, [v for k, v in zj.HUFF_ST.items() if st & k]
        assert (g.scan_blob() is None) == (c.expect == H.CPU)
    else:
        assert st & c.expect or (c.may_keep and st == 0), st
    assert np.array_equal(got, decoder(zj, ctx, c, zj.ENTROPY_CPU, sub).decode_buffer(c.data))
