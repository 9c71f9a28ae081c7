"""GPU: byte chroma (Cfg::CBYTE, zune-jpeg_amd/csrc/zj_device.h) through zj_decode_planes_device, byte for byte against the
oracle: the shapes and planted contents of tests/chroma_bytes_cases.py under the staged-store and the direct-store variant,
aligned widths (the fused kernels) and ragged ones (the ragged family).  The planted DC-only chroma blocks whose shortcut
value is 256 / -1 -- in a block wave and in a halo column -- send their tiles through the redo by the wide code."""
import ctypes as C
import importlib

import numpy as np
import pytest

import chroma_bytes_cases as cases
import oracle_c as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)  # no GPU -> raises; nothing falls back to the CPU
    yield c
    c.set_variant(0)
    c.close()


def _decode_device(zj, ctx, desc, planes):
    out_len = zj.lib().zj_out_len(C.byref(desc))
    bufs = [ctx.device_alloc(p.nbytes) for p in planes] + [ctx.device_alloc(out_len)]
    try:
        for p, b in zip(planes, bufs):
            ctx.h2d(b, p)
        ctx.decode_planes_device(desc, 1, bufs[0], bufs[1], bufs[2], bufs[3])
        ctx.sync()
        out = np.empty(out_len, np.uint8)
        ctx.d2h(out, bufs[3])
    finally:
        for b in bufs:
            ctx.device_free(b)
    return out


@pytest.mark.parametrize("mode", list(cases.MODES))
@pytest.mark.parametrize("kind", cases.OUT_KINDS)
@pytest.mark.parametrize("wh", cases.ALIGNED + cases.RAGGED)
def test_byte_chroma_on_the_device_matches_oracle(zj, ctx, mode, kind, wh):
    w, h = wh
    hs, vs = cases.MODES[mode]
    planes, qts = cases.frame(w, h, mode)
    cases.assert_planted(w, h, mode)  # the redo is exercised: the out-of-range blocks are in what the device is given
    cs = {"rgb": oc.RGB, "ycbcr": oc.YCBCR, "rgba": oc.RGBA, "chw": oc.RGB}[kind]
    for flags in cases.FLAG_SETS:
        exp = cases.expected(w, h, mode, kind, flags)
        desc = zj.FrameDesc.make(w, h, hs, vs, 3, cs, qts, flags=flags, out_layout=zj.LAYOUT_CHW if kind == "chw" else zj.LAYOUT_HWC)
        for variant in (0, 2):
            ctx.set_variant(variant)
            out = _decode_device(zj, ctx, desc, planes)
            bad = np.nonzero(out != exp)[0]
            assert bad.size == 0, (mode, kind, wh, flags, variant, bad.size, bad[:8])
