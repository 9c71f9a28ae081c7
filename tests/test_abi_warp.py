"""CPU: the C ABI of the affine warp -- declared in include/zjhip.h, let through by the version script,
exported by the library, declared in the Rust extern block and listed by the Python binding; the ABI version stays 8 (no
struct changed); the refusals that need no context; and the two host-only functions, which run without a GPU, against
tests/warp_model.py.  The statuses of a live context are in test_gpu_warp.py."""
import ctypes as C
import fnmatch
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import warp_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zj_warp_fixed", "zj_warp_source_window", "zj_warp_device", "zj_decode_crops_warped_device",
         "zj_decoder_finish_pixels_warped_device", "zj_decoder_finish_pixels_warped_batch_device"]
ARG = -1


@pytest.fixture(scope="module")
def zj():
    m = importlib.import_module("zune-jpeg_amd")
    if not os.path.exists(m.lib_path()):
        import __graft_entry__ as g
        g.build()
    return m


def test_names_in_header_map_exports_rust_and_binding(zj):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zjhip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    block = rs[rs.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    vs = open(os.path.join(ROOT, "zune-jpeg_amd", "csrc", "zjhip.map")).read()
    vs = re.sub(r"/\*.*?\*/", "", vs, flags=re.S)
    globs = re.findall(r"global:\s*([^;]+);", vs)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", zj.lib_path()], text=True)
    exported = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/zjhip.h"
        assert any(fnmatch.fnmatchcase(name, g.strip()) for g in globs), f"{name} is not let through by zjhip.map"
        assert name in exported, f"{name} is not exported by the library"
        assert re.search(r"pub fn " + name + r"\(", block), f"{name} is not in the Rust extern block"
        assert name in zj.abi_symbols() and hasattr(zj.lib(), name)
    for const, value in (("ZJ_WARP_FILL", 0), ("ZJ_WARP_REPLICATE", 1)):
        assert re.search(rf"#define {const} {value}\b", hdr) and f"pub const {const}: c_int = {value};" in rs
    assert (zj.WARP_FILL, zj.WARP_REPLICATE) == (0, 1)


def test_abi_version_is_unchanged(zj):
    assert zj.lib().zj_abi_version() == 8
    assert "#define ZJ_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "zjhip.h")).read()


def test_the_library_stays_under_its_size_limit(zj):
    if 1 not in zj.variants_available():
        assert os.path.getsize(zj.lib_path()) < 2_000_000


def test_the_wrappers_exist(zj):
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    assert hasattr(zj.Context, "warp_device") and hasattr(zj.Context, "decode_crops_warped_device")
    sig = inspect.signature(tensors.warp_to_tensor)
    assert list(sig.parameters) == ["ctx", "images", "matrices", "size", "dtype", "layout", "mean", "std", "fill", "edge", "stream"]
    assert sig.parameters["edge"].default == "fill" and sig.parameters["fill"].default is None
    assert list(inspect.signature(tensors.warp_matrix).parameters) == ["out_size", "center", "angle", "scale", "shear", "translate",
                                                                       "hflip"]
    assert inspect.signature(tensors.decode_warped_to_tensor).parameters["edge"].default == "fill"
    assert inspect.signature(tensors.decode_files_warped_to_tensor).parameters["apply_orientation"].default is False
    assert hasattr(zj, "finish_pixels_warped_batch") and hasattr(zj.Decoder, "finish_pixels_warped_device")
    with pytest.raises(ValueError):
        zj.warp_edge("wrap")


def test_the_refusals_without_a_context(zj):
    L = zj.lib()
    one = (C.c_void_p * 1)(16)
    wh = (C.c_uint * 2)(8, 8)
    ident = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    out = C.c_void_p(64)
    call = lambda ctx, n, ins, sizes, ch, m, ow, oh, edge, dst: L.zj_warp_device(ctx, n, ins, sizes, None, ch, m, ow, oh, 0, 0, None,
                                                                                 None, None, edge, dst, None)
    assert call(None, 1, one, wh, 3, ident, 8, 8, 0, out) == ARG       # no context
    assert call(None, 0, one, wh, 3, ident, 8, 8, 0, out) == ARG       # no images
    assert call(None, 1, None, wh, 3, ident, 8, 8, 0, out) == ARG and call(None, 1, one, None, 3, ident, 8, 8, 0, out) == ARG
    assert call(None, 1, one, wh, 3, None, 8, 8, 0, out) == ARG and call(None, 1, one, wh, 3, ident, 8, 8, 0, None) == ARG
    assert call(None, 1, one, wh, 2, ident, 8, 8, 0, out) == ARG and call(None, 1, one, wh, 3, ident, 8, 8, 2, out) == ARG
    assert L.zj_decode_crops_warped_device(None, None, 1, one, one, one, ident, 8, 8, 0, 0, None, None, None, 0, out, None) == ARG
    n = C.c_size_t(0)
    assert L.zj_decoder_finish_pixels_warped_device(None, None, ident, 0, 8, 8, 0, 0, None, None, None, 0, out, 1024, C.byref(n)) == ARG
    rcs = (C.c_int * 1)(7)
    assert L.zj_decoder_finish_pixels_warped_batch_device(None, 0, None, None, 0, 8, 8, 0, 0, None, None, None, 0, None, 0, None) == ARG
    assert L.zj_decoder_finish_pixels_warped_batch_device((C.c_void_p * 1)(None), 1, None, ident, 0, 8, 8, 0, 0, None, None, None, 0, out,
                                                          1024, rcs) == ARG and rcs[0] == 7
    q = (C.c_int64 * 6)()
    assert L.zj_warp_fixed(None, q) == ARG and L.zj_warp_fixed(ident, None) == ARG
    win = (C.c_uint * 4)()
    assert L.zj_warp_fixed(ident, q) == 0
    for bad in ((None, 8, 8, 4, 4, 0, win, q), (q, 0, 8, 4, 4, 0, win, q), (q, 8, 65536, 4, 4, 0, win, q), (q, 8, 8, 0, 4, 0, win, q),
                (q, 8, 8, 4, 8193, 0, win, q), (q, 8, 8, 4, 4, 2, win, q), (q, 8, 8, 4, 4, 0, None, q), (q, 8, 8, 4, 4, 0, win, None)):
        assert L.zj_warp_source_window(*bad) == ARG, bad
    huge = (C.c_int64 * 6)(1 << 33, 0, 0, 0, 1, 0)
    assert L.zj_warp_source_window(huge, 8, 8, 4, 4, 0, win, q) == ARG  # (no matrix has these integers)


def test_the_fixed_point_and_the_window_run_without_a_gpu(zj):
    rng = np.random.default_rng(16)
    for i in range(100):
        m = tuple(rng.uniform(-3, 3, 6) * (1, 1, 40, 1, 1, 40))
        q = zj.warp_fixed(m)
        assert q == wm.fixed(m)
        fw, fh, ow, oh = (int(v) for v in rng.integers(1, 40, 4))
        for edge, name in ((wm.FILL, "fill"), (wm.REPLICATE, "replicate")):
            assert zj.warp_source_window(q, fw, fh, ow, oh, name) == wm.source_window(q, fw, fh, ow, oh, edge)
    assert zj.warp_fixed((0, 1, 0, -1, 0, 37)) == [0, 1 << 24, 0, -(1 << 24), 0, 36 << 24]  # orientation 6 of a frame 37 high
    for bad in ((float("nan"), 0, 0, 0, 1, 0), (128.0, 0, 0, 0, 1, 0), (1, 0, 2.0 ** 31, 0, 1, 0), (1, 0, 0, 0, float("inf"), 0)):
        with pytest.raises(zj.ZjError) as e:
            zj.warp_fixed(bad)
        assert e.value.status == ARG
