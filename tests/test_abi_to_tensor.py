"""CPU: the C ABI of the u8-images-to-tensor stage and the oriented crop-tensor file calls -- declared in
include/zjhip.h, let through by the version script, exported by the library, declared in the Rust extern block and listed by
the Python binding; the ABI version stays 8 (no struct changed); and the refusals that need no context.  The statuses of a
live context are in test_gpu_to_tensor.py."""
import ctypes as C
import fnmatch
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zj_to_tensor_device", "zj_decoder_finish_pixels_crop_tensor_oriented_device",
         "zj_decoder_finish_pixels_crop_tensor_batch_oriented_device"]
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


def test_abi_version_is_unchanged(zj):
    assert zj.lib().zj_abi_version() == 8
    assert "#define ZJ_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "zjhip.h")).read()


def test_the_wrappers_exist(zj):
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    import inspect
    assert hasattr(zj.Context, "to_tensor_device")
    sig = inspect.signature(tensors.to_normalized_tensor)
    assert list(sig.parameters) == ["ctx", "images", "dtype", "layout", "mean", "std", "flips", "channels", "stream"]
    assert inspect.signature(tensors.decode_files_cropped_to_tensor).parameters["apply_orientation"].default is False


def test_null_zero_and_three_to_one_are_argument_errors_without_a_context(zj):
    L = zj.lib()
    one = (C.c_void_p * 1)(16)
    out = C.c_void_p(64)
    call = lambda ctx, n, ins, w, h, cin, cout, dst: L.zj_to_tensor_device(ctx, n, ins, w, h, None, cin, cout, 0, 0, None, None, None,
                                                                          dst, None)
    assert call(None, 1, one, 8, 8, 3, 3, out) == ARG           # no context
    assert call(None, 0, one, 8, 8, 3, 3, out) == ARG           # no images
    assert call(None, 1, None, 8, 8, 3, 3, out) == ARG and call(None, 1, one, 8, 8, 3, 3, None) == ARG
    assert call(None, 1, one, 0, 8, 3, 3, out) == ARG and call(None, 1, one, 8, 0, 3, 3, out) == ARG
    assert call(None, 1, one, 8, 8, 3, 1, out) == ARG           # three channels into one
    n = C.c_size_t(0)
    assert L.zj_decoder_finish_pixels_crop_tensor_oriented_device(None, None, 0, 0, 8, 8, 0, 0, None, None, 0, None, 0, C.byref(n)) == ARG
    rcs = (C.c_int * 1)(7)
    org = (C.c_uint * 2)(0, 0)
    assert L.zj_decoder_finish_pixels_crop_tensor_batch_oriented_device(None, 0, None, None, 8, 8, 0, 0, None, None, None, None, 0, None) == ARG
    assert L.zj_decoder_finish_pixels_crop_tensor_batch_oriented_device((C.c_void_p * 1)(None), 1, None, org, 8, 8, 0, 0, None, None,
                                                                        None, C.c_void_p(16), 1024, rcs) == ARG
    dec = zj.Decoder()
    try:  # a decoder that has decoded nothing, and no context
        assert L.zj_decoder_finish_pixels_crop_tensor_oriented_device(dec._d, None, 0, 0, 8, 8, 0, 0, None, None, 0, C.c_void_p(16), 1024,
                                                                      C.byref(n)) == ARG
    finally:
        dec.close()
