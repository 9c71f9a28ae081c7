"""CPU: the C ABI of the tone curves -- declared in include/zjhip.h, let through by the version script,
exported by the library, declared in the Rust extern block and listed by the Python binding with prototypes; the op
constants' values in the header, the Rust binding and the package; the ABI version stays 8 (functions only); the refusals
that need no context.  The statuses of a live context are in test_gpu_tone.py."""
import ctypes as C
import fnmatch
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import abi_types
import tone_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zj_histogram_device", "zj_tone_luts_device", "zj_lut_device", "zj_tone_device",
         "zj_decode_crops_resized_mixed_toned_device", "zj_decoder_finish_pixels_resized_crop_batch_toned_device"]
OPS = {"ZJ_TONE_IDENTITY": 0, "ZJ_TONE_INVERT": 1, "ZJ_TONE_POSTERIZE": 2, "ZJ_TONE_SOLARIZE": 3, "ZJ_TONE_AUTOCONTRAST": 4,
       "ZJ_TONE_EQUALIZE": 5}
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
        assert getattr(zj.lib(), name).argtypes, f"{name} has no prototype in host.py"
    assert not any(n.startswith("zjint_") for n in exported)


def test_the_constants_values(zj):
    hdr = open(os.path.join(ROOT, "include", "zjhip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, value in OPS.items():
        assert re.search(rf"#define {name} {value}\b", hdr), name
        assert re.search(rf"pub const {name}: i32 = {value};", rs), name
        assert getattr(zj, name[3:]) == value
    assert (tm.IDENTITY, tm.INVERT, tm.POSTERIZE, tm.SOLARIZE, tm.AUTOCONTRAST, tm.EQUALIZE) == tuple(OPS.values())
    assert zj.TONE_OPS == {k[8:].lower(): v for k, v in OPS.items()}


def test_the_toned_calls_are_their_neighbours_plus_one_pointer(zj):
    L = zj.lib()
    a, b = L.zj_decode_crops_resized_mixed_colored_device.argtypes, L.zj_decode_crops_resized_mixed_toned_device.argtypes
    assert len(b) == len(a) + 1 and list(b[:-3]) == list(a[:-2]) and list(b[-2:]) == list(a[-2:])
    a = L.zj_decoder_finish_pixels_resized_crop_batch_colored_device.argtypes
    b = L.zj_decoder_finish_pixels_resized_crop_batch_toned_device.argtypes
    assert len(b) == len(a) + 1 and list(b[:-4]) == list(a[:-3]) and list(b[-3:]) == list(a[-3:])


def test_abi_version_is_unchanged(zj):
    assert zj.lib().zj_abi_version() == 8
    assert "#define ZJ_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "zjhip.h")).read()


def test_the_library_stays_under_its_size_limit(zj):
    if 1 not in zj.variants_available():
        assert os.path.getsize(zj.lib_path()) < 2_000_000


def test_the_unit_is_built_and_linked():
    mk = open(os.path.join(ROOT, "zune-jpeg_amd", "csrc", "Makefile")).read()
    more = re.search(r"HIPUNITS_MORE := (.*)", mk).group(1).split()
    assert "zj_tone" in more and "$(HIPUNITS_MORE:%=$(HERE)%.o)" in mk
    for f in ("zj_tone.hip", "zj_tone.h", "zj_tone_launch.h", "zj_tone_ops.h"):
        assert os.path.exists(os.path.join(ROOT, "zune-jpeg_amd", "csrc", f))


def test_the_wrappers_exist(zj):
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    for m in ("histogram_device", "tone_luts_device", "lut_device", "tone_device"):
        assert hasattr(zj.Context, m)
    assert tensors.tone_op("equalize") == (5, 0) and tensors.tone_op("posterize", 4) == (2, 4) and tensors.tone_op(3, 256) == (3, 256)
    for bad in (("posterize", 0), ("solarize", 257), ("invert", 1)):
        with pytest.raises(ValueError):
            tensors.tone_op(*bad)
    g = tensors.gamma_lut(1.0)
    assert g.shape == (3, 256) and g.dtype == np.uint8 and np.array_equal(g[2], np.arange(256))
    g = tensors.gamma_lut(0.5, 2.0)
    assert list(g[0, :3]) == [min(255, int(255 * 2.0 * (i / 255) ** 0.5 + 0.5)) for i in range(3)] and g[0, 255] == 255
    sig = inspect.signature(tensors.tone_tensor)
    assert list(sig.parameters) == ["ctx", "images", "ops", "in_layout", "inplace", "stream"]
    assert sig.parameters["in_layout"].default == "HWC" and sig.parameters["inplace"].default is False
    assert hasattr(tensors, "histogram_tensor") and hasattr(tensors, "lut_tensor")
    for f in (tensors.decode_resized_crops_to_tensor, tensors.decode_files_resized_to_tensor):
        assert inspect.signature(f).parameters["tone"].default is None


def test_the_refusals_without_a_context(zj):
    L = zj.lib()
    one = (C.c_void_p * 1)(16)
    wh = (C.c_uint * 2)(8, 8)
    op = (C.c_int32 * 2)(1, 0)
    bad = (C.c_int32 * 2)(2, 9)
    tab = C.c_void_p(4096)
    assert L.zj_tone_device(None, 1, one, wh, None, 3, 0, op, one, None, None) == ARG
    assert L.zj_lut_device(None, 1, one, wh, None, 3, 0, tab, one, None, None) == ARG
    assert L.zj_histogram_device(None, 1, one, wh, None, 3, 0, tab, None) == ARG
    assert L.zj_tone_luts_device(None, 1, 3, op, None, tab, None) == ARG
    out = C.c_void_p(64)
    assert L.zj_decode_crops_resized_mixed_toned_device(None, None, 1, one, one, one, wh, 8, 8, 0, 0, None, None, None, 0, 0, None,
                                                        None, op, out, None) == ARG
    assert L.zj_decode_crops_resized_mixed_toned_device(None, None, 1, one, one, one, wh, 8, 8, 0, 0, None, None, None, 0, 0, None,
                                                        None, bad, out, None) == ARG
    rcs = (C.c_int * 1)(7)
    win = (C.c_uint * 4)(0, 0, 8, 8)
    assert L.zj_decoder_finish_pixels_resized_crop_batch_toned_device(None, 0, None, None, 8, 8, 0, 0, None, None, None, 0, 0, 0, None,
                                                                      op, None, 0, None) == ARG
    assert L.zj_decoder_finish_pixels_resized_crop_batch_toned_device((C.c_void_p * 1)(None), 1, None, win, 8, 8, 0, 0, None, None,
                                                                      None, 0, 0, 0, None, op, out, 1024, rcs) == ARG and rcs[0] == 7


def test_the_extern_block_matches_the_header():
    """tests/abi_types.py's comparison of every extern fn with the header, and the six new functions among both"""
    hdr = open(os.path.join(ROOT, "include", "zjhip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    c, r = abi_types.c_prototypes(hdr), abi_types.rust_externs(rs)
    for name in NAMES:
        assert name in c and name in r, name
    assert abi_types.compare(hdr, rs) == []
