"""CPU: the any-sampling extension at the ABI: the new functions are declared, exported, bound and in the
Rust extern block; the flag's value; ZJ_ABI_VERSION unchanged; the flag on a zj_frame_desc is an unknown bit; NULL and bad
arguments."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QTS = [np.ones(64, np.int32)] * 3
NEW = ("zj_planes_to_rgb_device", "zj_decoder_stored_rgb", "zj_decoder_component_sampling")


@pytest.fixture(scope="module")
def zj():
    m = importlib.import_module("zune-jpeg_amd")
    if not os.path.exists(m.lib_path()):
        import __graft_entry__ as g
        g.build()
    return m


def test_the_functions_are_declared_exported_and_bound(zj):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zjhip.h")).read(), flags=re.S)
    exported = [ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", zj.lib_path()], text=True).splitlines()
                if ln.strip()]
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    vmap = open(os.path.join(ROOT, "zune-jpeg_amd", "csrc", "zjhip.map")).read()
    assert re.search(r"global:\s*zj_\*;", vmap)  # (the version script exports what begins zj_: the header's functions)
    for name in NEW:
        assert re.search(r"\bZJ_API int " + name + r"\s*\(", header), name
        assert name in exported, name
        assert name in zj.abi_symbols(), name
        assert re.search(r"pub fn " + name + r"\(", rs), name
        assert getattr(zj.lib(), name).argtypes is not None, name
    assert re.search(r"#define ZJ_FLAG_ANY_SAMPLING 64u\b", header)
    assert re.search(r"#define ZJ_ABI_VERSION 8\b", header)  # (one flag bit and three functions: no struct changed)
    assert zj.lib().zj_abi_version() == 8
    assert re.search(r"pub const ZJ_FLAG_ANY_SAMPLING: u32 = 64;", rs)
    assert hasattr(zj.Context, "planes_to_rgb_device") and hasattr(zj.Decoder, "component_sampling") and hasattr(zj.Decoder, "stored_rgb")
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    assert callable(tensors.planes_to_rgb_tensor)


def test_the_argument_lists_agree(zj):
    """the header's parameter count against the ctypes binding and the Rust extern block"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zjhip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NEW:
        c_args = re.search(r"\bZJ_API int " + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        r_args = re.search(r"pub fn " + name + r"\((.*?)\)\s*->\s*c_int;", rs, flags=re.S).group(1)
        n = len(c_args.split(","))
        assert n == len(r_args.split(",")) == len(getattr(zj.lib(), name).argtypes), name


def test_the_flag(zj):
    assert zj.FLAG_ANY_SAMPLING == 64
    assert zj.FLAG_ANY_SAMPLING & (zj.FLAG_CORRECTED | zj.FLAG_FULL_AC_VALUES | zj.FLAG_GRAY_TO_RGB | zj.FLAG_CMYK_TO_RGB) == 0


def test_on_a_frame_descriptor_the_flag_is_an_unknown_bit(zj):
    L = zj.lib()
    F = zj.FLAG_ANY_SAMPLING
    w, h = C.c_uint(0), C.c_uint(0)
    for ncomp, cs in ((3, zj.ColorSpace.RGB), (3, zj.ColorSpace.YCbCr), (1, zj.ColorSpace.GRAYSCALE)):
        for extra in (0, zj.FLAG_CORRECTED, zj.FLAG_GRAY_TO_RGB):
            d = zj.FrameDesc.make(48, 40, 1, 1, ncomp, cs, QTS, flags=F | extra)
            assert L.zj_scaled_size(C.byref(d), 1, C.byref(w), C.byref(h)) == -1  # ZJ_ERR_ARG
            assert zj.crop_out_len(d, 8, 8) == 0
            assert zj.resized_out_len(d, 10, 7, zj.DTYPE_U8) == 0
            assert L.zj_scaled_crop_out_len(C.byref(d), 1, 8, 8, 0) == 0
    ok = zj.FrameDesc.make(48, 40, 1, 1, 3, zj.ColorSpace.RGB, QTS)
    assert L.zj_scaled_size(C.byref(ok), 1, C.byref(w), C.byref(h)) == 0 and (w.value, h.value) == (24, 20)


def test_the_new_calls_refuse_null_arguments(zj):
    L = zj.lib()
    wh = (C.c_uint * 2)(4, 4)
    rt = (C.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    p = (C.c_void_p * 1)(16)
    assert L.zj_planes_to_rgb_device(None, 1, p, p, p, wh, rt, None, 0, 0, p, None, None) == -1  # ZJ_ERR_ARG
    assert L.zj_decoder_stored_rgb(None) == 0
    hh, vv = C.c_uint(9), C.c_uint(9)
    assert L.zj_decoder_component_sampling(None, 0, C.byref(hh), C.byref(vv)) == -1
    d = zj.Decoder()
    assert not d.stored_rgb
    with pytest.raises(zj.DecodeError):
        d.component_sampling(0)  # (no file yet)
    assert (hh.value, vv.value) == (9, 9)
