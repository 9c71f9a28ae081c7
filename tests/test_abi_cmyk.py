"""CPU: the CMYK-to-RGB extension at the ABI: the new functions are declared, exported, bound and in the Rust
extern block; the flag's value; ZJ_ABI_VERSION unchanged; the flag on a zj_frame_desc is an unknown bit."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QTS = [np.ones(64, np.int32)] * 3
NEW = ("zj_cmyk_to_rgb_device", "zj_decoder_adobe_transform", "zj_decoder_plane")


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
    assert re.search(r"#define ZJ_FLAG_CMYK_TO_RGB 32u\b", header)
    assert re.search(r"#define ZJ_ABI_VERSION 8\b", header)  # (one flag bit and three functions: no struct changed)
    assert zj.lib().zj_abi_version() == 8
    assert re.search(r"pub const ZJ_FLAG_CMYK_TO_RGB: u32 = 32;", rs)
    assert hasattr(zj.Context, "cmyk_to_rgb_device") and hasattr(zj.Decoder, "plane") and hasattr(zj.Decoder, "adobe_transform")
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    assert callable(tensors.cmyk_to_rgb_tensor)


def test_the_flag(zj):
    assert zj.FLAG_CMYK_TO_RGB == 32
    assert zj.FLAG_CMYK_TO_RGB & (zj.FLAG_CORRECTED | zj.FLAG_FULL_AC_VALUES | zj.FLAG_GRAY_TO_RGB) == 0


def test_on_a_frame_descriptor_the_flag_is_an_unknown_bit(zj):
    L = zj.lib()
    F = zj.FLAG_CMYK_TO_RGB
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
    p = (C.c_void_p * 1)(16)
    assert L.zj_cmyk_to_rgb_device(None, 1, p, p, wh, None, None, 0, None, p, None, None) == -1
    assert L.zj_decoder_adobe_transform(None) == -1
    assert L.zj_decoder_plane(None, 0, None, None, None, None) == -1
    d = zj.Decoder()
    assert d.adobe_transform == -1
    with pytest.raises(zj.DecodeError):
        d.plane(0)  # (no file yet)
