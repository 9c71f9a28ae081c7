"""CPU: the gray-to-RGB extension at the ABI: zj_gray_to_rgb_device is declared, exported, bound and in the
Rust extern block; the flag's value; what zj_resized_out_len says for one- and three-component descriptors with the flag."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QTS = [np.ones(64, np.int32)] * 3


@pytest.fixture(scope="module")
def zj():
    m = importlib.import_module("zune-jpeg_amd")
    if not os.path.exists(m.lib_path()):
        import __graft_entry__ as g
        g.build()
    return m


def test_the_stage_is_declared_exported_and_bound(zj):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zjhip.h")).read(), flags=re.S)
    assert re.search(r"\bZJ_API int zj_gray_to_rgb_device\s*\(", header)
    assert re.search(r"#define ZJ_FLAG_GRAY_TO_RGB 16u\b", header)
    assert re.search(r"#define ZJ_ABI_VERSION 8\b", header)  # (one flag bit and one function: no struct changed)
    out = subprocess.check_output(["nm", "-D", "--defined-only", zj.lib_path()], text=True)
    assert "zj_gray_to_rgb_device" in [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert "zj_gray_to_rgb_device" in zj.abi_symbols()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"pub fn zj_gray_to_rgb_device\(ctx: \*mut zj_ctx, n: usize,", rs)
    assert re.search(r"pub const ZJ_FLAG_GRAY_TO_RGB: u32 = 16;", rs)
    assert hasattr(zj.Context, "gray_to_rgb_device")
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    assert callable(tensors.gray_to_rgb_tensor)


def test_the_flag(zj):
    assert zj.FLAG_GRAY_TO_RGB == 16
    assert zj.FLAG_GRAY_TO_RGB & (zj.FLAG_CORRECTED | zj.FLAG_FULL_AC_VALUES) == 0


def test_the_stage_refuses_a_null_context_and_null_arrays(zj):
    L = zj.lib()
    assert L.zj_gray_to_rgb_device(None, 1, None, None, None, 0, None, None, None) == -1  # ZJ_ERR_ARG
    wh = (C.c_uint * 2)(4, 4)
    p = (C.c_void_p * 1)(16)
    assert L.zj_gray_to_rgb_device(None, 1, p, wh, None, 0, p, None, None) == -1


def test_resized_out_len_with_the_flag(zj):
    F = zj.FLAG_GRAY_TO_RGB
    mk = lambda ncomp, cs, flags, **kw: zj.FrameDesc.make(48, 40, 1, 1, ncomp, cs, QTS, flags=flags, **kw)
    # one component, RGB, the flag: the 3-channel length, both crop layouts, with the other extensions beside it
    assert zj.resized_out_len(mk(1, zj.ColorSpace.RGB, F), 10, 7, zj.DTYPE_U8) == 3 * 70
    assert zj.resized_out_len(mk(1, zj.ColorSpace.RGB, F), 10, 7, zj.DTYPE_F32) == 3 * 70 * 4
    assert zj.resized_out_len(mk(1, zj.ColorSpace.RGB, F, out_layout=zj.LAYOUT_CHW), 10, 7, zj.DTYPE_BF16) == 3 * 70 * 2
    assert zj.resized_out_len(mk(1, zj.ColorSpace.RGB, F | zj.FLAG_CORRECTED), 10, 7, zj.DTYPE_U8) == 3 * 70
    # ... YCbCr: no such output
    assert zj.resized_out_len(mk(1, zj.ColorSpace.YCbCr, F), 10, 7, zj.DTYPE_U8) == 0
    # ... GRAYSCALE: the flag does nothing
    assert zj.resized_out_len(mk(1, zj.ColorSpace.GRAYSCALE, F), 10, 7, zj.DTYPE_U8) == 70
    # three components: the same length as without the flag, whatever the output
    for cs in (zj.ColorSpace.RGB, zj.ColorSpace.YCbCr, zj.ColorSpace.GRAYSCALE, zj.ColorSpace.RGBA):
        for hs, vs in ((1, 1), (2, 2)):
            a = zj.FrameDesc.make(48, 40, hs, vs, 3, cs, QTS, flags=F)
            b = zj.FrameDesc.make(48, 40, hs, vs, 3, cs, QTS)
            assert zj.resized_out_len(a, 10, 7, zj.DTYPE_F16) == zj.resized_out_len(b, 10, 7, zj.DTYPE_F16)
    assert zj.resized_out_len(zj.FrameDesc.make(48, 40, 2, 2, 3, zj.ColorSpace.RGB, QTS, flags=F), 10, 7, zj.DTYPE_U8) == 210
    # an unknown bit beside it is still refused
    assert zj.resized_out_len(mk(1, zj.ColorSpace.RGB, F | 32), 10, 7, zj.DTYPE_U8) == 0


def test_every_other_length_call_treats_the_flag_as_an_unknown_bit(zj):
    L = zj.lib()
    d = zj.FrameDesc.make(48, 40, 1, 1, 3, zj.ColorSpace.RGB, QTS, flags=zj.FLAG_GRAY_TO_RGB)
    assert zj.crop_out_len(d, 8, 8) == 0
    assert L.zj_scaled_crop_out_len(C.byref(d), 1, 8, 8, 0) == 0
