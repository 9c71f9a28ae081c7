"""CPU: the C ABI of the colour matrices -- declared in include/zjhip.h, let through by the version script,
exported by the library, declared in the Rust extern block and listed by the Python binding with prototypes; the ABI version
stays 8 (no struct changed); the library stays under its size limit; the refusals that need no context.  The statuses of a
live context are in test_gpu_color.py."""
import ctypes as C
import fnmatch
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zj_color_fixed", "zj_color_device", "zj_decode_crops_resized_mixed_colored_device",
         "zj_decoder_finish_pixels_resized_crop_batch_colored_device"]
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
    # the library-internal calls stay inside
    assert not any(n.startswith("zjint_") for n in exported)


def test_the_coloured_calls_are_their_neighbours_plus_one_pointer(zj):
    L = zj.lib()
    a, b = L.zj_decode_crops_resized_mixed_device.argtypes, L.zj_decode_crops_resized_mixed_colored_device.argtypes
    assert len(b) == len(a) + 1 and list(b[:-3]) == list(a[:-2]) and list(b[-2:]) == list(a[-2:])
    a = L.zj_decoder_finish_pixels_resized_crop_batch_device.argtypes
    b = L.zj_decoder_finish_pixels_resized_crop_batch_colored_device.argtypes
    assert len(b) == len(a) + 1 and list(b[:-4]) == list(a[:-3]) and list(b[-3:]) == list(a[-3:])


def test_abi_version_is_unchanged(zj):
    assert zj.lib().zj_abi_version() == 8
    assert "#define ZJ_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "zjhip.h")).read()


def test_the_library_stays_under_its_size_limit(zj):
    if 1 not in zj.variants_available():
        assert os.path.getsize(zj.lib_path()) < 2_000_000


def test_the_unit_is_in_the_makefile():
    mk = open(os.path.join(ROOT, "zune-jpeg_amd", "csrc", "Makefile")).read()
    units = re.search(r"HIPUNITS := (.*?)\n(?!\s)", mk, flags=re.S).group(1).replace("\\\n", " ").split()
    assert "zj_color" in units and len(units) == 17


def test_the_wrappers_exist(zj):
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    assert hasattr(zj.Context, "color_device") and hasattr(zj, "color_fixed")
    sig = inspect.signature(tensors.color_matrix)
    assert list(sig.parameters) == ["brightness", "contrast", "saturation", "hue", "contrast_center", "grayscale", "bgr"]
    assert [p.default for p in sig.parameters.values()] == [1.0, 1.0, 1.0, 0.0, 128.0, False, False]
    m = tensors.color_matrix()
    assert m.shape == (3, 4) and m.dtype == np.float64 and np.array_equal(m, np.eye(3, 4))
    assert "DALI" in tensors.color_matrix.__doc__ and "torchvision" in tensors.color_matrix.__doc__
    sig = inspect.signature(tensors.color_twist_tensor)
    assert list(sig.parameters) == ["ctx", "images", "matrices", "in_layout", "inplace", "stream"]
    assert sig.parameters["in_layout"].default == "HWC" and sig.parameters["inplace"].default is False
    for f in (tensors.decode_resized_crops_to_tensor, tensors.decode_files_resized_to_tensor):
        assert inspect.signature(f).parameters["color"].default is None


def test_the_refusals_without_a_context(zj):
    L = zj.lib()
    one = (C.c_void_p * 1)(16)
    wh = (C.c_uint * 2)(8, 8)
    ident = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    call = lambda ctx, n, ins, sizes, layout, m, outs: L.zj_color_device(ctx, n, ins, sizes, None, layout, m, outs, None, None)
    assert call(None, 1, one, wh, 0, ident, one) == ARG                  # no context
    out = C.c_void_p(64)
    assert L.zj_decode_crops_resized_mixed_colored_device(None, None, 1, one, one, one, wh, 8, 8, 0, 0, None, None, None, 0, 0, None,
                                                          ident, out, None) == ARG
    bad = (C.c_double * 12)(17, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    assert L.zj_decode_crops_resized_mixed_colored_device(None, None, 1, one, one, one, wh, 8, 8, 0, 0, None, None, None, 0, 0, None,
                                                          bad, out, None) == ARG
    rcs = (C.c_int * 1)(7)
    win = (C.c_uint * 4)(0, 0, 8, 8)
    assert L.zj_decoder_finish_pixels_resized_crop_batch_colored_device(None, 0, None, None, 8, 8, 0, 0, None, None, None, 0, 0, 0,
                                                                        ident, None, 0, None) == ARG
    assert L.zj_decoder_finish_pixels_resized_crop_batch_colored_device((C.c_void_p * 1)(None), 1, None, win, 8, 8, 0, 0, None, None,
                                                                        None, 0, 0, 0, ident, out, 1024, rcs) == ARG and rcs[0] == 7
    q = (C.c_int32 * 12)()
    assert L.zj_color_fixed(None, q) == ARG and L.zj_color_fixed(ident, None) == ARG and L.zj_color_fixed(bad, q) == ARG
    assert L.zj_color_fixed(ident, q) == 0 and list(q) == [65536, 0, 0, 0, 0, 65536, 0, 0, 0, 0, 65536, 0]
