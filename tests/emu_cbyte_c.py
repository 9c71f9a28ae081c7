"""ctypes binding of the CPU emulation of the fused tile kernel with byte chroma (tests/emu_cbyte).  TEST ONLY."""
import ctypes as C
import os

import numpy as np

import emu_build
from emu_c import FrameDesc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "emu_cbyte", "libzjemucbyte.so")
        csrc = os.path.join(ROOT, "zune-jpeg_amd", "csrc")
        srcs = [os.path.join(HERE, "emu_cbyte", "zj_emu_cbyte.cpp")] + [os.path.join(csrc, h) for h in ("zj_device.h", "zj_plan.h", "zj_geom.h")]
        emu_build.build(so, srcs, "-O1")
        _LIB = C.CDLL(so)
    return _LIB


def set_variant(variant):
    """0 = packed generation with staged stores where they apply, 2 = packed with direct stores"""
    lib().zjc_set_variant(C.c_int(int(variant)))


def stats():
    """(tiles decoded, tiles redone by the wide code, tiles whose chroma was staged as bytes) of the last decode_planes"""
    a = (C.c_longlong * 3)()
    lib().zjc_stats(a)
    return tuple(int(x) for x in a)


def tri_b(near, far):
    """The byte triangle filter (two byte averages) element by element; near, far: uint8 arrays, size % 4 == 0"""
    near, far = np.ascontiguousarray(near, np.uint8), np.ascontiguousarray(far, np.uint8)
    assert near.size == far.size and near.size % 4 == 0
    out = np.empty(near.size, np.uint8)
    lib().zjc_tri_b(C.c_void_p(near.ctypes.data), C.c_void_p(far.ctypes.data), C.c_void_p(out.ctypes.data), C.c_size_t(near.size))
    return out


def decode_planes(frame, planes, flags=0, out_layout=0, poison=0xAA):
    """frame: the oracle's zjo_frame; flags / out_layout: the extension fields of zj_frame_desc.  Returns (rc, bytes)."""
    arrs = [np.ascontiguousarray(p, np.int16) for p in planes]
    d = FrameDesc()
    for name in ("width", "height", "h_max", "v_max", "in_components", "out_colorspace"):
        setattr(d, name, getattr(frame, name))
    C.memmove(d.qt, frame.qt, 3 * 64 * 4)
    d.flags, d.out_layout, d.out_pitch = flags, out_layout, 0
    ncomp = {0: 3, 2: 3, 5: 4}[d.out_colorspace]
    out = np.full(d.width * d.height * ncomp, poison, np.uint8)
    rc = lib().zjc_decode_planes(C.byref(d), C.c_size_t(1), C.c_void_p(arrs[0].ctypes.data), C.c_void_p(arrs[1].ctypes.data),
                                 C.c_void_p(arrs[2].ctypes.data), C.c_void_p(out.ctypes.data), C.c_int(1))
    return rc, out
