"""ctypes binding of the CPU emulation of the antialiased resize kernel (tests/emu_resize_aa).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    L.zjea_weight.restype = C.c_uint32
    L.zjea_weight.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.zjea_axis.restype = None
    L.zjea_axis.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int),
                            C.POINTER(C.c_ulonglong)]
    L.zjea_resize.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def lib():
    return emu_build.load("emu_resize_aa", "libzjemuresizeaa.so", "zj_emu_resize_aa.cpp",
                          ("zj_stage_pack.h", "zj_resize_aa.h", "zj_resize.h", "zj_geom.h"),
                          "-O2", extra=("-ffp-contract=off",), bind=_bind)


def weights(i, n, m):
    """(lo, w[lo .. hi]) of destination index i: the emulated kernel's taps"""
    lo, hi, S = C.c_int(), C.c_int(), C.c_ulonglong()
    lib().zjea_axis(i, n, m, C.byref(lo), C.byref(hi), C.byref(S))
    return lo.value, np.array([lib().zjea_weight(i, n, m, j) for j in range(lo.value, hi.value + 1)], np.int64)


def resize(images, sizes, pitches, channels, in_chw, out_w, out_h, dtype, nhwc, s, b, flips=None, guard=64, poison=0xA5):
    """images: uint8 buffers (each in its layout at its pitch); returns the output bytes of the launch (guards checked)"""
    n = len(images)
    esz = {0: 4, 1: 2, 2: 2, 3: 1}[dtype]
    nb = n * channels * out_w * out_h * esz
    out = np.full(nb + 2 * guard, poison, np.uint8)
    ins = (C.c_void_p * n)(*[im.ctypes.data for im in images])
    wh = (C.c_uint * (2 * n))(*[v for sz in sizes for v in sz])
    pit = (C.c_uint * n)(*pitches)
    sf = (C.c_float * 3)(*(list(s) + [0.0] * (3 - len(s))))
    bf = (C.c_float * 3)(*(list(b) + [0.0] * (3 - len(b))))
    fl = (C.c_uint8 * n)(*[1 if f else 0 for f in flips]) if flips is not None else None
    rc = lib().zjea_resize(n, ins, wh, pit, channels, 1 if in_chw else 0, out_w, out_h, dtype, 1 if nhwc else 0, sf, bf, fl,
                           C.c_void_p(out.ctypes.data + guard))
    assert rc == 0
    assert (out[:guard] == poison).all() and (out[guard + nb:] == poison).all(), "the emulation wrote outside the output"
    return out[guard:guard + nb]
