"""ctypes binding of the CPU emulation of the resize kernel (tests/emu_resize).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    L.zjer_tap.restype = C.c_uint32
    L.zjer_tap.argtypes = [C.c_uint32] * 3
    L.zjer_f32.restype = C.c_float
    L.zjer_f32.argtypes = [C.c_uint32, C.c_float, C.c_float]
    L.zjer_f16.restype = C.c_uint32
    L.zjer_f16.argtypes = [C.c_float]
    L.zjer_bf16.restype = C.c_uint32
    L.zjer_bf16.argtypes = [C.c_float]
    L.zjer_resize.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def lib():
    return emu_build.load("emu_resize", "libzjemuresize.so", "zj_emu_resize.cpp",
                          ("zj_stage_pack.h", "zj_resize.h", "zj_geom.h"),
                          "-O1", extra=("-ffp-contract=off",), bind=_bind)


def tap(i, n, m):
    t = lib().zjer_tap(i, n, m)
    return t & 0xFFFF, (t >> 16) & 255, (t & 0xFFFF) + (t >> 24)


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
    rc = lib().zjer_resize(n, ins, wh, pit, channels, 1 if in_chw else 0, out_w, out_h, dtype, 1 if nhwc else 0, sf, bf, fl,
                           C.c_void_p(out.ctypes.data + guard))
    assert rc == 0
    assert (out[:guard] == poison).all() and (out[guard + nb:] == poison).all(), "the emulation wrote outside the output"
    return out[guard:guard + nb]
