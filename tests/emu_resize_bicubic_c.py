"""ctypes binding of the CPU emulation of the bicubic antialiased resize kernel (tests/emu_resize_bicubic).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    L.zjeb_axis.restype = None
    L.zjeb_axis.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.zjeb_K.restype = C.c_longlong
    L.zjeb_K.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.zjeb_R.restype = C.c_int
    L.zjeb_R.argtypes = [C.c_longlong, C.c_longlong]
    L.zjeb_resize.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def lib():
    return emu_build.load("emu_resize_bicubic", "libzjemuresizebicubic.so", "zj_emu_resize_bicubic.cpp",
                          ("zj_stage_pack.h", "zj_resize_bicubic.h", "zj_resize_aa.h", "zj_resize.h", "zj_geom.h"),
                          "-O2", extra=("-ffp-contract=off",), bind=_bind)


def weights(i, n, m):
    """(lo, w[lo .. hi], S) of destination index i from the emulated kernel's bc_axis, bc_K and bc_R"""
    lo, hi = C.c_int(), C.c_int()
    lib().zjeb_axis(i, n, m, C.byref(lo), C.byref(hi))
    Kp = np.zeros(hi.value - lo.value + 1, np.int32)
    S = lib().zjeb_K(i, n, m, Kp.ctypes.data)
    Cs = np.cumsum(Kp.astype(np.int64))
    if len(Cs) > 64:  # (a long axis: R of the whole prefix in numpy, of a sample through bc_R)
        R = (Cs * (1 << 14) + S // 2) // S
        for k in range(0, len(Cs), max(1, len(Cs) // 61)):
            assert lib().zjeb_R(int(Cs[k]), S) == R[k]
    else:
        R = np.array([lib().zjeb_R(int(c), S) for c in Cs], np.int64)
    return lo.value, np.diff(R, prepend=0), S


def resize(images, sizes, pitches, channels, in_chw, out_w, out_h, dtype, nhwc, s, b, flips=None, guard=64, poison=0xA5,
           clamped=None):
    """images: uint8 buffers (each in its layout at its pitch); returns the output bytes of the launch (guards checked).
    clamped: a list that receives how many values the final clamp cut at 0 and at 255 x 2^16"""
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
    cl = (C.c_longlong * 2)(0, 0)
    rc = lib().zjeb_resize(n, ins, wh, pit, channels, 1 if in_chw else 0, out_w, out_h, dtype, 1 if nhwc else 0, sf, bf, fl,
                           C.c_void_p(out.ctypes.data + guard), cl)
    assert rc == 0
    if clamped is not None:
        clamped[:] = [cl[0], cl[1]]
    assert (out[:guard] == poison).all() and (out[guard + nb:] == poison).all(), "the emulation wrote outside the output"
    return out[guard:guard + nb]
