"""ctypes binding of the CPU emulation of the u8-images-to-tensor kernel (tests/emu_to_tensor).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build

ELEM = {0: 4, 1: 2, 2: 2, 3: 1}


def _bind(L):
    L.zjtt_to_tensor.restype = C.c_int
    L.zjtt_to_tensor.argtypes = [C.c_int, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                 C.c_void_p]


def lib():
    return emu_build.load("emu_to_tensor", "libzjemutotensor.so", "zj_emu_to_tensor.cpp",
                          ("zj_stage_pack.h", "zj_to_tensor.h", "zj_resize.h", "zj_geom.h", "emu_common/zj_emu_arena.h"),
                          "-O2", extra=("-ffp-contract=off",), bind=_bind)


def run():
    return lib().zjtt_run()


def batch():
    return lib().zjtt_batch()


def params_bytes():
    return lib().zjtt_params_bytes()


def to_tensor(in_addrs, w, h, pitches, cin, cout, dtype, nhwc, factors_s, factors_b, flips, arena, out_offset):
    """The launches of one call: in_addrs = addresses of the images' first bytes (h rows of w * cin bytes, pitches[i] apart),
    the tensor at arena[out_offset:].  factors_s / factors_b: the kernel's factors (scale * 2^-16, bias), 3 each.
    Returns (write map of the arena, stores that fell outside it, loads that fell outside their image)."""
    n = len(in_addrs)
    ins = (C.c_void_p * n)(*in_addrs)
    pt = (C.c_uint * n)(*pitches)
    s = (C.c_float * 3)(*[float(v) for v in factors_s])
    b = (C.c_float * 3)(*[float(v) for v in factors_b])
    fl = (C.c_ubyte * n)(*[1 if v else 0 for v in flips]) if flips is not None else None
    wmap = np.zeros(arena.size, np.uint8)
    counts = (C.c_longlong * 2)()
    rc = lib().zjtt_to_tensor(n, ins, w, h, pt, cin, cout, dtype, 1 if nhwc else 0, s, b, fl,
                              C.c_void_p(arena.ctypes.data + out_offset), C.c_void_p(arena.ctypes.data), arena.size,
                              C.c_void_p(wmap.ctypes.data), counts)
    assert rc == 0, "the emulation refused its arguments"
    return wmap, counts[0], counts[1]
