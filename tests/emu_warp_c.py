"""ctypes binding of the CPU emulation of the affine-warp kernels (tests/emu_warp).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build

ELEM = {0: 4, 1: 2, 2: 2, 3: 1}
FILL, REPLICATE = 0, 1


def _bind(L):
    L.zjew_fixed.restype = C.c_int
    L.zjew_fixed.argtypes = [C.c_void_p, C.c_void_p]
    L.zjew_window.restype = None
    L.zjew_window.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    L.zjew_warp.restype = C.c_int
    L.zjew_warp.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                            C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                            C.c_void_p, C.c_void_p]


def lib():
    return emu_build.load("emu_warp", "libzjemuwarp.so", "zj_emu_warp.cpp",
                          ("zj_stage_pack.h", "zj_warp.h", "zj_warp_fixed.h", "zj_resize.h", "zj_geom.h", "emu_common/zj_emu_arena.h"),
                          "-O2", extra=("-ffp-contract=off",), bind=_bind)


def group():
    return lib().zjew_group()


def batch():
    return lib().zjew_batch()


def block_rows():
    return lib().zjew_block_rows()


def params_bytes():
    return lib().zjew_params_bytes()


def fixed(m):
    """the six integers of the matrix m (6 floats), None: refused"""
    md = (C.c_double * 6)(*[float(v) for v in m])
    q = (C.c_int64 * 6)()
    return None if lib().zjew_fixed(md, q) else [int(v) for v in q]


def window(q, fw, fh, out_w, out_h, edge):
    """(x, y, w, h), the shifted integers"""
    qi = (C.c_int64 * 6)(*q)
    win = (C.c_uint * 4)()
    sh = (C.c_int64 * 6)()
    lib().zjew_window(qi, fw, fh, out_w, out_h, edge, win, sh)
    return tuple(int(v) for v in win), [int(v) for v in sh]


def warp(in_addrs, whs, pitches, channels, ints, out_w, out_h, dtype, nhwc, factors_s, factors_b, fill, edge, arena, out_offset):
    """The launches of one call: in_addrs = addresses of the images' first bytes (whs[i] = (w, h), rows pitches[i] apart),
    ints[i] the six integers of image i, the tensor at arena[out_offset:].  factors_s / factors_b: the kernel's factors
    (scale * 2^-16, bias), 3 each.  Returns (write map of the arena, stores that fell outside it, loads that fell outside
    their image, loads)."""
    n = len(in_addrs)
    ins = (C.c_void_p * n)(*in_addrs)
    wh = (C.c_uint * (2 * n))(*[v for p in whs for v in p])
    pt = (C.c_uint * n)(*pitches)
    qi = (C.c_int64 * (6 * n))(*[v for q in ints for v in q])
    s = (C.c_float * 3)(*[float(v) for v in factors_s])
    b = (C.c_float * 3)(*[float(v) for v in factors_b])
    fl = (C.c_ubyte * 3)(*[int(v) for v in fill])
    wmap = np.zeros(arena.size, np.uint8)
    counts = (C.c_longlong * 3)()
    rc = lib().zjew_warp(n, ins, wh, pt, channels, qi, out_w, out_h, dtype, 1 if nhwc else 0, s, b, fl, edge,
                         C.c_void_p(arena.ctypes.data + out_offset), C.c_void_p(arena.ctypes.data), arena.size,
                         C.c_void_p(wmap.ctypes.data), counts)
    assert rc == 0, "the emulation refused its arguments"
    return wmap, counts[0], counts[1], counts[2]
