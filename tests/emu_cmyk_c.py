"""ctypes binding of the CPU emulation of the CMYK-to-RGB kernel (tests/emu_cmyk).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    L.zjck_combine.restype = C.c_longlong
    L.zjck_combine.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


def lib():
    return emu_build.load("emu_cmyk", "libzjemucmyk.so", "zj_emu_cmyk.cpp",
                          ("zj_stage_pack.h", "zj_cmyk.h", "zj_expand.h", "zj_resize.h", "zj_geom.h", "emu_common/zj_emu_arena.h"),
                          "-O2", bind=_bind)


def run():
    return lib().zjck_run()


def batch():
    return lib().zjck_batch()


def params_bytes():
    return lib().zjck_params_bytes()


def combine(a_addrs, k_addrs, sizes, a_pitches, k_pitches, chw, inverted, arena, out_offsets, out_pitches, zeros=np.zeros):
    """The launches of one call: a_addrs / k_addrs = addresses of the images' and the planes' first bytes, sizes = (w, h),
    outputs at arena[out_offsets[i]:] at out_pitches[i].  Returns (write map of the arena, stores that fell outside it)."""
    # zeros: the allocator of the maps (far_cases.zeros for arenas of gigabytes: no huge pages)
    n = len(a_addrs)
    arr = lambda v: (C.c_uint * n)(*v)
    wh = (C.c_uint * (2 * n))(*[v for sz in sizes for v in sz])
    inv = (C.c_uint8 * n)(*[1 if v else 0 for v in inverted])
    outs = (C.c_void_p * n)(*[arena.ctypes.data + off for off in out_offsets])
    wmap = zeros(arena.size, np.uint8)
    outside = lib().zjck_combine(n, (C.c_void_p * n)(*a_addrs), (C.c_void_p * n)(*k_addrs), wh, arr(a_pitches), arr(k_pitches),
                                 1 if chw else 0, inv, outs, arr(out_pitches), C.c_void_p(arena.ctypes.data), arena.size,
                                 C.c_void_p(wmap.ctypes.data))
    assert outside >= 0, "the emulation refused its arguments"
    return wmap, outside
