"""ctypes binding of the CPU emulation of the colour-matrix kernel (tests/emu_color).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    L.zjcl_color.restype = C.c_longlong
    L.zjcl_color.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.zjcl_fixed.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int32)]


def lib():
    return emu_build.load("emu_color", "libzjemucolor.so", "zj_emu_color.cpp",
                          ("zj_stage_pack.h", "zj_color.h", "zj_color_fixed.h", "zj_cmyk.h", "zj_expand.h", "zj_resize.h", "zj_geom.h", "emu_common/zj_emu_arena.h"),
                          "-O2", bind=_bind)


def run():
    return lib().zjcl_run()


def batch():
    return lib().zjcl_batch()


def params_bytes():
    return lib().zjcl_params_bytes()


def fixed(m):
    """zj_color_fixed.h's color_fixed: the 12 integers, or None"""
    q = (C.c_int32 * 12)()
    ok = lib().zjcl_fixed((C.c_double * 12)(*[float(v) for v in np.asarray(m, np.float64).reshape(12)]), q)
    return [int(v) for v in q] if ok else None


def color(src, in_offsets, sizes, in_pitches, chw, qs, arena, out_offsets, out_pitches, zeros=np.zeros):
    """The launches of one call: inputs at src[in_offsets[i]:] (src may be the arena: in place), sizes = (w, h), qs = 12
    integers each, outputs at arena[out_offsets[i]:].  Returns (read map of src, write map of the arena, loads and stores that
    fell outside them)."""
    # zeros: the allocator of the maps (far_cases.zeros for arenas of gigabytes: no huge pages)
    n = len(sizes)
    arr = lambda v: (C.c_uint * n)(*v)
    wh = (C.c_uint * (2 * n))(*[v for sz in sizes for v in sz])
    q = (C.c_int32 * (12 * n))(*[v for one in qs for v in one])
    ins = (C.c_void_p * n)(*[src.ctypes.data + off for off in in_offsets])
    outs = (C.c_void_p * n)(*[arena.ctypes.data + off for off in out_offsets])
    rmap, wmap = zeros(src.size, np.uint8), zeros(arena.size, np.uint8)
    outside = lib().zjcl_color(n, ins, wh, arr(in_pitches), 1 if chw else 0, q, outs, arr(out_pitches), C.c_void_p(src.ctypes.data),
                               src.size, C.c_void_p(rmap.ctypes.data), C.c_void_p(arena.ctypes.data), arena.size,
                               C.c_void_p(wmap.ctypes.data))
    assert outside >= 0, "the emulation refused its arguments"
    return rmap, wmap, outside
