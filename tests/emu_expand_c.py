"""ctypes binding of the CPU emulation of the gray-to-RGB kernel (tests/emu_expand).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    L.zjex_expand.restype = C.c_longlong
    L.zjex_expand.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_size_t, C.c_void_p]


def lib():
    return emu_build.load("emu_expand", "libzjemuexpand.so", "zj_emu_expand.cpp",
                          ("zj_stage_pack.h", "zj_expand.h", "zj_resize.h", "zj_geom.h", "emu_common/zj_emu_arena.h"),
                          "-O2", bind=_bind)


def run():
    return lib().zjex_run()


def batch():
    return lib().zjex_batch()


def params_bytes():
    return lib().zjex_params_bytes()


def expand(in_addrs, sizes, in_pitches, out_chw, arena, out_offsets, out_pitches, zeros=np.zeros):
    """The launches of one call: in_addrs = addresses of the planes' first bytes, sizes = (w, h), outputs at
    arena[out_offsets[i]:] at out_pitches[i].  Returns (write map of the arena, stores that fell outside it)."""
    # zeros: the allocator of the maps (far_cases.zeros for arenas of gigabytes: no huge pages)
    n = len(in_addrs)
    ins = (C.c_void_p * n)(*in_addrs)
    wh = (C.c_uint * (2 * n))(*[v for sz in sizes for v in sz])
    ip = (C.c_uint * n)(*in_pitches)
    op = (C.c_uint * n)(*out_pitches)
    outs = (C.c_void_p * n)(*[arena.ctypes.data + off for off in out_offsets])
    wmap = zeros(arena.size, np.uint8)
    outside = lib().zjex_expand(n, ins, wh, ip, 1 if out_chw else 0, outs, op, C.c_void_p(arena.ctypes.data), arena.size,
                                C.c_void_p(wmap.ctypes.data))
    assert outside >= 0, "the emulation refused its arguments"
    return wmap, outside
