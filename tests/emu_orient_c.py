"""ctypes binding of the CPU emulation of the orientation kernel (tests/emu_orient).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    L.zjeo_orient.restype = C.c_longlong
    L.zjeo_orient.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.zjeo_lds_bytes.argtypes = [C.c_int]


def lib():
    return emu_build.load("emu_orient", "libzjemuorient.so", "zj_emu_orient.cpp",
                          ("zj_stage_pack.h", "zj_orient.h", "zj_resize.h", "zj_geom.h", "emu_common/zj_emu_arena.h"),
                          "-O2", bind=_bind)


def tile():
    return lib().zjeo_tile()


def batch():
    return lib().zjeo_batch()


def orient(images, sizes, in_pitches, channels, in_chw, orientations, arena, out_offsets, out_pitches, zeros=np.zeros):
    """One launch: images = uint8 buffers (each in its layout at its pitch), sizes = STORED (w, h), outputs at
    arena[out_offsets[i]:] at out_pitches[i].  Returns (write map of the arena, stores that fell outside it)."""
    # zeros: the allocator of the maps (far_cases.zeros for arenas of gigabytes: no huge pages)
    n = len(images)
    ins = (C.c_void_p * n)(*[im.ctypes.data for im in images])
    wh = (C.c_uint * (2 * n))(*[v for sz in sizes for v in sz])
    ip = (C.c_uint * n)(*in_pitches)
    op = (C.c_uint * n)(*out_pitches)
    oo = (C.c_uint8 * n)(*orientations)
    outs = (C.c_void_p * n)(*[arena.ctypes.data + off for off in out_offsets])
    wmap = zeros(arena.size, np.uint8)
    outside = lib().zjeo_orient(n, ins, wh, ip, channels, 1 if in_chw else 0, oo, outs, op, C.c_void_p(arena.ctypes.data),
                                arena.size, C.c_void_p(wmap.ctypes.data))
    assert outside >= 0, "the emulation refused its arguments"
    return wmap, outside
