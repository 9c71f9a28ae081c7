"""ctypes binding of the CPU emulation of the planes-to-RGB kernel (tests/emu_planes).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    L.zjpl_combine.restype = C.c_longlong
    L.zjpl_bad_reads.restype = C.c_longlong
    L.zjpl_combine.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


def lib():
    return emu_build.load("emu_planes", "libzjemuplanes.so", "zj_emu_planes.cpp",
                          ("zj_stage_pack.h", "zj_planes.h", "zj_expand.h", "zj_resize.h", "zj_geom.h", "emu_common/zj_emu_arena.h"),
                          "-O2", bind=_bind)


def run():
    return lib().zjpl_run()


def batch():
    return lib().zjpl_batch()


def params_bytes():
    return lib().zjpl_params_bytes()


def combine(src, needed, plane_offsets, plane_pitches, sizes, geos, stored_rgb, chw, arena, out_offsets, out_pitches, zeros=np.zeros):
    """The launches of one call: planes at src[plane_offsets[i][c]:] at plane_pitches[i][c], sizes = (w, h) of the outputs,
    geos = ((rx, ry, px, py) x 3) each, outputs at arena[out_offsets[i]:] at out_pitches[i]; needed = the bytes of src that may
    be read.  Returns (write map of the arena, stores that fell outside it, loads that touched a byte not needed)."""
    # zeros: the allocator of the maps (far_cases.zeros for arenas of gigabytes: no huge pages)
    n = len(sizes)
    planes = (C.c_void_p * (3 * n))(*[src.ctypes.data + o for offs in plane_offsets for o in offs])
    pit = (C.c_uint * (3 * n))(*[p for ps in plane_pitches for p in ps])
    wh = (C.c_uint * (2 * n))(*[v for sz in sizes for v in sz])
    geo = (C.c_uint8 * (12 * n))(*[v for g in geos for comp in g for v in comp])
    outs = (C.c_void_p * n)(*[arena.ctypes.data + off for off in out_offsets])
    opit = (C.c_uint * n)(*out_pitches)
    wmap = zeros(arena.size, np.uint8)
    need = np.ascontiguousarray(needed, np.uint8)
    outside = lib().zjpl_combine(n, planes, pit, wh, geo, 1 if stored_rgb else 0, 1 if chw else 0, outs, opit,
                                 C.c_void_p(arena.ctypes.data), arena.size, C.c_void_p(wmap.ctypes.data),
                                 C.c_void_p(src.ctypes.data), src.size, C.c_void_p(need.ctypes.data))
    assert outside >= 0, "the emulation refused its arguments"
    return wmap, outside, lib().zjpl_bad_reads()
