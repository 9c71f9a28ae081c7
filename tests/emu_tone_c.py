"""ctypes binding of the CPU emulation of the tone stages' kernels (tests/emu_tone).  TEST ONLY."""
import ctypes as C

import numpy as np

import emu_build


def _bind(L):
    vp = C.c_void_p
    L.zjtn_hist.restype = C.c_longlong
    L.zjtn_hist.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_size_t, vp]
    L.zjtn_luts.argtypes = [C.c_int, C.c_int, vp, vp, vp]
    L.zjtn_lut.restype = C.c_longlong
    L.zjtn_lut.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp]


def lib():
    # -ffp-contract=off: autocontrast's product and sum are two roundings (zj_tone.h: tone_mul, tone_add)
    return emu_build.load("emu_tone", "libzjemutone.so", "zj_emu_tone.cpp",
                          ("zj_stage_pack.h", "zj_tone.h", "zj_tone_ops.h", "zj_cmyk.h", "zj_expand.h", "zj_resize.h", "zj_geom.h",
                           "emu_common/zj_emu_arena.h"), "-O2", extra=("-ffp-contract=off",), bind=_bind)


NAMES = ("run", "nt", "hist_runs", "hist_batch", "tone_lut_batch", "lut_batch", "hist_params", "tone_lut_params", "lut_params")


def const(name):
    return lib().zjtn_const(NAMES.index(name))


def op_valid(op, param):
    return bool(lib().zjtn_op_valid(op, param))


def _images(n, sizes, pitches):
    wh = (C.c_uint * (2 * n))(*[v for sz in sizes for v in sz])
    return wh, (C.c_uint * n)(*pitches)


def hist(src, offsets, sizes, pitches, channels, chw):
    """The launches of one histogram call: images at src[offsets[i]:], sizes = (w, h).  Returns (int64 [n, channels, 256],
    read map of src, loads that fell outside it)."""
    n = len(sizes)
    wh, pit = _images(n, sizes, pitches)
    ins = (C.c_void_p * n)(*[src.ctypes.data + off for off in offsets])
    out = np.full((n, channels, 256), 0xA5A5A5A5, np.uint32)
    rmap = np.zeros(src.size, np.uint8)
    outside = lib().zjtn_hist(n, ins, wh, pit, channels, 1 if chw else 0, C.c_void_p(out.ctypes.data), C.c_void_p(src.ctypes.data),
                              src.size, C.c_void_p(rmap.ctypes.data))
    assert outside >= 0, "the emulation refused its arguments"
    return out.astype(np.int64), rmap, outside


def luts(ops, channels, hist_bins):
    """the tables of the ops over hist_bins ([n, channels, 256] below 2^32, or None) as uint8 [n, channels, 256]; None: refused"""
    n = len(ops)
    flat = (C.c_int32 * (2 * n))(*[int(v) for op in ops for v in op])
    h = np.ascontiguousarray(np.asarray(hist_bins, np.uint64).astype(np.uint32).reshape(n, channels, 256)) if hist_bins is not None else None
    out = np.full((n, channels, 256), 0xA5, np.uint8)
    rc = lib().zjtn_luts(n, channels, flat, C.c_void_p(h.ctypes.data) if h is not None else None, C.c_void_p(out.ctypes.data))
    return out if rc == 0 else None


def lut(src, in_offsets, sizes, in_pitches, channels, chw, tables, arena, out_offsets, out_pitches):
    """The launches of one lookup call: inputs at src[in_offsets[i]:] (src may be the arena: in place), tables uint8
    [n, channels, 256], outputs at arena[out_offsets[i]:].  Returns (read map of src, write map of the arena, loads and
    stores that fell outside them)."""
    n = len(sizes)
    wh, ip = _images(n, sizes, in_pitches)
    op = (C.c_uint * n)(*out_pitches)
    ins = (C.c_void_p * n)(*[src.ctypes.data + off for off in in_offsets])
    outs = (C.c_void_p * n)(*[arena.ctypes.data + off for off in out_offsets])
    t = np.ascontiguousarray(tables, np.uint8)
    assert t.shape == (n, channels, 256)
    rmap, wmap = np.zeros(src.size, np.uint8), np.zeros(arena.size, np.uint8)
    outside = lib().zjtn_lut(n, ins, wh, ip, channels, 1 if chw else 0, C.c_void_p(t.ctypes.data), outs, op, C.c_void_p(src.ctypes.data),
                             src.size, C.c_void_p(rmap.ctypes.data), C.c_void_p(arena.ctypes.data), arena.size, C.c_void_p(wmap.ctypes.data))
    assert outside >= 0, "the emulation refused its arguments"
    return rmap, wmap, outside
