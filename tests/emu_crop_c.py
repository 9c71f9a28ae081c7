"""ctypes binding of the CPU emulation of the crop-window kernels and plan (tests/emu_crop).  TEST ONLY."""
import ctypes as C
import os

import numpy as np

import emu_build

from emu_c import FrameDesc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "emu_crop", "libzjemucrop.so")
        srcs = [os.path.join(HERE, "emu_crop", "zj_emu_crop.cpp"),
                os.path.join(ROOT, "zune-jpeg_amd", "csrc", "zj_device.h"),
                os.path.join(ROOT, "zune-jpeg_amd", "csrc", "zj_plan.h"),
                os.path.join(ROOT, "zune-jpeg_amd", "csrc", "zj_geom.h")]

        emu_build.build(so, srcs, "-O1")
        _LIB = C.CDLL(so)
        _LIB.zjec_crop_out_len.restype = C.c_size_t
        _LIB.zjec_crop_out_len.argtypes = [C.POINTER(FrameDesc), C.c_uint, C.c_uint, C.c_uint]
    return _LIB


def desc(w, h, hs, vs, in_comp, out_cs, qts, flags=0, out_layout=0):
    d = FrameDesc()
    d.width, d.height, d.h_max, d.v_max, d.in_components, d.out_colorspace = w, h, hs, vs, in_comp, out_cs
    for c in range(3):
        q = np.asarray(qts[min(c, len(qts) - 1)], np.int32)
        for k in range(64):
            d.qt[c][k] = int(q[k])
    d.flags, d.out_layout, d.out_pitch = flags, out_layout, 0
    return d


def crop_out_len(d, w, h, out_pitch=0):
    return lib().zjec_crop_out_len(C.byref(d), w, h, out_pitch)


def decode_crops(d, frames, origins, w, h, out_pitch=0, poison=0xAA, stage_poison=0x5C, guard=64, outs=None):
    """frames: list of [y, cb, cr] int16 arrays; returns (rc, outs) -- outs[f] = the crop bytes (crop_out_len), with
    `guard` poisoned bytes in front and behind checked untouched.  outs: the caller's own buffers of crop_out_len bytes,
    decoded into as they are (a far pitch: gigabytes, committed as they are touched) and returned"""
    n = len(frames)
    arrs = [[np.ascontiguousarray(p, np.int16) for p in fr] + [np.zeros(8, np.int16)] * (3 - len(fr)) for fr in frames]
    ln = crop_out_len(d, w, h, out_pitch)
    if outs is not None:
        assert len(outs) == n and all(b.dtype == np.uint8 and b.size == ln and b.flags.c_contiguous for b in outs)
        bufs, guard = outs, 0
    else:
        bufs = [np.full(max(ln, 1) + 2 * guard, poison, np.uint8) for _ in range(n)]
    ptr = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    P = C.c_void_p * n
    ys, cbs, crs = P(*[a[0].ctypes.data for a in arrs]), P(*[a[1].ctypes.data for a in arrs]), P(*[a[2].ctypes.data for a in arrs])
    optr = P(*[b.ctypes.data + guard for b in bufs])
    org = (C.c_uint * (2 * n))(*[int(v) for xy in origins for v in xy])
    rc = lib().zjec_decode_crops(C.byref(d), C.c_size_t(n), ys, cbs, crs, org, C.c_uint(w), C.c_uint(h), optr,
                                 C.c_uint(out_pitch), C.c_int(stage_poison))
    if outs is not None:
        return rc, outs
    for b in bufs:
        assert (b[:guard] == poison).all() and (b[guard + ln:] == poison).all(), "a crop wrote outside its bytes"
    return rc, [b[guard:guard + ln] for b in bufs]


def crop_window(d, x, y, w, h):
    """(rc_or_tiles, (s0, s1, k0, k1), own[0 .. tiles])"""
    out4 = (C.c_int * 4)()
    own = (C.c_int * 4096)()
    rc = lib().zjec_crop_window(C.byref(d), x, y, w, h, out4, own, 4096)
    return rc, tuple(out4), list(own[:rc + 1]) if rc > 0 else []


def _row_bytes(d):
    ncomp = {0: 3, 1: 1, 2: 3, 5: 4, 6: 4}[d.out_colorspace]
    return d.width if (d.out_layout == 1 and ncomp == 3) else d.width * ncomp


def row_owners(d, planes, k_lo=0):
    """the brute-force write map of a frame row: (tiles or rc, owner[b] = the column that writes byte b, -1 nobody, -2 more
    than one, -3 not examined: left of column k_lo, whose columns are not decoded)"""
    arrs = [np.ascontiguousarray(p, np.int16) for p in planes] + [np.zeros(8, np.int16)] * (3 - len(planes))
    owner = np.zeros(_row_bytes(d), np.int32)
    rc = lib().zjec_row_owners(C.byref(d), C.c_void_p(arrs[0].ctypes.data), C.c_void_p(arrs[1].ctypes.data),
                               C.c_void_p(arrs[2].ctypes.data), C.c_int(k_lo), C.c_void_p(owner.ctypes.data))
    return rc, owner


def plan_owners(d):
    """the crop plan's owner of every byte of a frame row: (tiles or rc, owner[b], -1 no column, -2 more than one)"""
    owner = np.zeros(_row_bytes(d), np.int32)
    rc = lib().zjec_plan_owners(C.byref(d), C.c_void_p(owner.ctypes.data))
    return rc, owner
