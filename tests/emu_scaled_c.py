"""ctypes binding of the CPU emulation of the reduced-size decode's kernel and plan (tests/emu_scaled).  TEST ONLY."""
import ctypes as C
import os

import numpy as np

import emu_build

from emu_c import FrameDesc
from emu_crop_c import desc  # noqa: F401  (the same descriptor helper)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "emu_scaled", "libzjemuscaled.so")
        csrc = os.path.join(ROOT, "zune-jpeg_amd", "csrc")
        srcs = [os.path.join(HERE, "emu_scaled", "zj_emu_scaled.cpp"), os.path.join(csrc, "zj_device.h"),
                os.path.join(csrc, "zj_scaled.h"), os.path.join(csrc, "zj_plan.h"), os.path.join(csrc, "zj_geom.h")]

        emu_build.build(so, srcs, "-O1")
        _LIB = C.CDLL(so)
        _LIB.zjes_out_len.restype = C.c_size_t
        _LIB.zjes_out_len.argtypes = [C.POINTER(FrameDesc), C.c_int, C.c_uint, C.c_uint, C.c_uint]
        _LIB.zjes_prescale_pick.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int]
        _LIB.zjes_prescale_window.restype = None
    return _LIB


def scaled_size(d, sl):
    w, h = C.c_uint(0), C.c_uint(0)
    rc = lib().zjes_scaled_size(C.byref(d), C.c_int(sl), C.byref(w), C.byref(h))
    return rc, w.value, h.value


def out_len(d, sl, w, h, out_pitch=0):
    return lib().zjes_out_len(C.byref(d), sl, w, h, out_pitch)


def decode(d, frames, sl, windows=None, out_pitch=0, poison=0xAA, lds_poison=0x5C, guard=64, outs=None):
    """frames: list of [y, cb, cr] int16 arrays; windows: None (whole reduced frames) or one (x, y, w, h) per frame in
    reduced pixels.  Returns (rc, outs): outs[f] = the crop's bytes, `guard` poisoned bytes in front and behind checked
    untouched.  outs: the caller's own buffers of out_len bytes each, decoded into as they are (a far pitch: gigabytes,
    committed as they are touched) and returned."""
    n = len(frames)
    arrs = [[np.ascontiguousarray(p, np.int16) for p in fr] + [np.zeros(64, np.int16)] * (3 - len(fr)) for fr in frames]
    _, rw, rh = scaled_size(d, sl)
    wins = windows if windows is not None else [(0, 0, rw, rh)] * n
    lens = [out_len(d, sl, w[2], w[3], out_pitch) for w in wins]
    if outs is not None:
        assert len(outs) == n and all(b.dtype == np.uint8 and b.size == ln and b.flags.c_contiguous for b, ln in zip(outs, lens))
        bufs, guard = outs, 0
    else:
        bufs = [np.full(max(ln, 1) + 2 * guard, poison, np.uint8) for ln in lens]
    P = C.c_void_p * n
    ys, cbs, crs = P(*[a[0].ctypes.data for a in arrs]), P(*[a[1].ctypes.data for a in arrs]), P(*[a[2].ctypes.data for a in arrs])
    optr = P(*[b.ctypes.data + guard for b in bufs])
    win = (C.c_uint * (4 * n))(*[int(v) for w in wins for v in w]) if windows is not None else None
    rc = lib().zjes_decode(C.byref(d), C.c_size_t(n), ys, cbs, crs, C.c_int(sl), win, optr, C.c_uint(out_pitch), C.c_int(lds_poison))
    if outs is not None:
        return rc, outs
    for b, ln in zip(bufs, lens):
        assert (b[:guard] == poison).all() and (b[guard + ln:] == poison).all(), "a crop wrote outside its bytes"
    return rc, [b[guard:guard + ln] for b, ln in zip(bufs, lens)]


def prescale_pick(w, h, out_w, out_h, max_log2):
    return lib().zjes_prescale_pick(w, h, out_w, out_h, max_log2)


def prescale_window(x, y, w, h, k, width, height):
    full = (C.c_uint * 4)(x, y, w, h)
    red = (C.c_uint * 4)()
    lib().zjes_prescale_window(full, C.c_int(k), C.c_uint(width), C.c_uint(height), red)
    return tuple(red)
