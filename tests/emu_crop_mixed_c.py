"""ctypes binding of the CPU emulation of the mixed-geometry crop kernels and their tables (tests/emu_crop_mixed).  TEST ONLY."""
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
        so = os.path.join(HERE, "emu_crop_mixed", "libzjemucropmixed.so")
        csrc = os.path.join(ROOT, "zune-jpeg_amd", "csrc")
        srcs = [os.path.join(HERE, "emu_crop_mixed", "zj_emu_crop_mixed.cpp")] + \
            [os.path.join(csrc, h) for h in ("zj_mixed.h", "zj_rzgroup.h", "zj_device.h", "zj_scaled.h", "zj_plan.h", "zj_geom.h")]
        emu_build.build(so, srcs, "-O1")
        _LIB = C.CDLL(so)
        _LIB.zjem_record_bytes.restype = C.c_size_t
        _LIB.zjem_rz_groups.restype = C.c_size_t
    return _LIB


def _common(descs, windows, orientations):
    n = len(descs)
    da = (FrameDesc * n)(*descs)
    win = (C.c_uint * (4 * n))(*[int(v) for w in windows for v in w])
    ori = (C.c_uint8 * n)(*[int(o) for o in orientations]) if orientations is not None else None
    return n, da, win, ori


def plan(descs, windows, out_w, out_h, max_k=0, orientations=None):
    """(rc, per frame (k, (x, y, w, h) of the crop stage, orientation)): the checks of the planes entry point"""
    n, da, win, ori = _common(descs, windows, orientations)
    info = (C.c_int * (6 * n))()
    rc = lib().zjem_plan(da, C.c_size_t(n), win, C.c_uint(out_w), C.c_uint(out_h), C.c_int(max_k), ori, info)
    return rc, [(info[6 * f], tuple(info[6 * f + 1:6 * f + 5]), info[6 * f + 5]) for f in range(n)] if rc == 0 else []


def crop_bytes(d, w, h):
    ncomp = {0: 3, 1: 1, 2: 3}[d.out_colorspace]
    return w * h * ncomp


def crops(descs, frames, windows, out_w, out_h, max_k=0, orientations=None, poison=0xAA, lds_poison=0x5C, guard=64):
    """One emulated launch group.  frames: list of [y, cb, cr] int16 arrays.  Returns (rc, outs, plan, counts): outs[f] =
    frame f's tight crop, `guard` poisoned bytes in front and behind checked untouched; counts = (crop, reduced, zero)
    launches."""
    rc, pl = plan(descs, windows, out_w, out_h, max_k, orientations)
    n, da, win, ori = _common(descs, windows, orientations)
    arrs = [[np.ascontiguousarray(p, np.int16) for p in fr] + [np.zeros(64, np.int16)] * (3 - len(fr)) for fr in frames]
    lens = [crop_bytes(d, p[1][2], p[1][3]) for d, p in zip(descs, pl)] if rc == 0 else [16] * n
    bufs = [np.full(ln + 2 * guard, poison, np.uint8) for ln in lens]
    P = C.c_void_p * n
    ys, cbs, crs = P(*[a[0].ctypes.data for a in arrs]), P(*[a[1].ctypes.data for a in arrs]), P(*[a[2].ctypes.data for a in arrs])
    outs = P(*[b.ctypes.data + guard for b in bufs])
    counts = (C.c_int * 3)()
    rc = lib().zjem_crops(da, C.c_size_t(n), ys, cbs, crs, win, C.c_uint(out_w), C.c_uint(out_h), C.c_int(max_k), ori, outs,
                          C.c_int(lds_poison), counts)
    for b, ln in zip(bufs, lens):
        assert (b[:guard] == poison).all() and (b[guard + ln:] == poison).all(), "a crop wrote outside its bytes"
    return rc, [b[guard:guard + ln] for b, ln in zip(bufs, lens)], pl, tuple(counts)


def rz_groups(sizes, orientations, channels, chw, cap=0):
    """The library's group planner (zj_rzgroup.h) over crops of sizes[f] = (w, h) and orientations[f] at `cap` bytes (0: the
    library's RZ_GROUP_CAP).  Returns (need, groups): need = the scratch bytes of the call; groups = a list of (bytes, frames),
    frames = a list of (f, crop, read) with crop / read = (offset, w, h, pitch) of the crop and of the image the resize reads."""
    n = len(sizes)
    wh = (C.c_uint * (2 * n))(*[int(v) for s in sizes for v in s])
    ori = (C.c_uint8 * n)(*[int(o) for o in orientations])
    group, place, gbytes = (C.c_int * n)(), (C.c_ulonglong * (8 * n))(), (C.c_ulonglong * n)()
    need = lib().zjem_rz_groups(wh, ori, C.c_size_t(n), C.c_int(channels), C.c_int(1 if chw else 0), C.c_size_t(cap), group, place,
                                gbytes)
    groups = [(int(gbytes[g]), []) for g in range(group[n - 1] + 1)] if n else []
    for f in range(n):
        groups[group[f]][1].append((f, tuple(place[8 * f:8 * f + 4]), tuple(place[8 * f + 4:8 * f + 8])))
    return need, groups
