"""ctypes binding of the resized-crop calls' launch-group planner with gray-to-RGB frames (tests/emu_rzgroup).  TEST ONLY."""
import ctypes as C
import os

import emu_build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "emu_rzgroup", "libzjemurzgroup.so")
        csrc = os.path.join(ROOT, "zune-jpeg_amd", "csrc")
        srcs = [os.path.join(HERE, "emu_rzgroup", "zj_emu_rzgroup.cpp"), os.path.join(csrc, "zj_rzgroup.h"),
                os.path.join(csrc, "zj_geom.h")]
        emu_build.build(so, srcs, "-O2")
        _LIB = C.CDLL(so)
        _LIB.zjer_groups.restype = C.c_size_t
    return _LIB


def groups(sizes, orientations, gray, channels, chw, cap=0):
    """The planner over crops of sizes[f] = (w, h), orientations[f] and gray[f] (None: frames built without the member) at
    `cap` bytes (0: the library's).  Returns (need, groups): need = the scratch bytes of the call; groups = a list of
    (bytes, frames), frames = a list of dicts f, crop, gray, read (each (offset, w, h, pitch)), turned, expand."""
    n = len(sizes)
    wh = (C.c_uint * (2 * n))(*[int(v) for s in sizes for v in s])
    ori = (C.c_uint8 * n)(*[int(o) for o in orientations])
    gr = (C.c_uint8 * n)(*[int(g) for g in gray]) if gray is not None else None
    group, place, gbytes = (C.c_int * n)(), (C.c_ulonglong * (16 * n))(), (C.c_ulonglong * n)()
    need = lib().zjer_groups(wh, ori, gr, C.c_size_t(n), C.c_int(channels), C.c_int(1 if chw else 0), C.c_size_t(cap), group, place,
                             gbytes)
    out = [(int(gbytes[g]), []) for g in range(group[n - 1] + 1)] if n else []
    for f in range(n):
        p = [int(v) for v in place[16 * f:16 * f + 16]]
        out[group[f]][1].append({"f": f, "crop": tuple(p[0:4]), "gray": tuple(p[4:8]), "read": tuple(p[8:12]),
                                 "turned": bool(p[12]), "expand": bool(p[13])})
    return need, out
