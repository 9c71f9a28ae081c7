"""ctypes binding of the CPU emulation of the fused tile kernel with the interior form of its colour rounds
(tests/emu_interior), built once with -DZJ_INTERIOR=1 and once with -DZJ_INTERIOR=0.  TEST ONLY."""
import ctypes as C
import os

import numpy as np

import emu_build
from emu_c import FrameDesc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIBS = {}
GENERAL, INTERIOR, REDO, DIRECT = 0, 1, 2, 3   # how a tile's colour phase went (zjc_ways)


def lib(knob):
    if knob not in _LIBS:
        so = os.path.join(HERE, "emu_interior", f"libzjemuinterior{knob}.so")
        csrc = os.path.join(ROOT, "zune-jpeg_amd", "csrc")
        srcs = [os.path.join(HERE, "emu_interior", "zj_emu_interior.cpp")] + [os.path.join(csrc, h) for h in ("zj_device.h", "zj_plan.h", "zj_geom.h")]
        emu_build.build(so, srcs, "-O1", extra=(f"-DZJ_INTERIOR={knob}",))
        _LIBS[knob] = C.CDLL(so)
        assert _LIBS[knob].zjc_knob() == knob
    return _LIBS[knob]


def decode_planes(knob, frame, planes, flags=0, out_pitch=0, zero_fill=1, poison=0xAA):
    """frame: the oracle's zjo_frame; flags / out_pitch: the extension fields of zj_frame_desc.  The output buffer starts
    as `poison`.  Returns (rc, rows (height, pitch), {(strip, tile): way})."""
    L = lib(knob)
    arrs = [np.ascontiguousarray(p, np.int16) for p in planes]
    d = FrameDesc()
    for name in ("width", "height", "h_max", "v_max", "in_components", "out_colorspace"):
        setattr(d, name, getattr(frame, name))
    C.memmove(d.qt, frame.qt, 3 * 64 * 4)
    d.flags, d.out_layout, d.out_pitch = flags, 0, out_pitch
    ncomp = {0: 3, 2: 3, 5: 4}[d.out_colorspace]
    pitch = out_pitch or d.width * ncomp
    out = np.full(pitch * d.height, poison, np.uint8)
    rc = L.zjc_decode_planes(C.byref(d), C.c_size_t(1), C.c_void_p(arrs[0].ctypes.data), C.c_void_p(arrs[1].ctypes.data),
                             C.c_void_p(arrs[2].ctypes.data), C.c_void_p(out.ctypes.data), C.c_int(zero_fill))
    L.zjc_tiles.restype = C.c_longlong
    n = int(L.zjc_tiles())
    ways = np.zeros((n, 4), np.int32)
    if n:
        L.zjc_ways(C.c_void_p(ways.ctypes.data))
    assert len({(s, t) for _, s, t, _ in ways.tolist()}) == n, "a tile decoded twice"
    return rc, out.reshape(d.height, pitch), {(s, t): w for _, s, t, w in ways.tolist()}
