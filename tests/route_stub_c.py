"""ctypes binding of the routing stub (tests/route_stub): the front-end zj_jpeg.cpp over stand-ins for everything it calls
outside itself, which launch nothing and record who was called for which file.  The prototypes and zj_options come from
include/zjhip.h through abi_types, not from zune-jpeg_amd/host.py (which binds libzjhip.so).  TEST ONLY."""
import ctypes as C
import glob
import os

import abi_types as at
import emu_build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = open(os.path.join(ROOT, "include", "zjhip.h")).read()
_SCALAR = {"c_int": C.c_int, "c_uint": C.c_uint, "usize": C.c_size_t, "f32": C.c_float, "f64": C.c_double, "i32": C.c_int32,
           "u32": C.c_uint32, "i64": C.c_int64, "u8": C.c_uint8, "u16": C.c_uint16, "i16": C.c_int16}
_LIB = None


def _ctype(t):
    base, chain = t
    if chain:
        return C.c_char_p if (base, len(chain)) == ("c_char", 1) else C.c_void_p
    return None if base == "c_void" else _SCALAR[base]


class Options(C.Structure):  # zj_options, field for field as the header declares it
    _fields_ = [(name, _SCALAR[base]) for name, base, dims in at.c_structs(HDR)["zj_options"]]


def status(name):
    import re
    return int(re.search(r"\b%s\s*=\s*(-?\d+)" % name, HDR).group(1))


def flag(name):
    import re
    return int(re.search(r"#define\s+%s\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?" % name, HDR).group(1), 0)


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "route_stub", "libzjroutestub.so")
        csrc = os.path.join(ROOT, "zune-jpeg_amd", "csrc")
        srcs = [os.path.join(HERE, "route_stub", "zj_route_stub.cpp"), os.path.join(csrc, "zj_jpeg.cpp"),
                os.path.join(ROOT, "include", "zjhip.h")] + sorted(glob.glob(os.path.join(csrc, "*.h")))
        emu_build.build(so, srcs, "-O1", extra=("-pthread", "-Wno-subobject-linkage"))
        L = C.CDLL(so)
        for name, (ret, args) in at.c_prototypes(HDR).items():
            if name.startswith("zj_decoder_"):
                f = getattr(L, name)
                f.restype = _ctype(ret)
                f.argtypes = [_ctype(a) for a in args]
        L.zjrs_begin.restype = None
        L.zjrs_begin.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int]
        L.zjrs_count.restype = C.c_size_t
        L.zjrs_name.restype = C.c_char_p
        L.zjrs_name.argtypes = [C.c_size_t]
        L.zjrs_file.restype = C.c_long
        L.zjrs_file.argtypes = [C.c_size_t]
        L.zjrs_nframes.restype = C.c_long
        L.zjrs_nframes.argtypes = [C.c_size_t]
        _LIB = L
    return _LIB


def begin(base, img, n, fail_nth=0, scan_rc=0):
    """start recording a batch whose output is n images of img bytes at address base; fail_nth: the n-th *_mixed_host
    call returns ZJ_ERR_HIP; scan_rc: what the entropy-stage stand-ins return"""
    lib().zjrs_begin(base, img, n, fail_nth, scan_rc)


def log():
    """[(stub name, file index or -1, nframes)] in call order"""
    L = lib()
    return [(L.zjrs_name(i).decode(), int(L.zjrs_file(i)), int(L.zjrs_nframes(i))) for i in range(L.zjrs_count())]
