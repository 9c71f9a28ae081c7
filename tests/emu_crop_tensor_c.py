"""ctypes binding of the CPU emulation of the crop-to-tensor kernels (tests/emu_crop_tensor).  TEST ONLY."""
import ctypes as C
import os

import numpy as np

import emu_build
import resize_model as rm

from emu_c import FrameDesc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None
ELEM = {rm.F32: 4, rm.F16: 2, rm.BF16: 2, rm.U8: 1}


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "emu_crop_tensor", "libzjemucroptensor.so")
        csrc = os.path.join(ROOT, "zune-jpeg_amd", "csrc")
        srcs = [os.path.join(HERE, "emu_crop_tensor", "zj_emu_crop_tensor.cpp")] + \
               [os.path.join(csrc, h) for h in ("zj_crop_tensor.h", "zj_resize.h", "zj_device.h", "zj_plan.h", "zj_geom.h")]
        emu_build.build(so, srcs, "-O1", extra=("-ffp-contract=off",))
        _LIB = C.CDLL(so)
        _LIB.zject_out_len.restype = C.c_size_t
        _LIB.zject_out_len.argtypes = [C.POINTER(FrameDesc), C.c_uint, C.c_uint, C.c_int]
    return _LIB


def out_len(d, w, h, dtype):
    return lib().zject_out_len(C.byref(d), w, h, dtype)


def decode_crops_tensor(d, frames, origins, w, h, dtype, layout="NCHW", scale=None, bias=None, flips=None, poison=0xAA,
                        stage_poison=0x5C, guard=64):
    """frames: list of [y, cb, cr] int16 arrays; returns (rc, buf) -- buf: the tensor's bytes (n images of out_len each), the
    whole of it poisoned first, with `guard` poisoned bytes in front of image 0 and behind the last checked untouched"""
    n = len(frames)
    ch = 1 if d.out_colorspace == 1 else 3
    arrs = [[np.ascontiguousarray(p, np.int16) for p in fr] + [np.zeros(8, np.int16)] * (3 - len(fr)) for fr in frames]
    ln = out_len(d, w, h, dtype)
    buf = np.full(n * max(ln, 1) + 2 * guard, poison, np.uint8)
    P = C.c_void_p * n
    ys, cbs, crs = P(*[a[0].ctypes.data for a in arrs]), P(*[a[1].ctypes.data for a in arrs]), P(*[a[2].ctypes.data for a in arrs])
    org = (C.c_uint * (2 * n))(*[int(v) for xy in origins for v in xy])
    s, b = rm.factors(ch, scale, bias)
    s3, b3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
    s3[:ch], b3[:ch] = s, b
    fl = None if flips is None else np.ascontiguousarray(np.asarray(flips, np.uint8))
    rc = lib().zject_decode_crops_tensor(C.byref(d), C.c_size_t(n), ys, cbs, crs, org, C.c_uint(w), C.c_uint(h), C.c_int(dtype),
                                         C.c_int(1 if layout == "NHWC" else 0), C.c_void_p(s3.ctypes.data),
                                         C.c_void_p(b3.ctypes.data), C.c_void_p(fl.ctypes.data if fl is not None else None),
                                         C.c_void_p(buf.ctypes.data + guard), C.c_int(stage_poison))
    assert (buf[:guard] == poison).all() and (buf[guard + n * ln:] == poison).all(), "the tensor call wrote outside the tensor"
    return rc, buf[guard:guard + n * ln]


def copyout_spans(rows, cuts, dtype, layout="NCHW", scale=None, bias=None, flip=False, poison=0xAA, guard=64):
    """crop_copyout_tensor by itself: rows = [h, w, 3] uint8 staged as one tile's rows, cut into spans at the byte offsets
    `cuts` (anywhere, inside a pixel too), one workgroup per span; returns (rc, the image's bytes, poisoned first)"""
    h, w, _ = rows.shape
    rows = np.ascontiguousarray(rows, np.uint8)
    ln = 3 * w * h * ELEM[dtype]
    buf = np.full(ln + 2 * guard, poison, np.uint8)
    s, b = rm.factors(3, scale, bias)
    cu = (C.c_int * max(len(cuts), 1))(*[int(c) for c in cuts])
    rc = lib().zject_copyout_spans(C.c_int(w), C.c_int(h), cu, C.c_int(len(cuts)), C.c_int(dtype), C.c_int(1 if layout == "NHWC" else 0),
                                   C.c_int(1 if flip else 0), C.c_void_p(s.ctypes.data), C.c_void_p(b.ctypes.data),
                                   C.c_void_p(rows.ctypes.data), C.c_void_p(buf.ctypes.data + guard))
    assert (buf[:guard] == poison).all() and (buf[guard + ln:] == poison).all(), "the copy-out wrote outside the image"
    return rc, buf[guard:guard + ln]


def decode_crops_tensor_mixed(descs, frames, origins, w, h, dtype, layout="NCHW", scale=None, bias=None, flips=None, poison=0xAA,
                              stage_poison=0x5C, guard=64):
    """the mixed-geometry call: descs = one FrameDesc per frame; otherwise as decode_crops_tensor"""
    n = len(frames)
    ch = 1 if descs[0].out_colorspace == 1 else 3
    arrs = [[np.ascontiguousarray(p, np.int16) for p in fr] + [np.zeros(8, np.int16)] * (3 - len(fr)) for fr in frames]
    ln = ch * w * h * ELEM.get(dtype, 0)
    buf = np.full(n * max(ln, 1) + 2 * guard, poison, np.uint8)
    P = C.c_void_p * n
    ys, cbs, crs = P(*[a[0].ctypes.data for a in arrs]), P(*[a[1].ctypes.data for a in arrs]), P(*[a[2].ctypes.data for a in arrs])
    org = (C.c_uint * (2 * n))(*[int(v) for xy in origins for v in xy])
    s, b = rm.factors(ch, scale, bias)
    s3, b3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
    s3[:ch], b3[:ch] = s, b
    fl = None if flips is None else np.ascontiguousarray(np.asarray(flips, np.uint8))
    darr = (FrameDesc * n)(*descs)
    rc = lib().zject_decode_crops_tensor_mixed(darr, C.c_size_t(n), ys, cbs, crs, org, C.c_uint(w), C.c_uint(h), C.c_int(dtype),
                                               C.c_int(1 if layout == "NHWC" else 0), C.c_void_p(s3.ctypes.data),
                                               C.c_void_p(b3.ctypes.data), C.c_void_p(fl.ctypes.data if fl is not None else None),
                                               C.c_void_p(buf.ctypes.data + guard), C.c_int(stage_poison))
    assert (buf[:guard] == poison).all() and (buf[guard + n * ln:] == poison).all(), "the tensor call wrote outside the tensor"
    return rc, buf[guard:guard + n * ln]
