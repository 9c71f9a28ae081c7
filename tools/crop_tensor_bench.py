#!/usr/bin/env python3
"""Crop windows straight into a normalised tensor (zj_decode_crops_tensor_device) against the path that
existed before it: zj_decode_crops_resized_device with out == window (the u8 crops through the context's buffer, then a
resize that does nothing).  Both calls in ONE process, alternating, timed with device events after a warm-up; medians of
`--reps` rounds of `--iters` calls each.  The outputs are compared for equality first.

Two shapes, both 4:2:0 frames of 4096 x 4096 resident in HBM (synth.make_frame_t on the GPU), bf16 NCHW:
  windows   128 random 224 x 224 windows of 128 frames, ImageNet mean / std
  frames    16 whole frames
Each JSON line also holds the bytes the call must move, from the shapes alone: the tensor written once (new), or the u8 crop
written and read back plus the tensor (old); the coefficient planes under the tiles the windows touch are the same for both
and are left out.

  python tools/crop_tensor_bench.py [--iters 20] [--reps 7] [--out profiles/crop_tensor_bench.txt]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = H = 4096
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
PEAK = 8e12  # bytes / s of HBM, MI355X


def spread(ts):
    ts = sorted(ts)
    return {"min": round(ts[0], 4), "median": round(ts[len(ts) // 2], 4), "max": round(ts[-1], 4)}


def timed(torch, s, iters, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def shape(a, zj, torch, ctx, s, name, n, w, h, mean, std):
    import numpy as np
    synth = importlib.import_module("zune-jpeg_amd.synth")
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    frames, qts = [], None
    for i in range(n):
        planes, qts = synth.make_frame_t(W, H, 2, 2, 3, seed=1234, frame_index=i, device="cuda")
        frames.append(planes)
    d = zj.FrameDesc.make(W, H, 2, 2, 3, zj.ColorSpace.RGB, qts)
    rng = np.random.default_rng(13)
    origins = [(int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1))) for _ in range(n)]
    scale, bias = tensors.normalize_factors(3, mean, std)
    out_new = torch.empty((n, 3, h, w), dtype=torch.bfloat16, device="cuda")
    out_old = torch.empty_like(out_new)
    y, cb, cr = ([f[k].data_ptr() for f in frames] for k in range(3))
    wins = [(x, yy, w, h) for (x, yy) in origins]
    torch.cuda.synchronize()

    # The calls go to the library with their argument arrays built ONCE: at 0.1 ms of device time per call the Python wrappers'
    # four ctypes arrays of 128 entries each would be part of what is timed.
    import ctypes as C
    L, h_ctx, st = zj.lib(), ctx.handle, C.c_void_p(s.cuda_stream)
    vp = lambda v: (C.c_void_p * n)(*v)
    ay, acb, acr = vp(y), vp(cb), vp(cr)
    org = (C.c_uint * (2 * n))(*[v for xy in origins for v in xy])
    win = (C.c_uint * (4 * n))(*[v for wd in wins for v in wd])
    fs, fb = (C.c_float * 3)(*scale), (C.c_float * 3)(*bias)
    p_new, p_old = C.c_void_p(out_new.data_ptr()), C.c_void_p(out_old.data_ptr())
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    au8 = vp([u8.data_ptr() + i * h * w * 3 for i in range(n)])

    def new():
        rc = L.zj_decode_crops_tensor_device(h_ctx, C.byref(d), n, ay, acb, acr, org, w, h, zj.DTYPE_BF16, zj.TENSOR_NCHW, fs, fb,
                                             None, p_new, st)
        assert rc == 0, rc

    def old():
        rc = L.zj_decode_crops_resized_device(h_ctx, C.byref(d), n, ay, acb, acr, win, w, h, zj.DTYPE_BF16, zj.TENSOR_NCHW, fs, fb,
                                              None, p_old, st)
        assert rc == 0, rc

    def crop_u8():  # (for scale: the u8 crop alone, the first half of the old path)
        rc = L.zj_decode_crops_device(h_ctx, C.byref(d), n, ay, acb, acr, org, w, h, au8, 0, st)
        assert rc == 0, rc

    for _ in range(3):  # warm-up of all, and the comparison
        new()
        old()
        crop_u8()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_new.view(torch.uint8), out_old.view(torch.uint8)))
    t_new, t_old, t_u8 = [], [], []
    for _ in range(a.reps):
        t_new.append(timed(torch, s, a.iters, new))
        t_old.append(timed(torch, s, a.iters, old))
        t_u8.append(timed(torch, s, a.iters, crop_u8))
    px = n * w * h
    b_new, b_old = px * 6, px * (3 + 3 + 6)
    mn, mo = spread(t_new)["median"], spread(t_old)["median"]
    return {"shape": name, "what": f"{n} windows of {w}x{h} of {n} resident {W}x{H} 4:2:0 frames -> bf16 NCHW"
            + (", ImageNet mean / std" if mean is not None else ""), "iters": a.iters, "reps": a.reps, "outputs_equal": equal,
            "new_ms": spread(t_new), "identity_resize_ms": spread(t_old), "u8_crop_alone_ms": spread(t_u8), "old_over_new_median": round(mo / mn, 3),
            "bytes_new": b_new, "bytes_identity_resize": b_old,
            "new_tensor_share_of_8TBps": round(b_new / (mn * 1e-3) / PEAK, 4),
            "identity_resize_bytes_share_of_8TBps": round(b_old / (mo * 1e-3) / PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # (first: one HIP runtime in the process)
    zj = importlib.import_module("zune-jpeg_amd")
    ctx = zj.Context(zj.BACKEND_HIP, 0)  # raises without a GPU: there is nothing to measure on a CPU
    s = torch.cuda.Stream()
    lines = [f"# tools/crop_tensor_bench.py --iters {a.iters} --reps {a.reps}; device: {torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    ok = True
    for args in (("windows", 128, 224, 224, MEAN, STD), ("frames", 16, W, H, None, None)):
        r = shape(a, zj, torch, ctx, s, *args)
        ok = ok and r["outputs_equal"]
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
