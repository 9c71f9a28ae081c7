#!/usr/bin/env python3
"""u8 images in HBM into a normalised tensor, not resized (zj_to_tensor_device) against the path these images
took before it: zj_resize_device with out == in (a resize that does nothing); and, for one-channel images shown in three
channels, against zj_gray_to_rgb_device followed by that resize.  Both paths in ONE process, alternating, timed with device
events after a warm-up; medians of `--reps` rounds of `--iters` calls each.  The outputs are compared for equality first.

Shapes, all tight u8 images resident in HBM, bf16 NCHW, ImageNet mean / std:
  rgb224     128 RGB images of 224 x 224
  rgb4096    16 RGB images of 4096 x 4096
  gray224    128 one-channel images of 224 x 224 into three channels
  gray4096   16 one-channel images of 4096 x 4096 into three channels
Each JSON line also holds the bytes each path must move, from the shapes alone: per pixel 3 B read + 6 B written for RGB on
both paths; for gray 1 B + 6 B (new) against 1 B + 3 B written + 3 B read + 6 B (expand, then resize).

  python tools/to_tensor_bench.py [--iters 20] [--reps 7] [--out profiles/to_tensor_bench.txt]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def shape(a, zj, torch, ctx, s, name, n, w, h, cin):
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    g = torch.Generator(device="cuda").manual_seed(17)
    src = torch.randint(0, 256, (n, h, w, cin), dtype=torch.uint8, device="cuda", generator=g)
    scale, bias = tensors.normalize_factors(3, MEAN, STD)
    out_new = torch.empty((n, 3, h, w), dtype=torch.bfloat16, device="cuda")
    out_old = torch.empty_like(out_new)
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda") if cin == 1 else src
    torch.cuda.synchronize()
    # (the argument arrays built ONCE: the Python wrappers' ctypes arrays would be part of what is timed)
    L, h_ctx, st = zj.lib(), ctx.handle, C.c_void_p(s.cuda_stream)
    vp = lambda t: (C.c_void_p * n)(*[t.data_ptr() + i * t[0].numel() for i in range(n)])
    a_src, a_rgb = vp(src), vp(rgb)
    wh = (C.c_uint * (2 * n))(*([w, h] * n))
    fs, fb = (C.c_float * 3)(*scale), (C.c_float * 3)(*bias)
    p_new, p_old = C.c_void_p(out_new.data_ptr()), C.c_void_p(out_old.data_ptr())

    def new():
        rc = L.zj_to_tensor_device(h_ctx, n, a_src, w, h, None, cin, 3, zj.DTYPE_BF16, zj.TENSOR_NCHW, fs, fb, None, p_new, st)
        assert rc == 0, rc

    def old():
        if cin == 1:
            rc = L.zj_gray_to_rgb_device(h_ctx, n, a_src, wh, None, zj.LAYOUT_HWC, a_rgb, None, st)
            assert rc == 0, rc
        rc = L.zj_resize_device(h_ctx, n, a_rgb, wh, None, 3, zj.LAYOUT_HWC, w, h, zj.DTYPE_BF16, zj.TENSOR_NCHW, fs, fb, None, p_old, st)
        assert rc == 0, rc

    for _ in range(3):  # warm-up of both, and the comparison
        new()
        old()
    torch.cuda.synchronize()
    equal = bool(torch.equal(out_new.view(torch.uint8), out_old.view(torch.uint8)))
    t_new, t_old = [], []
    for _ in range(a.reps):
        t_new.append(timed(torch, s, a.iters, new))
        t_old.append(timed(torch, s, a.iters, old))
    px = n * w * h
    b_new, b_old = px * (cin + 6), px * (3 + 6) + (px * (1 + 3) if cin == 1 else 0)
    mn, mo = spread(t_new)["median"], spread(t_old)["median"]
    return {"shape": name, "what": f"{n} u8 images of {w}x{h}, {cin} channel(s) -> bf16 NCHW, 3 channels, ImageNet mean / std",
            "iters": a.iters, "reps": a.reps, "outputs_equal": equal, "to_tensor_ms": spread(t_new),
            ("expand_then_identity_resize_ms" if cin == 1 else "identity_resize_ms"): spread(t_old),
            "old_over_new_median": round(mo / mn, 3), "bytes_to_tensor": b_new, "bytes_old_path": b_old,
            "to_tensor_share_of_8TBps": round(b_new / (mn * 1e-3) / PEAK, 4),
            "old_path_share_of_8TBps": round(b_old / (mo * 1e-3) / PEAK, 4)}


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
    lines = [f"# tools/to_tensor_bench.py --iters {a.iters} --reps {a.reps}; device: {torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    ok = True
    for args in (("rgb224", 128, 224, 224, 3), ("rgb4096", 16, 4096, 4096, 3), ("gray224", 128, 224, 224, 1), ("gray4096", 16, 4096, 4096, 1)):
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
