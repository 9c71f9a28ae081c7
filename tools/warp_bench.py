#!/usr/bin/env python3
"""Affine-warped images into a normalised tensor (zj_warp_device) next to the two stages it reduces to, and
the warped batch file call next to what a caller did before it.  Everything in ONE process, alternating, timed with device events
(the file part with the host clock around synchronous calls) after a warm-up; medians of `--reps` rounds of `--iters` calls.
No threshold is asserted: the numbers are what the profile records.

Stage: 128 tight RGB u8 images of 256 x 256 resident in HBM -> 224 x 224 bf16 NCHW, ImageNet mean / std, fill 0:
  identity      the matrix (1, 0, 16, 0, 1, 16): the centre 224 x 224, no interpolation
  rot15, rot45, rot90   about the image's centre, scale 1
  half          scale 1/2 about the centre: the output sees 448 x 448 source pixels, most of them outside (fill)
beside, on the same inputs: zj_resize_device bilinear 256 -> 224, and zj_to_tensor_device of the images' centre 224 x 224.
Files: `--files` JPEG files of 512 x 384 (4:2:0, made here), each rotated by its own angle about its centre into 224 x 224:
  warped        tensors.decode_files_warped_to_tensor, on zj_decoder_finish_pixels_warped_batch_device (only the part of each
                frame the output sees is decoded)
  grid_sample   the whole frame decoded by the library into a u8 tensor, then torch: float conversion, normalisation, affine_grid
                in pixel units and F.grid_sample (bilinear, zeros, align_corners=False) in bf16

  python tools/warp_bench.py [--iters 20] [--reps 7] [--files 64] [--out profiles/warp.txt]"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


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


def stage(a, zj, tz, torch, ctx, s):
    n, w, h, ow, oh = 128, 256, 256, 224, 224
    g = torch.Generator(device="cuda").manual_seed(17)
    src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    scale, bias = tz.normalize_factors(3, MEAN, STD)
    out = torch.empty((n, 3, oh, ow), dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    L, hc, st = zj.lib(), ctx.handle, C.c_void_p(s.cuda_stream)
    ptrs = (C.c_void_p * n)(*[src.data_ptr() + i * src[0].numel() for i in range(n)])
    centre = (C.c_void_p * n)(*[src.data_ptr() + i * src[0].numel() + (16 * w + 16) * 3 for i in range(n)])
    pitch = (C.c_uint * n)(*([3 * w] * n))
    wh = (C.c_uint * (2 * n))(*([w, h] * n))
    fs, fb = (C.c_float * 3)(*scale), (C.c_float * 3)(*bias)
    po = C.c_void_p(out.data_ptr())
    cases = {"identity": (1.0, 0.0, 16.0, 0.0, 1.0, 16.0), "half": tz.warp_matrix((ow, oh), (w / 2, h / 2), scale=0.5)}
    for ang in (15, 45, 90):
        cases[f"rot{ang}"] = tz.warp_matrix((ow, oh), (w / 2, h / 2), angle=ang)

    def warp(m):
        ms = (C.c_double * (6 * n))(*(list(m) * n))

        def run():
            rc = L.zj_warp_device(hc, n, ptrs, wh, None, 3, ms, ow, oh, zj.DTYPE_BF16, zj.TENSOR_NCHW, fs, fb, None, zj.WARP_FILL, po, st)
            assert rc == 0, rc
        return run

    def resize():
        rc = L.zj_resize_device(hc, n, ptrs, wh, None, 3, zj.LAYOUT_HWC, ow, oh, zj.DTYPE_BF16, zj.TENSOR_NCHW, fs, fb, None, po, st)
        assert rc == 0, rc

    def to_tensor():
        rc = L.zj_to_tensor_device(hc, n, centre, ow, oh, pitch, 3, 3, zj.DTYPE_BF16, zj.TENSOR_NCHW, fs, fb, None, po, st)
        assert rc == 0, rc

    fns = {f"warp_{k}": warp(m) for k, m in cases.items()}
    fns["resize_bilinear_256_to_224"] = resize
    fns["to_tensor_centre_224"] = to_tensor
    # the identity against the to-tensor stage of the same window: equal bytes
    fns["warp_identity"]()
    torch.cuda.synchronize()
    ident = out.clone()
    to_tensor()
    torch.cuda.synchronize()
    equal = bool(torch.equal(ident.view(torch.uint8), out.view(torch.uint8)))
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, f in fns.items():
            ts[k].append(timed(torch, s, a.iters, f))
    r = {"part": "stage", "what": f"{n} RGB u8 images of {w}x{h} -> {ow}x{oh} bf16 NCHW, ImageNet mean / std", "iters": a.iters,
         "reps": a.reps, "identity_equals_to_tensor": equal}
    r.update({k + "_ms": spread(v) for k, v in ts.items()})
    return r, equal


def files(a, zj, tz, torch, ctx):
    import torch.nn.functional as F
    import jpeg_enc as je
    synth = importlib.import_module("zune-jpeg_amd.synth")
    n, W, H, ow, oh = a.files, 512, 384, 224, 224
    blobs = [je.encode_baseline(je.small_planes(W, H, 2, 2, 3, seed=k), synth.quant_tables(85), W, H, 2, 2, 3) for k in range(min(n, 8))]
    blobs = [blobs[k % len(blobs)] for k in range(n)]
    ms = [tz.warp_matrix((ow, oh), (W / 2, H / 2), angle=-30 + 60 * k / max(1, n - 1), scale=0.7) for k in range(n)]
    decs, decs2 = [], []
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    # output pixel centre -> source pixel coordinates, as grid_sample's normalised grid (align_corners=False)
    Y, X = torch.meshgrid(torch.arange(oh, device="cuda") + 0.5, torch.arange(ow, device="cuda") + 0.5, indexing="ij")
    m = torch.tensor(ms, device="cuda", dtype=torch.float32)
    gx = (m[:, 0, None, None] * X + m[:, 1, None, None] * Y + m[:, 2, None, None]) * (2.0 / W) - 1
    gy = (m[:, 3, None, None] * X + m[:, 4, None, None] * Y + m[:, 5, None, None]) * (2.0 / H) - 1
    grid = torch.stack([gx, gy], -1)

    def warped():
        return tz.decode_files_warped_to_tensor(ctx, blobs, ms, (ow, oh), mean=MEAN, std=STD, workers=a.workers, decoders=decs)

    def old():
        full = tz.decode_files_resized_to_tensor(ctx, blobs, None, (W, H), dtype=torch.uint8, workers=a.workers, decoders=decs2)
        x = ((full.float() / 255 - mean) / std).to(torch.bfloat16)
        return F.grid_sample(x, grid.to(torch.bfloat16), mode="bilinear", padding_mode="zeros", align_corners=False)

    for _ in range(2):
        o1, o2 = warped(), old()
    torch.cuda.synchronize()
    # (the fill differs: 0 before the normalisation here, 0 after it in grid_sample; compared where the output lies inside)
    t1, t2 = [], []
    for _ in range(a.reps):
        for fn, ts in ((warped, t1), (old, t2)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"part": "files", "what": f"{n} JPEG files of {W}x{H} 4:2:0, each rotated about its centre at scale 0.7 -> {ow}x{oh} bf16 NCHW",
            "reps": a.reps, "workers": a.workers, "decode_files_warped_ms": spread(t1), "full_decode_plus_grid_sample_ms": spread(t2),
            "largest_difference": round(float((o1.float() - o2.float()).abs().max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # (first: one HIP runtime in the process)
    zj = importlib.import_module("zune-jpeg_amd")
    tz = importlib.import_module("zune-jpeg_amd.tensors")
    ctx = zj.Context(zj.BACKEND_HIP, 0)  # raises without a GPU: there is nothing to measure on a CPU
    s = torch.cuda.Stream()
    lines = [f"# tools/warp_bench.py --iters {a.iters} --reps {a.reps} --files {a.files}; device: {torch.cuda.get_device_name(0)}; "
             f"libzjhip.so: {os.path.getsize(zj.lib_path())} bytes"]
    print(lines[0], flush=True)
    r, ok = stage(a, zj, tz, torch, ctx, s)
    lines.append(json.dumps(r))
    print(lines[-1], flush=True)
    lines.append(json.dumps(files(a, zj, tz, torch, ctx)))
    print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
