"""Resized crop decode, HIP-event timings on one GPU, one JSON line per part (profiles/resize_crop.txt):

  (a) the resize kernel alone: 128 u8 HWC crops of RandomResizedCrop sizes (scale 0.08-1, ratio 3/4-4/3) of a 4096x4096
      frame -> 224x224 bfloat16 NCHW (zj_resize_device); bytes written, and written + the input bytes the taps touch, over
      the time as a share of 8 TB/s.  Run this part under `rocprofv3 --kernel-trace --stats` for the kernel's own time.
  (b) tensors.decode_resized_crops_to_tensor over 128 resident 4096x4096 4:2:0 frames (synth.make_frame_t on the GPU, like
      bench.py) with such windows, against the best torch path to the same tensor: the crop entry point per distinct window
      size (tensors.decode_crops_to_tensor) + F.interpolate(bilinear, align_corners=False, antialias=False) + normalise +
      .to(bfloat16), in the same run, on the same stream.

Each time is the mean over --iters calls between one event pair; --reps such measurements give the spread (min / median /
max).  --antialias runs both parts with the triangle filter (ZJ_RESIZE_BILINEAR_AA, profiles/resize_aa.txt): the torch path
then uses F.interpolate(antialias=True), and part (a) counts every byte of the crops as read (each output reads all the
source pixels under it).

--max-prescale 2|4|8 (profiles/scaled_decode.txt) times part (b)'s call with a reduced-size decode under the resize
 against max_prescale=1 in the same process, alternating, for the bilinear and the antialiased filter (or,
with --antialias, that one alone), and gives the largest difference between the two outputs.

--filter bicubic runs the same parts with the bicubic antialiased filter (ZJ_RESIZE_BICUBIC_AA, profiles/resize_bicubic.txt).

usage: python tools/resize_bench.py [--part a|b|all] [--iters N] [--reps R] [--antialias] [--filter bilinear|bicubic]
                                    [--max-prescale S]"""
import argparse
import importlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W = H = 4096
N = 128
OUT = 224
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def rrc_windows(rng, n):
    """torchvision's RandomResizedCrop.get_params (scale 0.08-1, ratio 3/4-4/3, 10 tries then the whole frame)"""
    out = []
    for _ in range(n):
        for _ in range(10):
            area = W * H * rng.uniform(0.08, 1.0)
            r = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
            w, h = int(round(math.sqrt(area * r))), int(round(math.sqrt(area / r)))
            if 0 < w <= W and 0 < h <= H:
                out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
                break
        else:
            out.append((0, 0, W, H))
    return out


def spread(ts):
    ts = sorted(ts)
    return {"min": round(ts[0], 4), "median": round(ts[len(ts) // 2], 4), "max": round(ts[-1], 4)}


def timer(torch, s, iters):
    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(iters):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    return timed


def part_a(a, zj, torch, ctx, s):
    import numpy as np
    import resize_model as rm
    rng = np.random.default_rng(11)
    wins = rrc_windows(rng, N)
    crops = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda") for (_, _, w, h) in wins]
    out = torch.empty((N, 3, OUT, OUT), dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    scale, bias = tensors.normalize_factors(3, MEAN, STD)
    ptrs, sizes = [c.data_ptr() for c in crops], [(w, h) for (_, _, w, h) in wins]
    fn = lambda: ctx.resize_device(ptrs, sizes, 3, zj.LAYOUT_HWC, OUT, OUT, zj.DTYPE_BF16, zj.TENSOR_NCHW, out.data_ptr(),
                                   scale, bias, None, None, s.cuda_stream, antialias=a.antialias, interpolation=a.filter)
    timed = timer(torch, s, a.iters)
    ts = [timed(fn) for _ in range(a.reps)]
    written = out.numel() * 2
    read = 0  # the input bytes the taps touch: rows x columns x 3 of each crop (antialiased: all of it)
    for (_, _, w, h) in wins:
        if a.antialias:
            read += w * h * 3
            continue
        x0, _, x1 = rm.taps(w, OUT)
        y0, _, y1 = rm.taps(h, OUT)
        read += len(set(x0) | set(x1)) * len(set(y0) | set(y1)) * 3
    med = spread(ts)["median"]
    fname = "zj_resize_filtered_device (ZJ_RESIZE_BILINEAR_AA)" if a.antialias else "zj_resize_device"
    if a.filter == "bicubic":
        fname = "zj_resize_filtered_device (ZJ_RESIZE_BICUBIC_AA)"
    return {"part": "a", "what": f"{fname} {N} RandomResizedCrop u8 HWC crops of {W}x{H} -> {OUT}x{OUT} bf16 NCHW",
            "iters": a.iters, "reps": a.reps, "ms": spread(ts), "crop_bytes": sum(w * h * 3 for (_, _, w, h) in wins),
            "bytes_written": written, "bytes_read_touched": read,
            "written_share_of_8TBps": round(written / (med * 1e-3) / 8e12, 4),
            "written_plus_read_share_of_8TBps": round((written + read) / (med * 1e-3) / 8e12, 4)}


def part_b(a, zj, torch, ctx, s):
    import numpy as np
    import torch.nn.functional as F
    synth = importlib.import_module("zune-jpeg_amd.synth")
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    frames, qts = [], None
    for i in range(N):
        planes, qts = synth.make_frame_t(W, H, 2, 2, 3, seed=1234, frame_index=i, device="cuda")
        frames.append(planes)
    d = zj.FrameDesc.make(W, H, 2, 2, 3, zj.ColorSpace.RGB, qts)
    rng = np.random.default_rng(12)
    wins = rrc_windows(rng, N)
    torch.cuda.synchronize()

    def ours():
        with torch.cuda.stream(s):
            return tensors.decode_resized_crops_to_tensor(ctx, d, frames, wins, (OUT, OUT), dtype=torch.bfloat16, mean=MEAN,
                                                          std=STD, stream=s, antialias=a.antialias, interpolation=a.filter)

    groups = {}
    for i, (x, y, w, h) in enumerate(wins):
        groups.setdefault((w, h), []).append(i)
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)

    def torch_path():
        with torch.cuda.stream(s):
            out = torch.empty((N, 3, OUT, OUT), dtype=torch.bfloat16, device="cuda")
            for (w, h), idx in groups.items():
                crops = tensors.decode_crops_to_tensor(ctx, d, [frames[i] for i in idx], [wins[i][:2] for i in idx], (w, h),
                                                       stream=s)
                x = crops.permute(0, 3, 1, 2).float()
                y = F.interpolate(x, size=(OUT, OUT), mode=a.filter, align_corners=False, antialias=a.antialias)
                y = (y / 255 - mean) / std
                out[idx] = y.to(torch.bfloat16)
            return out

    timed = timer(torch, s, a.iters)
    t_ours, t_torch = [], []
    for _ in range(a.reps):
        t_ours.append(timed(ours))
        t_torch.append(timed(torch_path))
    o, t = ours(), torch_path()
    torch.cuda.synchronize()
    diff = (o.float() - t.float()).abs().max().item()
    mo, mt = spread(t_ours)["median"], spread(t_torch)["median"]
    return {"part": "b", "antialias": a.antialias, "filter": a.filter, "what": f"decode_resized_crops_to_tensor, {N} resident {W}x{H} 4:2:0 frames, RandomResizedCrop "
            f"windows -> {OUT}x{OUT} bf16 NCHW normalised", "iters": a.iters, "reps": a.reps, "distinct_sizes": len(groups),
            "ours_ms": spread(t_ours), "torch_path_ms": spread(t_torch), "speedup_median": round(mt / mo, 2),
            "max_abs_diff_vs_torch": round(diff, 4)}


def part_prescale(a, zj, torch, ctx, s):
    import numpy as np
    synth = importlib.import_module("zune-jpeg_amd.synth")
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    frames, qts = [], None
    for i in range(N):
        planes, qts = synth.make_frame_t(W, H, 2, 2, 3, seed=1234, frame_index=i, device="cuda")
        frames.append(planes)
    d = zj.FrameDesc.make(W, H, 2, 2, 3, zj.ColorSpace.RGB, qts)
    wins = rrc_windows(np.random.default_rng(12), N)
    if a.windows == "half":  # the windows that decode at 1/2: 448..895 source pixels per side for a 224 output
        rng = np.random.default_rng(13)
        wins = []
        for _ in range(N):
            w, h = int(rng.integers(2 * OUT, 4 * OUT)), int(rng.integers(2 * OUT, 4 * OUT))
            wins.append((int(rng.integers(W - w + 1)), int(rng.integers(H - h + 1)), w, h))
    torch.cuda.synchronize()
    scales = {}
    for (x, y, w, h) in wins:
        k = 1
        while 2 * k <= a.max_prescale and w // (2 * k) >= OUT and h // (2 * k) >= OUT:
            k *= 2
        scales[k] = scales.get(k, 0) + 1
    timed = timer(torch, s, a.iters)
    res = []
    for aa in ((True,) if a.antialias else (False, True)):
        def run(mp):
            with torch.cuda.stream(s):
                return tensors.decode_resized_crops_to_tensor(ctx, d, frames, wins, (OUT, OUT), dtype=torch.bfloat16, mean=MEAN,
                                                              std=STD, stream=s, antialias=aa, max_prescale=mp,
                                                              interpolation=a.filter)
        t_plain, t_pre = [], []
        for _ in range(a.reps):
            t_plain.append(timed(lambda: run(1)))
            t_pre.append(timed(lambda: run(a.max_prescale)))
        o, q = run(1), run(a.max_prescale)
        torch.cuda.synchronize()
        mp_, mq = spread(t_plain)["median"], spread(t_pre)["median"]
        res.append({"part": "prescale", "windows": a.windows, "antialias": aa, "filter": a.filter, "max_prescale": a.max_prescale,
                    "what": f"decode_resized_crops_to_tensor, {N} resident {W}x{H} 4:2:0 frames, RandomResizedCrop windows -> "
                            f"{OUT}x{OUT} bf16 NCHW normalised", "iters": a.iters, "reps": a.reps,
                    "images_per_scale": {str(k): v for k, v in sorted(scales.items())},
                    "max_prescale_1_ms": spread(t_plain), "prescaled_ms": spread(t_pre), "ratio_median": round(mp_ / mq, 2),
                    "max_abs_diff_between_them": round((o.float() - q.float()).abs().max().item(), 4)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["a", "b", "all"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--antialias", action="store_true")
    ap.add_argument("--filter", default="bilinear", choices=["bilinear", "bicubic"],
                    help="bicubic: ZJ_RESIZE_BICUBIC_AA (DESIGN.md 3.9, profiles/resize_bicubic.txt); implies --antialias")
    ap.add_argument("--max-prescale", type=int, default=1, choices=[1, 2, 4, 8])
    ap.add_argument("--windows", default="rrc", choices=["rrc", "half"],
                    help="with --max-prescale: RandomResizedCrop windows, or windows of 448..895 pixels (all decode at 1/2)")
    a = ap.parse_args()
    if a.filter == "bicubic":
        a.antialias = True
    import torch
    zj = importlib.import_module("zune-jpeg_amd")
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    s = torch.cuda.Stream()  # (a stream of its own: a null handle would mean the library's stream, not torch's)
    if a.max_prescale > 1:
        for r in part_prescale(a, zj, torch, ctx, s):
            print(json.dumps(r), flush=True)
        ctx.close()
        return
    if a.part in ("a", "all"):
        print(json.dumps(part_a(a, zj, torch, ctx, s)), flush=True)
    if a.part in ("b", "all"):
        print(json.dumps(part_b(a, zj, torch, ctx, s)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
