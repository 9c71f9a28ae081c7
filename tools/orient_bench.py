"""EXIF orientation, HIP-event timings on one GPU, one JSON line per measurement (profiles/orient.txt):

  (a) zj_orient_device on 128 u8 RGB HWC crops of about 1000x800 (their sizes vary by +-10 %), orientations 1, 3 and 6,
      against a device-to-device copy of the same bytes (one torch copy_ of the crops' common storage) in the same
      process, alternating; bytes read + written over the time as a share of 8 TB/s.
  (b) tensors.decode_resized_crops_to_tensor over 128 resident 4096x4096 4:2:0 frames with RandomResizedCrop windows ->
      224x224 bf16 NCHW (the workload of tools/resize_bench.py part b), bilinear and antialiased, with orientations = None
      (the call as it was), all 1, all 3, all 6 -- alternating in one process.

Each time is the mean over --iters calls between one event pair; --reps such measurements give the spread (min / median /
max).

usage: python tools/orient_bench.py [--part a|b|all] [--iters N] [--reps R] [--frames N]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from resize_bench import H, MEAN, OUT, STD, W, rrc_windows, spread, timer  # noqa: E402


def part_a(a, zj, torch, ctx, s):
    import numpy as np
    rng = np.random.default_rng(21)
    n = 128
    sizes = [(int(rng.integers(900, 1101)), int(rng.integers(720, 881))) for _ in range(n)]
    offs, at = [], 0
    for w, h in sizes:
        offs.append(at)
        at += (w * h * 3 + 255) // 256 * 256
    src = torch.randint(0, 256, (at,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    nbytes = sum(w * h * 3 for w, h in sizes)
    ins, outs = [src.data_ptr() + o for o in offs], [dst.data_ptr() + o for o in offs]
    timed = timer(torch, s, a.iters)

    def copy():
        with torch.cuda.stream(s):
            dst.copy_(src)

    res = []
    for o in (1, 3, 6):
        fn = lambda: ctx.orient_device(ins, sizes, 3, zj.LAYOUT_HWC, [o] * n, outs, None, None, s.cuda_stream)
        t_o, t_c = [], []
        for _ in range(a.reps):
            t_o.append(timed(fn))
            t_c.append(timed(copy))
        mo, mc = spread(t_o)["median"], spread(t_c)["median"]
        res.append({"part": "a", "orientation": o, "what": f"zj_orient_device, {n} u8 RGB HWC crops of about 1000x800",
                    "iters": a.iters, "reps": a.reps, "bytes": nbytes, "orient_ms": spread(t_o), "d2d_copy_ms": spread(t_c),
                    "orient_over_copy_median": round(mo / mc, 2),
                    "read_plus_written_share_of_8TBps": round(2 * nbytes / (mo * 1e-3) / 8e12, 4)})
    return res


def part_b(a, zj, torch, ctx, s):
    import numpy as np
    synth = importlib.import_module("zune-jpeg_amd.synth")
    tensors = importlib.import_module("zune-jpeg_amd.tensors")
    frames, qts = [], None
    for i in range(a.frames):
        planes, qts = synth.make_frame_t(W, H, 2, 2, 3, seed=1234, frame_index=i, device="cuda")
        frames.append(planes)
    d = zj.FrameDesc.make(W, H, 2, 2, 3, zj.ColorSpace.RGB, qts)
    wins = rrc_windows(np.random.default_rng(12), a.frames)  # (a square frame: the same windows suit every orientation)
    torch.cuda.synchronize()
    timed = timer(torch, s, a.iters)
    res = []
    for aa in (False, True):
        def run(oris):
            with torch.cuda.stream(s):
                return tensors.decode_resized_crops_to_tensor(ctx, d, frames, wins, (OUT, OUT), dtype=torch.bfloat16, mean=MEAN,
                                                              std=STD, stream=s, antialias=aa, orientations=oris)
        cases = {"none": None, "1": [1] * a.frames, "3": [3] * a.frames, "6": [6] * a.frames}
        ts = {k: [] for k in cases}
        for _ in range(a.reps):
            for k, oris in cases.items():
                ts[k].append(timed(lambda: run(oris)))
        same = bool(torch.equal(run(None), run(cases["1"])))
        torch.cuda.synchronize()
        res.append({"part": "b", "antialias": aa,
                    "what": f"decode_resized_crops_to_tensor, {a.frames} resident {W}x{H} 4:2:0 frames, RandomResizedCrop windows "
                            f"-> {OUT}x{OUT} bf16 NCHW normalised", "iters": a.iters, "reps": a.reps,
                    "ms": {k: spread(v) for k, v in ts.items()}, "orientation_1_equals_none": same})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["a", "b", "all"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128)
    a = ap.parse_args()
    import torch
    zj = importlib.import_module("zune-jpeg_amd")
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    s = torch.cuda.Stream()
    for part in (part_a, part_b):
        if a.part in (part.__name__[-1], "all"):
            for r in part(a, zj, torch, ctx, s):
                print(json.dumps(r), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
