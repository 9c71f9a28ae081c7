#!/usr/bin/env python3
"""Times of the tone stages (zj_histogram_device, zj_lut_device, zj_tone_device) and of the toned file-batch
call on one GPU.  The figures in profiles/tone.txt come from here; nothing is asserted.
  stage    on 16 images of 4096 x 4096 and on 128 of 224 x 224, HWC, in one process on one stream with HIP events around
           each call, the ways alternated in every round:
             histogram (random)   zj_histogram_device on uniformly random bytes: the counters spread over all bins
             histogram (flat)     ... on images of one value: every lane adds to the same three counters
             lookup               zj_lut_device, apart, random permutation tables
             tone (equalize)      zj_tone_device in place: memset + histogram + table build + lookup
             colour               zj_color_device, apart, jitter matrices (profiles/color.txt's stage)
             torch copy           a device-to-device copy of as many bytes as the lookup reads plus writes
  files    128 Pillow-written files of 200..640 pixels a side -> 224 x 224 bf16 (profiles/mixed_batch.txt's workload),
           decoders prepared once, a host clock around the synchronous finish call, alternated in every round:
             plain    zj_decoder_finish_pixels_resized_crop_batch_device (the toned call's body with no op)
             equalize zj_decoder_finish_pixels_resized_crop_batch_toned_device with an equalize op per file
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SIZE = (224, 224)


def bench_stage(zj, tz, ctx, torch, reps):
    from color_bench import jitter_matrices
    st = torch.cuda.Stream()  # (a stream of its own: the null stream's handle would select the context's stream instead)
    eq = (zj.TONE_EQUALIZE, 0)
    for n, side in ((16, 4096), (128, 224)):
        g = torch.Generator(device="cuda")
        g.manual_seed(side)
        rnd = [torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
        flat = [torch.full((side, side, 3), 90 + i, dtype=torch.uint8, device="cuda") for i in range(n)]
        work = [t.clone() for t in rnd]
        out = [torch.empty_like(t) for t in rnd]
        hist = torch.empty((n, 3, 256), dtype=torch.int32, device="cuda")
        luts = torch.stack([torch.stack([torch.randperm(256, device="cuda", generator=g).to(torch.uint8) for _ in range(3)]) for _ in range(n)])
        ms = jitter_matrices(tz, n)
        moved = 2 * 3 * side * side * n
        c0 = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        c1 = torch.empty_like(c0)
        torch.cuda.synchronize()
        ptr = lambda v: [t.data_ptr() for t in v]
        sizes = [(side, side)] * n
        hwc = zj.LAYOUT_HWC
        calls = {
            "histogram (random)": (lambda: ctx.histogram_device(ptr(rnd), sizes, 3, hwc, hist.data_ptr(), stream=st.cuda_stream), moved // 2),
            "histogram (flat)": (lambda: ctx.histogram_device(ptr(flat), sizes, 3, hwc, hist.data_ptr(), stream=st.cuda_stream), moved // 2),
            "lookup": (lambda: ctx.lut_device(ptr(rnd), sizes, 3, hwc, luts.data_ptr(), ptr(out), stream=st.cuda_stream), moved),
            "tone (equalize)": (lambda: ctx.tone_device(ptr(work), sizes, 3, hwc, [eq] * n, ptr(work), stream=st.cuda_stream), 3 * moved // 2),
            "colour": (lambda: ctx.color_device(ptr(rnd), sizes, hwc, ms, ptr(out), stream=st.cuda_stream), moved),
            "torch copy": (lambda: c1.copy_(c0), moved),
        }
        times = {k: [] for k in calls}
        with torch.cuda.stream(st):
            for call, _ in calls.values():
                for _ in range(3):
                    call()
            st.synchronize()
            for _ in range(reps):
                for name, (call, _) in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    call()
                    e1.record(st)
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
        copy = statistics.median(times["torch copy"])
        for name, (_, nbytes) in calls.items():
            t = times[name]
            med = statistics.median(t)
            rate = nbytes / med / 1e6
            print(f"stage: {n} x {side}x{side} HWC {name:20s} median {med * 1000:9.1f} us  min {min(t) * 1000:9.1f} us  "
                  f"{rate:7.1f} GB/s moved ({nbytes / 1e6:.1f} MB)  {rate / (moved / copy / 1e6):5.2f} of the copy's rate  "
                  f"{med / copy:5.2f} of the copy's time")


def bench_files(zj, tz, ctx, torch, rounds):
    from color_bench import make_files
    blobs, sizes = make_files(128)
    n = len(blobs)
    decs = []
    for b in blobs:
        d = zj.Decoder(None, ctx)
        d.prepare(b)
        decs.append(d)
    wins = [(0, 0, w, h) for w, h in sizes]
    scale, bias = tz.normalize_factors(3, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    out = torch.empty((n, 3, SIZE[1], SIZE[0]), dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    cap = out.numel() * out.element_size()

    def finish(tones):
        rcs = zj.finish_pixels_resized_crop_batch(decs, ctx, wins, SIZE[0], SIZE[1], zj.DTYPE_BF16, zj.TENSOR_NCHW, out.data_ptr(), cap,
                                                  scale, bias, None, False, 2, False, "bilinear", tones=tones)
        assert not any(rcs), rcs

    ways = {"plain": lambda: finish(None), "equalize": lambda: finish([(zj.TONE_EQUALIZE, 0)] * n)}
    for call in ways.values():
        for _ in range(3):
            call()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for name, call in ways.items():
            t0 = time.perf_counter()
            call()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in times.items():
        print(f"files: 128 files -> 224x224 bf16, max_prescale 2, {name:8s} median {statistics.median(v):7.3f} ms  min {min(v):7.3f} ms"
              f"  max {max(v):7.3f} ms  ({rounds} rounds, the ways alternated)")
    print(f"files: equalize / plain = {statistics.median(times['equalize']) / statistics.median(times['plain']):.3f} (medians)")
    for d in decs:
        d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["files", "stage"])
    a = ap.parse_args()
    import torch
    zj = importlib.import_module("zune-jpeg_amd")
    tz = importlib.import_module("zune-jpeg_amd.tensors")
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    if a.only != "files":
        bench_stage(zj, tz, ctx, torch, a.reps)
    if a.only != "stage":
        bench_files(zj, tz, ctx, torch, a.rounds)
    ctx.close()


if __name__ == "__main__":
    main()
