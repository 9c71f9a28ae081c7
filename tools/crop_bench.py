"""Crop-window decode against the full decode, HIP-event timings on 128 resident 4096x4096 4:2:0 frames (synth.make_frame_t
on the GPU, like bench.py), one JSON line:

  --scaled            the reduced whole-frame decode of 16 frames at 1/2, 1/4, 1/8 against 16 full decodes
  whole_rate_ratio    16 whole-frame windows (zj_decode_crops_device) vs 16 full decodes (zj_decode_frames_device): rate
  centre_time_ratio   16 centre 2048x2048 windows vs 16 full decodes: time
  random224_speedup   128 random 224x224 windows vs 128 full decodes
  upload_fraction     the file path (zj_decoder_finish_pixels_crop_device, CPU entropy): plane bytes a 1024-row window
                      uploads / all plane bytes, from the window's strip range (32-row strips)

usage: python tools/crop_bench.py [--iters N]
       python tools/crop_bench.py --file F.jpg [--rows 1024]   the file path alone (CPU entropy): one crop of `rows` rows
                                                               from row 1536; run it under rocprofv3 --memory-copy-trace to
                                                               see the bytes it uploads (profiles/crop_decode.txt)"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--file")
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--scaled", action="store_true", help="only the reduced whole-frame case (profiles/scaled_decode.txt)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.file:
        return file_upload(a)
    import numpy as np
    import torch
    zj = importlib.import_module("zune-jpeg_amd")
    synth = importlib.import_module("zune-jpeg_amd.synth")
    W = H = 4096
    N = 128
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    frames, qts = [], None
    for i in range(N):
        planes, qts = synth.make_frame_t(W, H, 2, 2, 3, seed=1234, frame_index=i, device="cuda")
        frames.append(planes)
    d = zj.FrameDesc.make(W, H, 2, 2, 3, zj.ColorSpace.RGB, qts)
    out_len = zj.lib().zj_out_len(__import__("ctypes").byref(d))
    full = [torch.empty(out_len, dtype=torch.uint8, device="cuda") for _ in range(N)]
    crop_buf = torch.empty(N * out_len // 16 + 16 * out_len, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()  # (a stream of its own: a null handle would mean the library's stream, not torch's)
    ptrs = lambda k, n: [f[k].data_ptr() for f in frames[:n]]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(a.iters):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    def full_n(n):
        return lambda: ctx.decode_frames_device(d, ptrs(0, n), ptrs(1, n), ptrs(2, n), [o.data_ptr() for o in full[:n]], s.cuda_stream)

    def crops(n, origins, w, h):
        ln = zj.crop_out_len(d, w, h)
        base = crop_buf.data_ptr()
        outs = [base + i * ln for i in range(n)]
        return lambda: ctx.decode_crops_device(d, ptrs(0, n), ptrs(1, n), ptrs(2, n), origins, w, h, outs, 0, s.cuda_stream)

    if a.scaled:
        # Reduced whole-frame decode (zj_decode_crops_scaled_device, windows NULL) of 16 resident frames at each scale
        # against zj_decode_frames_device of the same frames, alternating; bytes = the planes read (every block is one
        # 128-byte line whatever the scale: the floor) + the pixels written, as a fraction of 8 TB/s
        plane_bytes = 16 * W * H * 3                       # 4:2:0: 1.5 coefficients of 2 bytes per pixel
        res = {"frames": f"16 of {N} x {W}x{H} 4:2:0 RGB, resident", "iters": a.iters, "reps": a.reps,
               "plane_bytes": plane_bytes, "floor_ms_at_8TBs": round(plane_bytes / 8e12 * 1e3, 4)}
        sp = lambda ts: {"min": round(min(ts), 4), "median": round(sorted(ts)[len(ts) // 2], 4), "max": round(max(ts), 4)}
        for scale in (2, 4, 8):
            rw, rh = zj.scaled_size(d, scale)
            ln = zj.scaled_crop_out_len(d, scale, rw, rh)
            outs = [crop_buf.data_ptr() + i * ln for i in range(16)]
            run = lambda: ctx.decode_crops_scaled_device(d, ptrs(0, 16), ptrs(1, 16), ptrs(2, 16), scale, outs, None, 0, s.cuda_stream)
            t_s, t_f = [], []
            for _ in range(a.reps):
                t_f.append(timed(full_n(16)))
                t_s.append(timed(run))
            ms, mf = sp(t_s)["median"], sp(t_f)["median"]
            res[f"1/{scale}"] = {"scaled16_ms": sp(t_s), "full16_ms": sp(t_f), "time_ratio_full_over_scaled": round(mf / ms, 2),
                                 "bytes": plane_bytes + 16 * ln,
                                 "fraction_of_8TBs": round((plane_bytes + 16 * ln) / (ms * 1e-3) / 8e12, 3),
                                 "full_fraction_of_8TBs": round((plane_bytes + 16 * out_len) / (mf * 1e-3) / 8e12, 3),
                                 "times_the_plane_floor": round(ms / (plane_bytes / 8e12 * 1e3), 2)}
        print(json.dumps(res))
        ctx.close()
        return
    t_full16 = timed(full_n(16))
    t_full128 = timed(full_n(N))
    t_whole16 = timed(crops(16, [(0, 0)] * 16, W, H))
    t_centre16 = timed(crops(16, [(1024, 1024)] * 16, 2048, 2048))
    rng = np.random.default_rng(7)
    org = [(int(rng.integers(W - 224 + 1)), int(rng.integers(H - 224 + 1))) for _ in range(N)]
    t_rand128 = timed(crops(N, org, 224, 224))
    # the file path's upload: strips [y / 32, ceil((y + 1024) / 32)) of 128 (a window starting on a strip boundary)
    y0 = 1536
    s0, s1 = y0 // 32, -(-(y0 + 1024) // 32)
    res = {
        "frames": f"{N} x {W}x{H} 4:2:0 RGB, resident", "iters": a.iters,
        "full16_ms": round(t_full16, 4), "full128_ms": round(t_full128, 4),
        "whole16_ms": round(t_whole16, 4), "whole_rate_ratio": round(t_full16 / t_whole16, 3),
        "centre2048_16_ms": round(t_centre16, 4), "centre_time_ratio": round(t_centre16 / t_full16, 3),
        "random224_128_ms": round(t_rand128, 4), "random224_speedup": round(t_full128 / t_rand128, 2),
        "upload_fraction": round((s1 - s0) / 128, 4),
    }
    print(json.dumps(res))
    ctx.close()


def file_upload(a):
    """one window of a file through zj_decoder_finish_pixels_crop_device with the CPU walker's planes; prints the plane
    bytes of the whole file and of the window's strips (what the call should upload), nothing else copies to the device"""
    import ctypes as C
    zj = importlib.import_module("zune-jpeg_amd")
    data = open(a.file, "rb").read()
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    dec = zj.Decoder(zj.ZuneJpegOptions(), ctx)
    desc, _ = dec.prepare(data)
    W, H = desc.width, desc.height
    y0, h = 1536, min(a.rows, H - 1536)
    ln = zj.crop_out_len(desc, W, h)
    d_out = ctx.device_alloc(ln)
    dec.finish_pixels_crop_device(0, y0, W, h, d_out, ln)
    ctx.device_free(d_out)
    planes = sum(zj.lib().zj_plane_len(C.byref(desc), c) for c in range(desc.in_components)) * 2
    sh = 8 * desc.v_max * (2 if desc.h_max == 2 else 1)  # luma rows per strip (zj_plan.h)
    n_strips = (-(-H // (8 * desc.v_max))) // (2 if desc.h_max == 2 else 1)
    s0, s1 = y0 // sh, min(-(-(y0 + h) // sh), n_strips)
    print(json.dumps({"file": os.path.basename(a.file), "width": W, "height": H, "window_rows": [y0, y0 + h],
                      "strips": [s0, s1], "n_strips": n_strips, "plane_bytes": planes,
                      "window_strip_bytes": planes * (s1 - s0) // n_strips, "expected_fraction": round((s1 - s0) / n_strips, 4)}))
    dec.close()
    ctx.close()


if __name__ == "__main__":
    main()
