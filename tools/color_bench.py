#!/usr/bin/env python3
"""Times of the colour-matrix stage (zj_color_device) and of the coloured file-batch call on one GPU.  The
figures in profiles/color.txt come from here; nothing is asserted.
  files    128 Pillow-written files of 200..640 pixels a side -> 224 x 224 bf16, decoders prepared once, the finish call timed
           by a host clock around it (it ends synchronised), the three ways alternated in every round:
             plain    zj_decoder_finish_pixels_resized_crop_batch_device
             colour   ..._batch_colored_device with random jitter matrices
             einsum   plain, then a per-image torch.einsum over the tensor (what a caller did before), synchronised
  stage    the stage alone on 128 images of 256 x 256 and 16 of 4096 x 4096, HWC and CHW, apart and in place, HIP events on
           one stream, beside torch's device-to-device copy of as many bytes as the stage reads plus writes
  paths    the share of the files' 16-pixel runs that take the 16-byte loads and stores, from the shapes (no GPU needed)
  launches one coloured plane call with all-identity matrices, or the uncoloured call (--launches identity / plain): to be run
           under a kernel trace, which counts the launches; no timing
"""
import argparse
import importlib
import io
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZE = (224, 224)


def make_files(n, seed=7):
    from PIL import Image
    rng = np.random.default_rng(seed)
    blobs, sizes = [], []
    for k in range(n):
        w, h = (int(v) for v in rng.integers(200, 641, 2))
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 3 + yy * 2 + k * 17) % 256, (xx * yy // 7 + 40 * k) % 256, (255 - xx - 2 * yy) % 256], -1)
        img = (img + rng.integers(0, 24, img.shape)).clip(0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=85, subsampling="4:2:0")
        blobs.append(buf.getvalue())
        sizes.append((w, h))
    return blobs, sizes


def jitter_matrices(tz, n, seed=11):
    """ColorJitter(0.4, 0.4, 0.4, 0.1)'s ranges, one draw per image"""
    rng = np.random.default_rng(seed)
    return [tz.color_matrix(*(float(v) for v in rng.uniform(0.6, 1.4, 3)), hue=float(rng.uniform(-0.1, 0.1))) for _ in range(n)]


def sixteen_byte_share(sizes):
    """the share of 16-pixel runs of tight HWC images at 16-byte-aligned addresses that are whole and start on a 16-byte
    boundary (cmyk_get / expand_put's first branch): a run of row r starts at byte 3 w r + 48 i"""
    fast = total = 0
    for w, h in sizes:
        runs = (w + 15) // 16
        for r in range(h):
            total += runs
            if (3 * w * r) % 16 == 0:
                fast += w // 16
    return fast / total


def bench_files(zj, tz, ctx, torch, rounds):
    blobs, sizes = make_files(128)
    n = len(blobs)
    decs = []
    for b in blobs:
        d = zj.Decoder(None, ctx)
        d.prepare(b)
        decs.append(d)
    wins = [(0, 0, w, h) for w, h in sizes]
    ms = jitter_matrices(tz, n)
    scale, bias = tz.normalize_factors(3, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    out = torch.empty((n, 3, SIZE[1], SIZE[0]), dtype=torch.bfloat16, device="cuda")
    lin = torch.tensor(np.stack([m[:, :3] for m in ms]), dtype=torch.float32, device="cuda")
    # (on the normalised values the caller has to rewrite each matrix: y' = s (M ((y - b) / s) + t) + b)
    s_t, b_t = torch.tensor(scale, device="cuda"), torch.tensor(bias, device="cuda")
    off = torch.tensor(np.stack([m[:, 3] for m in ms]), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    cap = out.numel() * out.element_size()

    def finish(colors):
        rcs = zj.finish_pixels_resized_crop_batch(decs, ctx, wins, SIZE[0], SIZE[1], zj.DTYPE_BF16, zj.TENSOR_NCHW, out.data_ptr(), cap,
                                                  scale, bias, None, False, 2, False, "bilinear", colors=colors)
        assert not any(rcs), rcs

    def einsum():
        finish(None)
        grey = (out.float() - b_t[None, :, None, None]) / s_t[None, :, None, None]
        y = torch.einsum("nck,nkhw->nchw", lin, grey) + off[:, :, None, None]
        res = (y * s_t[None, :, None, None] + b_t[None, :, None, None]).to(torch.bfloat16)
        torch.cuda.synchronize()
        return res

    ways = {"plain": lambda: finish(None), "colour": lambda: finish(ms), "einsum": einsum}
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
        print(f"files: 128 files -> 224x224 bf16, max_prescale 2, {name:7s} median {statistics.median(v):7.3f} ms  min {min(v):7.3f} ms"
              f"  max {max(v):7.3f} ms  ({rounds} rounds, the ways alternated)")
    u8_sizes = []
    for w, h in sizes:  # the u8 image each file's matrix acts on: the window at the scale the call picks
        k = 1 if (w >> 1) >= SIZE[0] and (h >> 1) >= SIZE[1] else 0
        u8_sizes.append(((w + (1 << k) - 1) >> k, (h + (1 << k) - 1) >> k))
    print(f"paths: {sixteen_byte_share(u8_sizes):.3f} of the 16-pixel runs of these files' u8 images are whole and 16-byte aligned "
          f"(computed from the shapes, tight rows at aligned addresses)")
    for d in decs:
        d.close()


def bench_stage(zj, ctx, torch, reps):
    st = torch.cuda.Stream()  # (a stream of its own: the null stream's handle would select the context's stream instead)
    tz = importlib.import_module("zune-jpeg_amd.tensors")
    for n, side in ((128, 256), (16, 4096)):
        g = torch.Generator(device="cuda")
        g.manual_seed(side)
        ms = jitter_matrices(tz, n)
        moved = 2 * 3 * side * side * n
        flat = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        flat2 = torch.empty_like(flat)
        for chw in (False, True):
            a = [torch.randint(0, 256, (3, side, side) if chw else (side, side, 3), dtype=torch.uint8, device="cuda", generator=g)
                 for _ in range(n)]
            out = [torch.empty_like(t) for t in a]
            torch.cuda.synchronize()
            ptr = lambda v: [t.data_ptr() for t in v]
            lay = zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC
            sizes = [(side, side)] * n
            calls = {"colour apart": lambda: ctx.color_device(ptr(a), sizes, lay, ms, ptr(out), stream=st.cuda_stream),
                     "colour in place": lambda: ctx.color_device(ptr(a), sizes, lay, ms, ptr(a), stream=st.cuda_stream),
                     "torch copy": lambda: flat2.copy_(flat)}
            for name, call in calls.items():
                with torch.cuda.stream(st):
                    for _ in range(5):
                        call()
                    st.synchronize()
                    t = []
                    for _ in range(reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        call()
                        e1.record(st)
                        e1.synchronize()
                        t.append(e0.elapsed_time(e1))
                med = statistics.median(t)
                print(f"stage: {n} x {side}x{side} {'CHW' if chw else 'HWC'} {name:16s} median {med * 1000:9.1f} us  min {min(t) * 1000:9.1f} us"
                      f"  {moved / med / 1e6:7.1f} GB/s read + written")


def one_plane_call(zj, tz, ctx, torch, which):
    synth = importlib.import_module("zune-jpeg_amd.synth")
    frames = []
    for i, (w, h) in enumerate([(96, 80), (517, 40), (300, 200)]):
        planes, qts = synth.make_frame(w, h, 2, 2, 3, seed=i)
        frames.append((zj.FrameDesc.make(w, h, 2, 2, 3, zj.ColorSpace.RGB, qts), [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes], w, h))
    out = torch.empty((len(frames), 3, 32, 32), dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_crops_resized_mixed_device([f[0] for f in frames], [f[1][0].data_ptr() for f in frames], [f[1][1].data_ptr() for f in frames],
                                          [f[1][2].data_ptr() for f in frames], [(0, 0, f[2], f[3]) for f in frames], 32, 32, zj.DTYPE_BF16,
                                          zj.TENSOR_NCHW, out.data_ptr(), colors=[None] * len(frames) if which == "identity" else None)
    ctx.sync()
    print(f"launches: one plane call over {len(frames)} frames, {which}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--launches", choices=["identity", "plain"])
    ap.add_argument("--only", choices=["files", "stage"])
    ap.add_argument("--paths-only", action="store_true")
    a = ap.parse_args()
    if a.paths_only:
        _, sizes = make_files(128)
        print(f"paths: {sixteen_byte_share(sizes):.3f} at full size")
        return
    import torch
    zj = importlib.import_module("zune-jpeg_amd")
    tz = importlib.import_module("zune-jpeg_amd.tensors")
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    if a.launches:
        one_plane_call(zj, tz, ctx, torch, a.launches)
    else:
        if a.only != "stage":
            bench_files(zj, tz, ctx, torch, a.rounds)
        if a.only != "files":
            bench_stage(zj, ctx, torch, a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
