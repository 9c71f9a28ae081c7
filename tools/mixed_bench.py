#!/usr/bin/env python3
"""Mixed-size JPEG batches into one resized-crop tensor: the batch call
(zj_decoder_finish_pixels_resized_crop_batch_device) against a loop of the single-file call
(zj_decoder_finish_pixels_resized_crop_oriented_device) over the SAME prepared decoders, in one process.

128 synthetic files (Pillow; nothing is downloaded): widths and heights drawn from 200..640, 4:2:0 / 4:4:4 / 4:2:2 mixed,
qualities 50..95; one RandomResizedCrop window per file (scale 0.08..1 of the area, aspect 3/4..4/3), resized to 224 x 224
bfloat16 NCHW.  Settings: bilinear, antialiased, bicubic, each with max_prescale 1 and 8.

The entropy stage (prepare: headers + the CPU Huffman walker) is timed on its own; the GPU stage is what differs between
the two paths and is timed with a host clock around calls that end in a device synchronise (both calls synchronise the
context's stream before they return).  Per setting: both paths warmed up, then `--repeats` alternating rounds of
`--inner` calls each, medians and the spread.  The outputs of the two paths are compared for equality first.

  python tools/mixed_bench.py [--files 128] [--repeats 15] [--inner 4] [--out profiles/mixed_batch.txt] [--once]
                              [--gray-share P]

--gray-share P (default 0: the runs above as they are): round(P x files) of the files, picked by a generator of their own, are
saved as single-component JPEGs of their first channel, and every decoder gets ZJ_FLAG_GRAY_TO_RGB: those
files come out as RGB with R = G = B, in the same batch call.

--once: one batch call and one loop per setting, no timing table; with --path batch (or loop) only that one: the run to put
under `rocprofv3 --kernel-trace --stats`, whose per-kernel call counts are the launch counts."""
import argparse
import importlib
import io
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("bilinear", False, "bilinear"), ("antialiased", True, "bilinear"), ("bicubic", True, "bicubic")]


def make_files(n, seed, gray=()):
    from PIL import Image
    rng = np.random.default_rng(seed)
    files = []
    for i in range(n):
        w, h = int(rng.integers(200, 641)), int(rng.integers(200, 641))
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * (1 + i % 5) + yy) % 256, (xx // 3 + yy * (2 + i % 3)) % 256, (xx * yy // (50 + i)) % 256], -1)
        img = (base + rng.normal(0, 12, base.shape)).clip(0, 255).astype(np.uint8)
        buf = io.BytesIO()
        quality = int(rng.integers(50, 96))
        if i in gray:
            Image.fromarray(img[..., 0]).save(buf, "JPEG", quality=quality)
        else:
            Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=["4:2:0", "4:4:4", "4:2:2"][i % 3])
        files.append((buf.getvalue(), w, h))
    return files


def random_resized_crop(rng, w, h):
    """torchvision's RandomResizedCrop.get_params: scale (0.08, 1), ratio (3/4, 4/3), ten tries, then the centre"""
    area = w * h
    for _ in range(10):
        target = area * rng.uniform(0.08, 1.0)
        ratio = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        cw, ch = int(round(np.sqrt(target * ratio))), int(round(np.sqrt(target / ratio)))
        if 0 < cw <= w and 0 < ch <= h:
            return int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch
    s = min(w, h)
    return (w - s) // 2, (h - s) // 2, s, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--path", choices=["both", "batch", "loop"], default="both", help="with --once: which of the two to run")
    ap.add_argument("--gray-share", type=float, default=0.0, help="share of the files that are single-component JPEGs")
    a = ap.parse_args()

    import torch  # (first: one HIP runtime in the process)
    zj = importlib.import_module("zune-jpeg_amd")
    tz = importlib.import_module("zune-jpeg_amd.tensors")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if not 0.0 <= a.gray_share <= 1.0:
        ap.error("--gray-share is a share: 0..1")
    ngray = int(round(a.gray_share * a.files))
    gray = set(int(i) for i in np.random.default_rng(a.seed + 2).choice(a.files, ngray, replace=False)) if ngray else set()
    files = make_files(a.files, a.seed, gray)
    rng = np.random.default_rng(a.seed + 1)
    wins = [random_resized_crop(rng, w, h) for _, w, h in files]
    n = len(files)
    ctx = zj.Context(zj.BACKEND_HIP, 0)  # raises without a GPU: there is nothing to measure on a CPU
    opt = None
    if gray:
        opt = zj.ZuneJpegOptions()
        opt.flags = zj.FLAG_GRAY_TO_RGB
    decs = [zj.Decoder(opt, ctx) for _ in range(n)]
    say(f"# tools/mixed_bench.py: {n} files, {sum(len(f[0]) for f in files) / 1e6:.2f} MB, sizes "
        f"{min(f[1] for f in files)}..{max(f[1] for f in files)} x {min(f[2] for f in files)}..{max(f[2] for f in files)}, "
        f"{sum(f[1] * f[2] for f in files) / 1e6:.1f} MP; windows {sum(w[2] * w[3] for w in wins) / 1e6:.1f} MP -> 224 x 224 bf16 NCHW")
    if gray:
        say(f"# --gray-share {a.gray_share:g}: {ngray} single-component files, decoded to RGB (ZJ_FLAG_GRAY_TO_RGB)")
    say(f"# device: {torch.cuda.get_device_name(0)}")

    # entropy stage: prepare() of every file, on one thread (the walker; the same for both paths)
    t_prep = []
    for _ in range(1 if a.once else 5):
        t0 = time.perf_counter()
        for d, f in zip(decs, files):
            d.prepare(f[0])
        t_prep.append(time.perf_counter() - t0)
    say(f"entropy stage (prepare, CPU walker, 1 thread): median {statistics.median(t_prep) * 1e3:.2f} ms per {n} files "
        f"(min {min(t_prep) * 1e3:.2f}, max {max(t_prep) * 1e3:.2f})")

    size = (224, 224)
    scale, bias = tz.normalize_factors(3, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    out_b = torch.empty((n, 3, 224, 224), dtype=torch.bfloat16, device="cuda")
    out_l = torch.empty_like(out_b)
    img = out_b[0].numel() * 2
    torch.cuda.synchronize()

    def batch(aa, interp, mp):
        rcs = zj.finish_pixels_resized_crop_batch(decs, ctx, wins, 224, 224, zj.DTYPE_BF16, zj.TENSOR_NCHW, out_b.data_ptr(),
                                                  n * img, scale, bias, None, aa, mp, True, interp)
        assert not any(rcs), rcs

    def loop(aa, interp, mp):
        for k, d in enumerate(decs):
            w = wins[k]
            d.finish_pixels_resized_crop_device(w[0], w[1], w[2], w[3], 224, 224, zj.DTYPE_BF16, zj.TENSOR_NCHW,
                                                out_l.data_ptr() + k * img, img, scale, bias, False, aa, mp, True, interp)

    say()
    say(f"GPU stage, {n} files per call; host clock around synchronising calls; {a.repeats} alternating rounds of {a.inner} calls")
    say(f"{'setting':<14}{'prescale':>9}{'batch ms':>10}{'(min..max)':>16}{'loop ms':>10}{'(min..max)':>16}{'loop/batch':>11}{'files/s batch':>15}")
    for name, aa, interp in SETTINGS:
        for mp in (1, 8):
            if a.once and a.path != "both":
                (batch if a.path == "batch" else loop)(aa, interp, mp)
                say(f"{name:<14}{mp:>9}   one {'batch call' if a.path == 'batch' else 'loop of single-file calls'}")
                continue
            batch(aa, interp, mp)
            loop(aa, interp, mp)
            ctx.sync()
            same = torch.equal(out_b.view(torch.uint8), out_l.view(torch.uint8))
            if not same:
                say(f"{name} prescale {mp}: THE TWO PATHS DIFFER")
                return 1
            if a.once:
                say(f"{name:<14}{mp:>9}   one batch call and one loop, outputs equal")
                continue
            for _ in range(2):  # warm-up of both at this setting
                batch(aa, interp, mp)
                loop(aa, interp, mp)
            tb, tl = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    batch(aa, interp, mp)
                t1 = time.perf_counter()
                for _ in range(a.inner):
                    loop(aa, interp, mp)
                t2 = time.perf_counter()
                tb.append((t1 - t0) / a.inner)
                tl.append((t2 - t1) / a.inner)
            mb, ml = statistics.median(tb), statistics.median(tl)
            say(f"{name:<14}{mp:>9}{mb * 1e3:>10.3f}{f'({min(tb) * 1e3:.3f}..{max(tb) * 1e3:.3f})':>16}{ml * 1e3:>10.3f}"
                f"{f'({min(tl) * 1e3:.3f}..{max(tl) * 1e3:.3f})':>16}{ml / mb:>11.2f}{n / mb:>15.0f}")
    for d in decs:
        d.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
