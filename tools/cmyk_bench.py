#!/usr/bin/env python3
"""Time of the CMYK-to-RGB stage (zj_cmyk_to_rgb_device) beside the gray-to-RGB stage (zj_gray_to_rgb_device) for the same
images on the same GPU: 128 images of 224 x 224 and of 1024 x 1024, both layouts, HIP events on one stream, warm, the median
of 20 calls.  The figures in profiles/cmyk_rgb.txt come from here; nothing is asserted."""
import importlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    zj = importlib.import_module("zune-jpeg_amd")
    ctx = zj.Context(zj.BACKEND_HIP, 0)
    st = torch.cuda.Stream()  # (a stream of its own: the null stream's handle would select the context's stream instead)
    assert st.cuda_stream != 0
    n, reps = 128, 20
    for side in (224, 1024):
        g = torch.Generator(device="cuda")
        g.manual_seed(side)
        a = [torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
        k = [torch.randint(0, 256, (side, side), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
        out = [torch.empty_like(t) for t in a]
        sizes = [(side, side)] * n
        torch.cuda.synchronize()  # (the inputs were made on torch's current stream)
        ptr = lambda v: [t.data_ptr() for t in v]
        for chw in (False, True):
            lay = zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC
            calls = {
                "cmyk_to_rgb": lambda: ctx.cmyk_to_rgb_device(ptr(a), ptr(k), sizes, lay, ptr(out), [1] * n, stream=st.cuda_stream),
                "cmyk_to_rgb in place": lambda: ctx.cmyk_to_rgb_device(ptr(a), ptr(k), sizes, lay, ptr(a), [0] * n, stream=st.cuda_stream),
                "gray_to_rgb": lambda: ctx.gray_to_rgb_device(ptr(k), sizes, lay, ptr(out), stream=st.cuda_stream),
            }
            for name, call in calls.items():
                for _ in range(3):
                    call()
                st.synchronize()
                ms = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    call()
                    e1.record(st)
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                med = statistics.median(ms)
                moved = n * side * side * (7 if name.startswith("cmyk") else 4)
                print(f"{n} x {side}x{side} {'CHW' if chw else 'HWC'} {name:22s} median {med * 1000:8.1f} us  min {min(ms) * 1000:8.1f} us"
                      f"  {moved / med / 1e6:7.1f} GB/s")
    ctx.close()


if __name__ == "__main__":
    main()
