#!/usr/bin/env python3
"""Time of the planes-to-RGB stage (zj_planes_to_rgb_device) beside the gray-to-RGB stage (zj_gray_to_rgb_device) for the same
outputs on the same GPU: 128 images of 500 x 375 -- 4:1:1 planes (chroma at ratio 4 across), 4:1:0-like planes (ratio 4
across, 2 down), every plane at ratio 4 both ways, every plane at ratio 1 -- both layouts, both colour modes, HIP events on
one stream, warm, the median of 20 calls.  The figures in profiles/any_sampling.txt come from here; nothing is asserted."""
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
    n, reps, w, h = 128, 20, 500, 375
    g = torch.Generator(device="cuda")
    g.manual_seed(w)
    shapes = {"4:1:1": ((1, 1), (4, 1), (4, 1)), "4:1:0": ((1, 1), (4, 2), (4, 2)), "4x4 all": ((4, 4), (4, 4), (4, 4)),
              "1x1 all": ((1, 1), (1, 1), (1, 1))}
    gray = [torch.randint(0, 256, (h, w), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    out = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]
    sizes = [(w, h)] * n
    ptr = lambda v: [t.data_ptr() for t in v]
    for name, rs in shapes.items():
        planes = [[torch.randint(0, 256, (-(-h // ry), -(-w // rx)), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
                  for rx, ry in rs]
        torch.cuda.synchronize()  # (the inputs were made on torch's current stream)
        read = sum(-(-h // ry) * -(-w // rx) for rx, ry in rs)
        for chw in (False, True):
            lay = zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC
            calls = {
                f"planes {name}": (lambda: ctx.planes_to_rgb_device(ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), sizes, [rs] * n, lay,
                                                                     ptr(out), False, stream=st.cuda_stream), read + 3 * w * h),
                f"planes {name} stored RGB": (lambda: ctx.planes_to_rgb_device(ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), sizes,
                                                                                [rs] * n, lay, ptr(out), True, stream=st.cuda_stream),
                                              read + 3 * w * h),
                "gray_to_rgb": (lambda: ctx.gray_to_rgb_device(ptr(gray), sizes, lay, ptr(out), stream=st.cuda_stream), 4 * w * h),
            }
            for label, (call, moved) in calls.items():
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
                print(f"{n} x {w}x{h} {'CHW' if chw else 'HWC'} {label:28s} median {med * 1000:8.1f} us  min {min(ms) * 1000:8.1f} us"
                      f"  {n * moved / med / 1e6:7.1f} GB/s")
    ctx.close()


if __name__ == "__main__":
    main()
