"""GPU: the affine warp's position arithmetic at its matrix limits on an MI355X (tests/warp_limit_cases.py; zj_warp.h,
DESIGN.md 3.16): entries of +-2^31, offsets near +-2^55, first-tap indices beyond int32 on both sides, the clamp of warp_pos
from both sides, negative U at every edge of the two shifts.  The stage must equal the numpy model (tests/warp_model.py, shown
exact on these inputs by Python integers in warp_limit_cases.assert_cases) byte for byte, between guard bytes that stay
untouched; zj_warp_fixed and zj_warp_source_window must give the Python-integer values; the plane call and the file call under
limit matrices must equal the stage over the full decode."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import resize_model as rm
import warp_limit_cases as wl
import warp_model as wm
from test_gpu_crop_tensor import ESZ, GUARD, MODES, body, factors, frame_on_device, guarded, layout_code, run_u8_crops
from test_gpu_to_tensor import images_on_device
from test_gpu_warp import EDGES, differ, displayed_u8, model, run_planes, run_stage, warped_call

pytestmark = pytest.mark.gpu
NAMES = wl.names()
GROUPS = sorted({n.split("/")[0] for n in NAMES})
FRAME_COMBOS = [(rm.F32, "NHWC"), (rm.U8, "NCHW"), (rm.BF16, "NCHW"), (rm.F16, "NHWC")]


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def je():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import jpeg_enc
    return jpeg_enc


def run_stage_at(zj, ctx, torch, base, ptrs_, sizes, pitches, ch, ms, ow, oh, dtype, layout, scale, bias, fill, edge):
    """run_stage with the tensor `base` elements behind the guard: the bytes in front of it and behind it must stay as well"""
    E = ESZ[dtype]
    n = len(ptrs_) * ch * ow * oh * E
    buf = guarded(torch, n + 8 * E)
    ctx.warp_device(ptrs_, sizes, ch, ms, ow, oh, dtype, layout_code(zj, layout), buf.data_ptr() + GUARD + base * E, scale, bias, fill,
                    EDGES[edge], pitches)
    ctx.sync()
    whole = body(torch, buf, n + 8 * E)
    assert bool((whole[:base * E] == 0xAA).all()) and bool((whole[base * E + n:] == 0xAA).all()), "a byte beside the tensor was written"
    return whole[base * E:base * E + n]


def calls(group):
    """the group's cases, up to three of one source size, channel count and output size a call: [(first index, [cases])]"""
    runs = {}
    for k, c in enumerate(wl.cases()):
        if c["group"] == group:
            runs.setdefault((c["src"], c["ch"], c["out"]), []).append((k, c))
    return [(part[0][0], [c for _, c in part]) for run in runs.values() for part in (run[i:i + 3] for i in range(0, len(run), 3))]


# ---- 1. the stage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [wm.FILL, wm.REPLICATE], ids=["fill", "replicate"])
@pytest.mark.parametrize("group", GROUPS)
def test_stage_equals_the_model_at_the_limits(zj, ctx, torch, group, edge):
    ran = 0
    for k, cs in calls(group):
        c0 = cs[0]
        (w, h), ch, (ow, oh) = c0["src"], c0["ch"], c0["out"]
        combos, pad, base = wl.rotation(k)
        rng = np.random.default_rng(zlib.crc32(f"{c0['name']}-{edge}".encode()))
        pads, mis = [(0, 1, 13)[(k + i) % 3] for i in range(len(cs))], [(k + i) % 4 for i in range(len(cs))]
        dev, ptrs_, pitches, imgs = images_on_device(torch, rng, len(cs), w, h, ch, pads, mis)
        ms = [c["m"] for c in cs]
        for j, (dtype, layout) in enumerate(combos):
            scale, bias = factors(rng, ch)
            fill = wl.FILLS[(k + j) % 2]
            got = run_stage_at(zj, ctx, torch, (base + j) % 8, ptrs_, [(w, h)] * len(cs), pitches, ch, ms, ow, oh, dtype, layout, scale, bias,
                               fill, edge)
            differ(got, model(imgs, ms, ow, oh, dtype, layout, scale, bias, fill, edge),
                   f"{[c['name'] for c in cs]} dtype {dtype} {layout} pads {pads} misalign {mis} base {(base + j) % 8} edge {edge}")
        ran += len(cs)
    assert ran == sum(c["group"] == group for c in wl.cases())


def test_every_case_is_in_a_call():
    seen = [c["name"] for g in GROUPS for _, cs in calls(g) for c in cs]
    assert sorted(seen) == sorted(NAMES)


@pytest.mark.parametrize("ch", [1, 3])
def test_a_second_launch_packs_the_limit_matrices(zj, ctx, torch, ch):
    """49 images of their own sizes, one more than a launch holds, the limit matrices in turn"""
    rng = np.random.default_rng(4900 + ch)
    n = 49
    all_ms = wl.cycle_matrices()
    sizes = [[(1, 1), (2, 1), (5, 3), (7, 5), (258, 3)][i % 5] for i in range(n)]
    ms = [all_ms[i % len(all_ms)] for i in range(n)]
    host = [rng.integers(0, 256, (h, w, ch), dtype=np.uint8) for (w, h) in sizes]
    devs = [torch.from_numpy(im).cuda() for im in host]
    torch.cuda.synchronize()
    scale, bias = factors(rng, ch)
    for (dtype, layout, edge) in [(rm.F32, "NHWC", wm.REPLICATE), (rm.U8, "NCHW", wm.FILL), (rm.BF16, "NCHW", wm.REPLICATE)]:
        got = run_stage(zj, ctx, torch, [t.data_ptr() for t in devs], sizes, None, ch, ms, 65, 33, dtype, layout, scale, bias, wl.FILLS[1], edge)
        differ(got, model(host, ms, 65, 33, dtype, layout, scale, bias, wl.FILLS[1], edge), f"49 images C {ch} dtype {dtype} {layout} edge {edge}")


# ---- 2. the ABI's own host rules --------------------------------------------------------------------------------------
def test_the_abi_gives_the_python_integer_values(zj):
    L = zj.lib()
    win, sh = (C.c_uint * 4)(), (C.c_int64 * 6)()
    for c in wl.cases():
        assert zj.warp_fixed(c["m"]) == list(c["ints"]), c["name"]
        for (fw, fh) in wl.FRAMES:
            for edge in wl.BOTH:
                want = wl.window_ints(c["ints"], fw, fh, *c["out"], edge)
                assert zj.warp_source_window(c["ints"], fw, fh, *c["out"], EDGES[edge]) == want, (c["name"], fw, fh, edge)
                # (the shifted integers are integers the library takes again: warp_ints_valid's bound)
                assert L.zj_warp_source_window((C.c_int64 * 6)(*want[1]), fw, fh, *c["out"], edge, win, sh) == 0, (c["name"], fw, fh, edge)
    for (W, H) in ((96, 80), (48, 64)):
        for name, (ow, oh), m, _ in wl.frame_cases(W, H):
            q = wl.fixed_ints(m)
            assert zj.warp_fixed(m) == q, name
            for edge in wl.BOTH:
                assert zj.warp_source_window(q, W, H, ow, oh, EDGES[edge]) == wl.window_ints(q, W, H, ow, oh, edge), (name, edge)


# ---- 3. the plane call ------------------------------------------------------------------------------------------------
def by_output(W, H):
    runs = {}
    for name, out, m, kind in wl.frame_cases(W, H):
        runs.setdefault(out, []).append((name, m, kind))
    return runs


def all_fill(got, n, ow, oh, ch, E, layout):
    """every pixel of each of the n images is the image's first"""
    a = got.cpu().numpy().reshape((n, oh * ow, ch * E) if layout == "NHWC" else (n, ch, oh * ow, E))
    px = a[:, :1] if layout == "NHWC" else a[:, :, :1]
    return bool((a == px).all())


@pytest.mark.parametrize("mode", ["none", "hv"], ids=["444", "420"])
def test_plane_call_under_limit_matrices_equals_the_stage(zj, ctx, torch, synth, mode):
    hs, vs = MODES[mode]
    W, H = 96, 80
    wl.assert_frame_cases(W, H)
    rng = np.random.default_rng(zlib.crc32(f"warp-limit-planes-{mode}".encode()))
    d, dev = frame_on_device(zj, torch, synth, W, H, hs, vs, "rgb", 0, seed=31)
    full = run_u8_crops(zj, ctx, torch, d, [dev], [(0, 0)], W, H)[0]
    full_dev = torch.from_numpy(np.ascontiguousarray(full)).cuda()
    torch.cuda.synchronize()
    k = 0
    for (ow, oh), run in by_output(W, H).items():
        ms = [m for _, m, _ in run]
        for edge in wl.BOTH:
            dtype, layout = FRAME_COMBOS[k % 4]
            scale, bias = factors(rng, 3)
            fill = wl.FILLS[1]
            got = run_planes(zj, ctx, torch, d, [dev] * len(ms), 3, ms, ow, oh, dtype, layout, scale, bias, fill, edge)
            ref = run_stage(zj, ctx, torch, [full_dev.data_ptr()] * len(ms), [(W, H)] * len(ms), None, 3, ms, ow, oh, dtype, layout, scale, bias,
                            fill, edge)
            differ(got, ref, f"{mode} {[n for n, _, _ in run]} -> {ow}x{oh} dtype {dtype} {layout} edge {edge}")
            differ(ref, model([full] * len(ms), ms, ow, oh, dtype, layout, scale, bias, fill, edge), f"the stage over the full decode, edge {edge}")
            far = [i for i, (_, _, kind) in enumerate(run) if kind in ("corner", "column", "row")]
            if edge == wm.FILL and far:  # an empty window: nothing decoded, the output all fill
                per = 3 * ow * oh * ESZ[dtype]
                for i in far:
                    assert all_fill(got[i * per:(i + 1) * per], 1, ow, oh, 3, ESZ[dtype], layout), run[i][0]
            k += 1
    assert k == 8


# ---- 4. one file call -------------------------------------------------------------------------------------------------
def test_file_call_under_limit_matrices_equals_the_stage(zj, ctx, torch, synth, je):
    from test_gpu_to_tensor import colour_file, options
    import orient_model as om
    opt = options(zj)
    W, H, o = 64, 48, 6
    blob = colour_file(je, synth, W, H, 2, 2, 5, orientation=o)
    dw, dh = om.oriented_size(o, W, H)
    assert (dw, dh) == (48, 64)
    wl.assert_frame_cases(dw, dh)
    img = displayed_u8(zj, ctx, torch, blob, opt, dw, dh)
    shown = img.cpu().numpy().reshape(dh, dw, 3)
    rng = np.random.default_rng(66)
    k = 0
    for name, (ow, oh), m, kind in wl.frame_cases(dw, dh):
        for edge in wl.BOTH:
            dtype, layout = FRAME_COMBOS[k % 4]
            scale, bias = factors(rng, 3)
            rc, got, text = warped_call(zj, ctx, torch, blob, opt, m, ow, oh, dtype, layout, scale, bias, wl.FILLS[1], edge)
            assert rc == 0, (name, rc, text)
            ref = run_stage(zj, ctx, torch, [img.data_ptr()], [(dw, dh)], None, 3, [m], ow, oh, dtype, layout, scale, bias, wl.FILLS[1], edge)
            differ(got, ref, f"turned file, {name} edge {edge} dtype {dtype} {layout}")
            differ(ref, model([shown], [m], ow, oh, dtype, layout, scale, bias, wl.FILLS[1], edge), f"the stage over the displayed image, {name}")
            if edge == wm.FILL and kind in ("corner", "column", "row"):
                assert all_fill(got, 1, ow, oh, 3, ESZ[dtype], layout), name
            k += 1
    assert k == 22
