"""GPU: frames and files of mixed geometry into one resized-crop tensor on an MI355X.
zj_decode_crops_resized_mixed_device against zj_decode_crops_resized_oriented_device run for each frame alone, and
zj_decoder_finish_pixels_resized_crop_batch_device / tensors.decode_files_resized_to_tensor against the single-file call,
in the same process.  Every comparison is torch.equal on the outputs' bytes: there are no tolerances."""
import ctypes as C
import importlib
import io
import os

import numpy as np
import pytest

import orient_model as om

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MODES = {"444": (1, 1), "422": (2, 1), "440": (1, 2), "420": (2, 2)}
FILL = 0xA5
ERR_ARG = -1


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def tz():
    return importlib.import_module("zune-jpeg_amd.tensors")


@pytest.fixture(scope="module")
def synth():
    return importlib.import_module("zune-jpeg_amd.synth")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)
    yield c
    c.close()


class Frame:
    """one frame: its descriptor and its planes in device memory"""

    def __init__(self, zj, torch, synth, w, h, mode="420", cs=None, layout=0, flags=0, seed=1, quality=90, in_comp=3):
        hs, vs = MODES[mode] if in_comp == 3 else (1, 1)
        planes, qts = synth.make_frame(w, h, hs, vs, in_comp, seed=seed, quality=quality)
        cs = zj.ColorSpace.RGB if cs is None else cs
        self.desc = zj.FrameDesc.make(w, h, hs, vs, in_comp, cs, qts, flags=flags, out_layout=layout)
        self.planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]
        self.w, self.h = w, h

    def ptr(self, c):
        return self.planes[c].data_ptr() if c < len(self.planes) else None


def tdtype(torch, name):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}[name]


def filled(torch, n, channels, size, dtype, layout):
    """an output of n images pre-filled with a byte pattern"""
    ow, oh = size
    shape = (n, channels, oh, ow) if layout == "NCHW" else (n, oh, ow, channels)
    numel = int(np.prod(shape))
    raw = torch.full((numel * torch.empty((), dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device="cuda")
    return raw, raw.view(dtype).view(shape)


def mixed_vs_single(zj, tz, ctx, torch, frames, windows, size=(16, 12), dtype="f32", layout="NCHW", antialias=False,
                    interpolation="bilinear", max_prescale=1, oris=None, flips=None, mean=None, std=None):
    """ONE mixed call over all frames; then the one-geometry call for each frame alone; equal bytes image by image"""
    n = len(frames)
    dt = tdtype(torch, dtype)
    code = tz._resize_dtype(dt)
    channels = zj.ColorSpace(frames[0].desc.out_colorspace).num_components()
    scale, bias = tz.normalize_factors(channels, mean, std)
    lay = zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC
    raw, out = filled(torch, n, channels, size, dt, layout)
    torch.cuda.synchronize()
    ctx.decode_crops_resized_mixed_device([f.desc for f in frames], [f.ptr(0) for f in frames], [f.ptr(1) for f in frames],
                                          [f.ptr(2) for f in frames], windows, size[0], size[1], code, lay, out.data_ptr(),
                                          scale, bias, flips, None, antialias, max_prescale, oris, interpolation)
    ctx.sync()
    for i, f in enumerate(frames):
        _, one = filled(torch, 1, channels, size, dt, layout)
        torch.cuda.synchronize()
        ctx.decode_crops_resized_device(f.desc, [f.ptr(0)], [f.ptr(1)], [f.ptr(2)], [windows[i]], size[0], size[1], code, lay,
                                        one.data_ptr(), scale, bias, [flips[i]] if flips is not None else None, None, antialias,
                                        max_prescale, [oris[i]] if oris is not None else None, interpolation)
        ctx.sync()
        assert torch.equal(out[i].view(torch.uint8), one[0].view(torch.uint8)), \
            f"image {i}: {f.w}x{f.h} window {windows[i]} differs from the single-frame call"
        assert not bool((one[0].view(torch.uint8) == FILL).all()), "the single-frame call wrote nothing"
    return out


def whole(frames):
    return [(0, 0, f.w, f.h) for f in frames]


# ---- the planes entry point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["420", "422"])
def test_tile_seams_and_row_ends(zj, tz, ctx, torch, synth, mode):
    """widths below the generic threshold (17, 33), around a 256-pixel tile (255, 256, 257, 261: the hole case, 272: the
    tail on a tile boundary) and 500, all in one call; whole frames, then each row's last pixels"""
    widths = [17, 33, 255, 256, 257, 261, 272, 500]
    frames = [Frame(zj, torch, synth, w, 24 + 8 * (i % 3), mode, seed=i, quality=50 + 5 * i) for i, w in enumerate(widths)]
    mixed_vs_single(zj, tz, ctx, torch, frames, whole(frames))
    mixed_vs_single(zj, tz, ctx, torch, frames, [(f.w - min(f.w, 30), 1, min(f.w, 30), f.h - 1) for f in frames], dtype="u8",
                    layout="NHWC")


@pytest.mark.parametrize("mode", ["420", "440"])
def test_dropped_mcu_rows_beside_complete_ones(zj, tz, ctx, torch, synth, mode):
    """heights 40 and 72 beside 32 and 64: the rows below each frame's own last complete strip are that frame's zeros"""
    frames = [Frame(zj, torch, synth, 48 + 16 * i, h, mode, seed=20 + i) for i, h in enumerate([40, 32, 72, 64])]
    out = mixed_vs_single(zj, tz, ctx, torch, frames, whole(frames), size=(48, 40), dtype="u8", layout="NHWC")
    if mode == "420":
        assert (out[0][32:] == 0).all() and bool(out[0][:32].any())  # (48 x 40 -> 48 x 40: the resize is the identity)
    mixed_vs_single(zj, tz, ctx, torch, frames, [(3, f.h - 9, 20, 9) for f in frames])


@pytest.mark.parametrize("layout", [0, 1])
def test_every_mode_tables_and_flags_in_one_call(zj, tz, ctx, torch, synth, layout):
    modes = ["444", "422", "440", "420", "420", "444", "422", "440"]
    frames = [Frame(zj, torch, synth, 70 + 37 * i, 40 + 11 * i, m, layout=layout, flags=zj.FLAG_CORRECTED if i % 2 else 0,
                    seed=30 + i, quality=30 + 9 * i) for i, m in enumerate(modes)]
    mixed_vs_single(zj, tz, ctx, torch, frames, whole(frames), dtype="bf16", antialias=True,
                    mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])


def test_ycbcr_output_in_every_mode(zj, tz, ctx, torch, synth):
    frames = [Frame(zj, torch, synth, 261 + 30 * i, 33 + 14 * i, m, cs=zj.ColorSpace.YCbCr, seed=45 + i, quality=45 + 10 * i,
                    flags=zj.FLAG_CORRECTED if i == 1 else 0) for i, m in enumerate(["422", "444", "440", "420", "422"])]
    mixed_vs_single(zj, tz, ctx, torch, frames, whole(frames), dtype="u8")
    mixed_vs_single(zj, tz, ctx, torch, frames, [(f.w - 40, 2, 40, f.h - 3) for f in frames], max_prescale=4, size=(9, 7))


def test_grayscale_run_with_a_single_component_frame(zj, tz, ctx, torch, synth):
    g = zj.ColorSpace.GRAYSCALE
    frames = [Frame(zj, torch, synth, 64, 40, "444", cs=g, in_comp=1, seed=40), Frame(zj, torch, synth, 96, 72, "420", cs=g, seed=41),
              Frame(zj, torch, synth, 272, 33, "422", cs=g, seed=42, flags=zj.FLAG_CORRECTED), Frame(zj, torch, synth, 48, 48, "440", cs=g, seed=43)]
    mixed_vs_single(zj, tz, ctx, torch, frames, whole(frames), antialias=True, interpolation="bicubic")


def test_windows(zj, tz, ctx, torch, synth):
    """the whole frame, the bottom-right corner in the last strip, 1 x 1, and exactly out_w x out_h"""
    size = (16, 12)
    frames = [Frame(zj, torch, synth, 261 + 20 * i, 50 + 9 * i, m, seed=50 + i) for i, m in enumerate(["420", "444", "422", "440"])]
    for pick in range(4):
        wins = []
        for i, f in enumerate(frames):
            wins.append([(0, 0, f.w, f.h), (f.w - 7, f.h - 5, 7, 5), (f.w // 2, f.h // 3, 1, 1),
                         (f.w - size[0] - 3, 2, size[0], size[1])][(pick + i) % 4])
        mixed_vs_single(zj, tz, ctx, torch, frames, wins, size=size, antialias=pick % 2 == 1)


@pytest.mark.parametrize("layout", [0, 1])
def test_orientations_1_to_8_with_flips(zj, tz, ctx, torch, synth, layout):
    frames = [Frame(zj, torch, synth, 60 + 23 * o, 44 + 10 * o, ["420", "422", "444", "440"][o % 4], layout=layout, seed=60 + o)
              for o in range(1, 9)]
    oris = list(range(1, 9))
    wins = []
    for f, o in zip(frames, oris):
        dw, dh = om.oriented_size(o, f.w, f.h)
        wins.append((3, 2, dw - 7, dh - 5))
    mixed_vs_single(zj, tz, ctx, torch, frames, wins, oris=oris, flips=[o % 3 == 0 for o in oris], dtype="bf16", layout="NHWC")
    mixed_vs_single(zj, tz, ctx, torch, frames, wins, oris=oris, max_prescale=8, size=(9, 7))


@pytest.mark.parametrize("interp", ["bilinear", "aa", "bicubic"])
def test_prescale_puts_every_scale_into_one_group(zj, tz, ctx, torch, synth, interp):
    size = (16, 12)
    spec = [("420", 300, 200, (5, 3, 20, 14)), ("420", 300, 200, (5, 3, 40, 30)), ("420", 310, 220, (1, 1, 70, 50)),
            ("420", 321, 231, (0, 0, 321, 231)), ("444", 200, 150, (9, 9, 140, 100)), ("422", 270, 120, (2, 0, 268, 120)),
            ("440", 150, 290, (10, 20, 66, 50)), ("444", 90, 90, (0, 0, 16, 12))]
    frames = [Frame(zj, torch, synth, w, h, m, seed=70 + i, quality=40 + 7 * i, flags=zj.FLAG_CORRECTED if i % 3 == 0 else 0)
              for i, (m, w, h, _) in enumerate(spec)]
    wins = [s[3] for s in spec]
    ks = {max(k for k in range(4) if (w[2] >> k) >= size[0] and (w[3] >> k) >= size[1]) for w in wins}  # prescale_pick
    assert ks == {0, 1, 2, 3}
    mixed_vs_single(zj, tz, ctx, torch, frames, wins, size=size, max_prescale=8, antialias=interp != "bilinear",
                    interpolation="bicubic" if interp == "bicubic" else "bilinear", dtype="f32" if interp == "bilinear" else "u8")


def test_40_frames_pass_the_scattered_limit(zj, tz, ctx, torch, synth):
    assert zj.SCATTER_MAX < 40
    frames = [Frame(zj, torch, synth, 48, 48, "420", seed=100 + i, quality=30 + i) for i in range(40)]
    mixed_vs_single(zj, tz, ctx, torch, frames, [(i % 7, i % 5, 48 - i % 7, 48 - i % 5) for i in range(40)], size=(8, 8))


def test_130_frames_pass_a_resize_launch(zj, tz, ctx, torch, synth):
    frames = [Frame(zj, torch, synth, 16 + (7 * i) % 49, 16 + (5 * i) % 33, ["420", "444", "422", "440"][i % 4], seed=200 + i)
              for i in range(130)]
    oris = [1 + i % 8 for i in range(130)]
    wins = []
    for f, o in zip(frames, oris):
        dw, dh = om.oriented_size(o, f.w, f.h)
        wins.append((0, 0, dw, dh))
    mixed_vs_single(zj, tz, ctx, torch, frames, wins, size=(8, 8), oris=oris, dtype="u8")


def test_crops_beyond_one_scratch_group(zj, tz, ctx, torch):
    """two windows of 9600 x 9600 and 9600 x 9400 RGB pixels: 276 MB and 271 MB of crop bytes, each a launch group (256 MB) of
    its own, the table and the buffer reused between them.  The planes are random small integers made on the device, the
    same buffers under both descriptors."""
    w, h = 9600, 9600
    qt = [np.full(64, 3, np.int32)] * 3
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    ylen, clen = (w // 16) * (h // 16) * 4 * 64, (w // 16) * (h // 16) * 64
    planes = [torch.randint(-6, 7, (n,), dtype=torch.int16, device="cuda", generator=g) for n in (ylen, clen, clen)]

    class Big:
        def __init__(self, hh):
            self.desc = zj.FrameDesc.make(w, hh, 2, 2, 3, zj.ColorSpace.RGB, qt)
            self.w, self.h = w, hh

        def ptr(self, c):
            return planes[c].data_ptr()

    frames = [Big(9600), Big(9400)]
    mixed_vs_single(zj, tz, ctx, torch, frames, whole(frames), size=(32, 32), antialias=True)


def test_one_bad_frame_in_the_middle_launches_nothing(zj, tz, ctx, torch, synth):
    frames = [Frame(zj, torch, synth, 40 + 8 * i, 32, "420", seed=i) for i in range(5)]
    wins = whole(frames)
    raw, out = filled(torch, 5, 3, (8, 8), torch.float32, "NCHW")
    torch.cuda.synchronize()

    def call(descs, wins, oris=None):
        n = len(descs)
        arr = lambda c: (C.c_void_p * n)(*[f.ptr(c) for f in frames])
        rc = zj.lib().zj_decode_crops_resized_mixed_device(
            ctx.handle, (zj.FrameDesc * n)(*descs), n, arr(0), arr(1), arr(2), (C.c_uint * (4 * n))(*[v for w in wins for v in w]),
            8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, None, None, None, zj.RESIZE_BILINEAR, 0,
            (C.c_uint8 * n)(*oris) if oris else None, out.data_ptr(), None)
        ctx.sync()
        return rc

    descs = [f.desc for f in frames]
    bad = list(wins)
    bad[2] = (1, 0, frames[2].w, frames[2].h)
    assert call(descs, bad) == ERR_ARG
    assert call(descs, wins, [1, 2, 9, 4, 5]) == ERR_ARG
    import copy
    other = [copy.copy(d) for d in descs]
    other[3].out_colorspace = int(zj.ColorSpace.YCbCr)
    assert call(other, wins) == ERR_ARG
    assert bool((raw == FILL).all()), "a refused call wrote to the output"
    assert call(descs, wins) == 0 and not bool((raw == FILL).all())


# ---- files ------------------------------------------------------------------------------------------------------------
def pillow_file(w, h, subsampling, quality, seed, orientation=None, gray=False):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 3 + yy * 2 + seed * 17) % 256, (xx * yy // 7 + 40 * seed) % 256, (255 - xx - 2 * yy) % 256], -1)
    img = (img + rng.integers(0, 24, img.shape)).clip(0, 255).astype(np.uint8)
    buf = io.BytesIO()
    if gray:
        Image.fromarray(img[..., 0]).save(buf, "JPEG", quality=quality)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    data = buf.getvalue()
    return om.splice(data, om.exif_segment(orientation)) if orientation else data


def synthetic_files():
    spec = [(200, 150, "4:2:0", 85, 6), (333, 201, "4:4:4", 60, 3), (97, 260, "4:2:2", 92, 8), (640, 427, "4:2:0", 75, None),
            (45, 31, "4:4:4", 50, 5), (258, 64, "4:2:0", 95, 2), (120, 500, "4:2:2", 70, 7), (301, 299, "4:2:0", 40, 4)]
    return [pillow_file(w, h, s, q, i, o) for i, (w, h, s, q, o) in enumerate(spec)]


def golden_files():
    names = ["test-baseline.jpg", "test-progressive.jpg", "ref/medium_horiz_samp_2500x1786.jpg", "ref/medium_no_samp_2500x1786.jpg",
             "ref/medium_vertical_samp_2500x1786.jpg"]
    return [open(os.path.join(GOLD, n), "rb").read() for n in names]


def files_vs_single(zj, tz, ctx, torch, blobs, windows, size, options, apply_orientation, max_prescale=1, antialias=False,
                    interpolation="bilinear", dtype=None, layout="NCHW", workers=1, flips=None):
    dtype = torch.float32 if dtype is None else dtype
    out = tz.decode_files_resized_to_tensor(ctx, blobs, windows, size, dtype=dtype, layout=layout, flips=flips,
                                            antialias=antialias, interpolation=interpolation, max_prescale=max_prescale,
                                            apply_orientation=apply_orientation, options=options, workers=workers)
    code = tz._resize_dtype(dtype)
    lay = zj.TENSOR_NCHW if layout == "NCHW" else zj.TENSOR_NHWC
    scale, bias = tz.normalize_factors(3, None, None)  # (the tensor call's: the [0, 1] image)
    for k, blob in enumerate(blobs):
        dec = zj.Decoder(options, ctx)
        _, info = dec.prepare(blob)
        w = windows[k] if windows is not None and windows[k] is not None else None
        if w is None:
            iw, ih = int(info.width), int(info.height)
            w = (0, 0) + (zj.oriented_size(dec.orientation, iw, ih) if apply_orientation else (iw, ih))
        one = torch.empty_like(out[k:k + 1])
        torch.cuda.synchronize()
        dec.finish_pixels_resized_crop_device(w[0], w[1], w[2], w[3], size[0], size[1], code, lay, one.data_ptr(),
                                              one.numel() * one.element_size(), scale, bias, bool(flips[k]) if flips else False,
                                              antialias, max_prescale, apply_orientation, interpolation)
        dec.close()
        assert torch.equal(out[k].view(torch.uint8), one[0].view(torch.uint8)), f"file {k} differs from the single-file call"
    return out


def entropy_options(zj, entropy):
    o = zj.ZuneJpegOptions()
    o.entropy = getattr(zj, entropy)
    return o


@pytest.mark.parametrize("gpu_entropy", ["ENTROPY_CPU", "ENTROPY_GPU"])
def test_golden_files_in_one_batch(zj, tz, ctx, torch, gpu_entropy):
    blobs = golden_files()
    wins = [None, (100, 50, 900, 700), (1200, 800, 1300, 986), None, (7, 9, 2400, 1700)]
    files_vs_single(zj, tz, ctx, torch, blobs, wins, (64, 48), entropy_options(zj, gpu_entropy), False, max_prescale=8,
                    antialias=True)


@pytest.mark.parametrize("gpu_entropy", ["ENTROPY_CPU", "ENTROPY_GPU", "ENTROPY_GPU_ALWAYS"])
def test_synthetic_files_with_exif_orientations(zj, tz, ctx, torch, gpu_entropy):
    blobs = synthetic_files()
    opt = entropy_options(zj, gpu_entropy)
    files_vs_single(zj, tz, ctx, torch, blobs, None, (32, 24), opt, True, dtype=torch.bfloat16, layout="NHWC")
    wins = [(3, 5, 40, 30)] * len(blobs)
    wins[4] = None
    files_vs_single(zj, tz, ctx, torch, blobs, wins, (16, 16), opt, True, max_prescale=2, antialias=True, interpolation="bicubic",
                    flips=[k % 2 == 1 for k in range(len(blobs))])
    files_vs_single(zj, tz, ctx, torch, blobs, wins, (16, 16), opt, False, dtype=torch.uint8)


def test_workers_4_equals_workers_1(zj, tz, ctx, torch):
    blobs = synthetic_files() * 3
    a = tz.decode_files_resized_to_tensor(ctx, blobs, None, (24, 24), apply_orientation=True, workers=1)
    keep = []
    b = tz.decode_files_resized_to_tensor(ctx, blobs, None, (24, 24), apply_orientation=True, workers=4, decoders=keep)
    c = tz.decode_files_resized_to_tensor(ctx, blobs, None, (24, 24), apply_orientation=True, workers=4, decoders=keep)
    assert len(keep) == len(blobs)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8), c.view(torch.uint8))


def test_a_damaged_file_leaves_its_slot_and_stops_nobody(zj, tz, ctx, torch):
    blobs = synthetic_files()[:5]
    k_bad = 2
    bad = blobs[k_bad]
    blobs_bad = list(blobs)
    blobs_bad[k_bad] = bad[:120]  # cut inside its tables: prepare fails, the decoder has nothing to finish
    decs = []
    for b in blobs_bad:
        d = zj.Decoder(None, ctx)
        try:
            d.prepare(b)
        except zj.DecodeError:
            pass
        decs.append(d)
    size, n = (16, 16), len(blobs)
    raw, out = filled(torch, n, 3, size, torch.float32, "NCHW")
    torch.cuda.synchronize()
    wins = [(0, 0, 40, 30)] * n
    scale, bias = tz.normalize_factors(3, None, None)  # (the tensor call's, for the comparison below)
    rcs = zj.finish_pixels_resized_crop_batch(decs, ctx, wins, size[0], size[1], zj.DTYPE_F32, zj.TENSOR_NCHW, out.data_ptr(),
                                              raw.numel(), scale, bias)
    assert rcs[k_bad] != 0 and all(rc == 0 for k, rc in enumerate(rcs) if k != k_bad), rcs
    img = raw.numel() // n
    assert bool((raw[k_bad * img:(k_bad + 1) * img] == FILL).all()), "the failed file's slot was written"
    good = [b for k, b in enumerate(blobs) if k != k_bad]
    ref = tz.decode_files_resized_to_tensor(ctx, good, [(0, 0, 40, 30)] * len(good), size, dtype=torch.float32)
    got = torch.cat([out[:k_bad], out[k_bad + 1:]])
    assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8))
    with pytest.raises(zj.DecodeError, match=f"file {k_bad}"):
        tz.decode_files_resized_to_tensor(ctx, blobs_bad, wins, size)
    for d in decs:
        d.close()


def test_batch_call_errors_of_its_own(zj, ctx, torch):
    blobs = synthetic_files()[:2]
    o = zj.ZuneJpegOptions()
    o.out_colorspace = zj.ColorSpace.YCbCr
    decs = [zj.Decoder(None, ctx), zj.Decoder(o, ctx)]
    for d, b in zip(decs, blobs):
        d.prepare(b)
    raw, out = filled(torch, 2, 3, (8, 8), torch.float32, "NCHW")
    torch.cuda.synchronize()
    wins = [(0, 0, 8, 8)] * 2
    with pytest.raises(zj.ZjError):   # colour spaces differ
        zj.finish_pixels_resized_crop_batch(decs, ctx, wins, 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, out.data_ptr(), raw.numel())
    with pytest.raises(zj.ZjError):   # room for one image only
        zj.finish_pixels_resized_crop_batch(decs[:1] * 2, ctx, wins, 8, 8, zj.DTYPE_F32, zj.TENSOR_NCHW, out.data_ptr(),
                                            raw.numel() // 2)
    assert bool((raw == FILL).all())
    for d in decs:
        d.close()
