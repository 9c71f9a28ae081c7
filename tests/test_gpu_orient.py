"""GPU: EXIF orientation on an MI355X.  zj_orient_device against the numpy definition (tests/orient_model.py);
oriented resized crops against the EXISTING resize entry point run over the model's oriented copy of the bytes
zj_decode_crops_device (or the reduced decode) writes for the mapped stored window; the decoder's oriented outputs against
the model's orientation of its unoriented ones.  Every comparison is for equality of bytes."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import orient_model as om

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
T = 64          # the kernel's tile side (zj_orient.h: ORIENT_T; tests/test_orient_emu.py checks the constant)
BATCH = 128     # images per launch (ORIENT_BATCH)
GUARD = 256
FILL = 0xA5


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


def up(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()  # (the uploads are torch's, the reads the library's stream)
    return t


def shape_of(w, h, channels, chw):
    return (3, h, w) if chw else ((h, w, 3) if channels == 3 else (h, w))


# ---- 1, 2. zj_orient_device against the model ------------------------------------------------------------------------
def run_orient(zj, ctx, torch, imgs, oris, channels, chw, pad_in, pad_out):
    """imgs: host arrays [H, W, 3] / [H, W] / [3, H, W]; every output behind the one before with a guard between them"""
    bpp, npl = (1, 3) if chw else (channels, 1)
    n = len(imgs)
    ins, sizes, ipit, opit, offs = [], [], [], [], []
    at = GUARD
    for im, o in zip(imgs, oris):
        h, w = (im.shape[1], im.shape[2]) if chw else im.shape[:2]
        ip = (w * bpp + 127) // 128 * 128 if pad_in else w * bpp
        rows = np.full((npl, h, ip), 0x5A, np.uint8)
        rows[:, :, :w * bpp] = im.reshape(npl, h, w * bpp)
        ins.append(up(torch, rows))
        dw, dh = om.oriented_size(o, w, h)
        op = (dw * bpp + 127) // 128 * 128 + 4 if pad_out else dw * bpp
        sizes.append((w, h)); ipit.append(ip); opit.append(op); offs.append(at)
        at += op * dh * npl + GUARD + (0 if pad_out else 1)  # (tight: the next image starts at another alignment)
    buf = torch.full((at,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.orient_device([t.data_ptr() for t in ins], sizes, channels, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, oris,
                      [buf.data_ptr() + x for x in offs], ipit if pad_in else None, opit if pad_out else None)
    ctx.sync()
    a = buf.cpu().numpy()
    body = np.zeros(a.size, bool)
    for im, o, (w, h), op, off in zip(imgs, oris, sizes, opit, offs):
        dw, dh = om.oriented_size(o, w, h)
        assert zj.oriented_size(o, w, h) == (dw, dh)
        rows = a[off:off + op * dh * npl].reshape(npl, dh, op)
        exp = om.orient_chw(im, o) if chw else om.orient(im, o)
        assert np.array_equal(rows[:, :, :dw * bpp].reshape(exp.shape), exp), (w, h, o)
        body[off:off + op * dh * npl].reshape(npl, dh, op)[:, :, :dw * bpp] = True
    assert (a[~body] == FILL).all(), "padding or guard bytes written"


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("channels,chw", [(3, False), (1, False), (3, True)])
def test_orient_device_equals_the_model(zj, ctx, torch, channels, chw, padded):
    rng = np.random.default_rng(5 + channels + 2 * chw)
    sizes = [(1, 1), (1, 67), (67, 1), (T - 1, T + 1), (T + 1, T - 1), (130, 3), (3, 130)]
    imgs, oris = [], []
    for i, (w, h) in enumerate(sizes):
        for o in range(1, 9):
            imgs.append(rng.integers(0, 256, shape_of(w, h, channels, chw), dtype=np.uint8))
            oris.append(o)
    run_orient(zj, ctx, torch, imgs, oris, channels, chw, padded, padded)


def test_a_batch_one_larger_than_a_launch(zj, ctx, torch):
    rng = np.random.default_rng(2)
    n = BATCH + 1
    imgs = [rng.integers(0, 256, (3, 4, 3), dtype=np.uint8) for _ in range(n)]
    run_orient(zj, ctx, torch, imgs, [1 + i % 8 for i in range(n)], 3, False, False, False)


def test_no_orientation_is_a_copy(zj, ctx, torch):
    im = np.random.default_rng(1).integers(0, 256, (70, 90, 3), dtype=np.uint8)
    src = up(torch, im)
    dst = torch.zeros_like(src)
    ctx.orient_device([src.data_ptr()], [(90, 70)], 3, zj.LAYOUT_HWC, None, [dst.data_ptr()])
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), im)


# ---- 3. oriented resized crops ---------------------------------------------------------------------------------------
MODES = {"420": (2, 2), "444": (1, 1)}
_frames = {}


def frame(zj, torch, synth, mode, gray, W, H, chw=False):
    key = (mode, gray, W, H, chw)
    if key not in _frames:
        hs, vs = MODES[mode]
        planes, qts = synth.make_frame(W, H, hs, vs, 3, seed=W + H)
        d = zj.FrameDesc.make(W, H, hs, vs, 3, zj.ColorSpace.GRAYSCALE if gray else zj.ColorSpace.RGB, qts)
        d.out_layout = zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC
        _frames[key] = (d, [up(torch, np.ascontiguousarray(p, np.int16)) for p in planes], {})
    return _frames[key]


def stored_crop(zj, ctx, torch, d, dev, cache, win, scale=1):
    """the bytes the library's own crop (scale 1) or reduced-size decode writes for a stored window, on the host"""
    key = (win, scale)
    if key not in cache:
        x, y, w, h = win
        n = zj.crop_out_len(d, w, h) if scale == 1 else zj.scaled_crop_out_len(d, scale, w, h)
        buf = torch.empty((n,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        p = [t.data_ptr() for t in dev]
        if scale == 1:
            ctx.decode_crops_device(d, [p[0]], [p[1]], [p[2]], [(x, y)], w, h, [buf.data_ptr()])
        else:
            ctx.decode_crops_scaled_device(d, [p[0]], [p[1]], [p[2]], scale, [buf.data_ptr()], [win])
        ctx.sync()
        gray = d.out_colorspace == zj.ColorSpace.GRAYSCALE
        chw = d.out_layout == zj.LAYOUT_CHW and not gray
        cache[key] = buf.cpu().numpy().reshape(shape_of(w, h, 1 if gray else 3, chw))
    return cache[key]


def resize_ref(zj, ctx, torch, imgs, channels, chw, size, dtype, aa, flips=None):
    """the existing resize entry point over host images"""
    ow, oh = size
    ts = [up(torch, im) for im in imgs]
    sizes = [((im.shape[2], im.shape[1]) if chw else (im.shape[1], im.shape[0])) for im in imgs]
    esz = 4 if dtype == zj.DTYPE_F32 else 1
    out = torch.full((len(imgs) * channels * ow * oh * esz,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.resize_device([t.data_ptr() for t in ts], sizes, channels, zj.LAYOUT_CHW if chw else zj.LAYOUT_HWC, ow, oh, dtype,
                      zj.TENSOR_NCHW, out.data_ptr(), SCALE[:channels], BIAS[:channels], flips, None, None, aa)
    ctx.sync()
    return out.cpu().numpy()


def oriented(zj, ctx, torch, d, dev, wins, oris, channels, size, dtype, aa, flips=None, max_prescale=1):
    ow, oh = size
    n = len(wins)
    esz = 4 if dtype == zj.DTYPE_F32 else 1
    out = torch.full((n * channels * ow * oh * esz + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in dev]
    ctx.decode_crops_resized_device(d, [p[0]] * n, [p[1]] * n, [p[2]] * n, wins, ow, oh, dtype, zj.TENSOR_NCHW, out.data_ptr(),
                                    SCALE[:channels], BIAS[:channels], flips, None, aa, max_prescale, oris)
    ctx.sync()
    a = out.cpu().numpy()
    assert (a[-GUARD:] == FILL).all()
    return a[:-GUARD]


SCALE = [1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)]
BIAS = [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]


def displayed_windows(W, H):
    """per orientation: windows touching each corner of the DISPLAYED frame, and one inside"""
    wins, oris = [], []
    for o in range(1, 9):
        dw, dh = om.oriented_size(o, W, H)
        a, b = dw // 2 + 1, dh // 2 + 3
        for win in ((0, 0, a, b), (dw - a, 0, a, b), (0, dh - b, a, b), (dw - a, dh - b, a, b), (dw // 4, dh // 4, dw // 2, dh // 3)):
            wins.append(win)
            oris.append(o)
    return wins, oris


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("W,H", [(96, 80), (250, 70)])
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_oriented_resized_crops(zj, ctx, torch, synth, mode, gray, W, H, aa, dtype):
    """250 x 70: a ragged width, so the zero tail of the reference's RGB rows (Q5) lies inside S and turns with it"""
    d, dev, cache = frame(zj, torch, synth, mode, gray, W, H)
    ch = 1 if gray else 3
    dt = zj.DTYPE_U8 if dtype == "u8" else zj.DTYPE_F32
    wins, oris = displayed_windows(W, H)
    imgs = []
    for win, o in zip(wins, oris):
        st = om.stored_window(o, W, H, win)
        assert zj.orient_window(o, W, H, win) == st
        imgs.append(om.orient(stored_crop(zj, ctx, torch, d, dev, cache, st), o))
        assert imgs[-1].shape[:2] == (win[3], win[2])
    size = (24, 20)
    exp = resize_ref(zj, ctx, torch, imgs, ch, False, size, dt, aa)
    got = oriented(zj, ctx, torch, d, dev, wins, oris, ch, size, dt, aa)
    per = exp.size // len(wins)
    for i in range(len(wins)):
        assert np.array_equal(got[i * per:(i + 1) * per], exp[i * per:(i + 1) * per]), (wins[i], oris[i])


def test_oriented_resized_crops_of_planes(zj, ctx, torch, synth):
    """ZJ_LAYOUT_CHW: every plane of the crop is turned on its own"""
    W, H = 96, 80
    d, dev, cache = frame(zj, torch, synth, "420", False, W, H, chw=True)
    wins, oris = displayed_windows(W, H)
    imgs = [om.orient_chw(stored_crop(zj, ctx, torch, d, dev, cache, om.stored_window(o, W, H, win)), o) for win, o in zip(wins, oris)]
    exp = resize_ref(zj, ctx, torch, imgs, 3, True, (24, 20), zj.DTYPE_F32, True)
    assert np.array_equal(oriented(zj, ctx, torch, d, dev, wins, oris, 3, (24, 20), zj.DTYPE_F32, True), exp)


def prescale_pick(w, h, ow, oh, max_log2):
    k = 0
    for c in range(1, max_log2 + 1):
        if (w >> c) >= ow and (h >> c) >= oh:
            k = c
    return k


def prescale_window(win, k, W, H):
    x, y, w, h = win
    s = 1 << k
    rw, rh = -(-W // s), -(-H // s)
    x1, y1 = min(-(-(x + w) // s), rw), min(-(-(y + h) // s), rh)
    return (x // s, y // s, x1 - x // s, y1 - y // s)


@pytest.mark.parametrize("aa", [False, True])
def test_oriented_prescaled_crops(zj, ctx, torch, synth, aa):
    """the reduced crop of the STORED window, at the scale picked from the displayed window's sides, turned, then resized"""
    W, H = 400, 304
    d, dev, cache = frame(zj, torch, synth, "420", False, W, H)
    size = (40, 30)
    wins, oris, imgs, scales = [], [], [], []
    for o in range(1, 9):
        dw, dh = om.oriented_size(o, W, H)
        for win in ((0, 0, dw, dh), (dw - 171, dh - 133, 171, 133), (3, 5, 85, 61), (dw // 2, 1, 79, 75)):
            st = om.stored_window(o, W, H, win)
            k = prescale_pick(win[2], win[3], size[0], size[1], 2)
            crop = stored_crop(zj, ctx, torch, d, dev, cache, prescale_window(st, k, W, H), 1 << k) if k else \
                stored_crop(zj, ctx, torch, d, dev, cache, st)
            wins.append(win); oris.append(o); scales.append(k)
            imgs.append(om.orient(crop, o))
    assert set(scales) == {0, 1, 2}
    exp = resize_ref(zj, ctx, torch, imgs, 3, False, size, zj.DTYPE_F32, aa)
    got = oriented(zj, ctx, torch, d, dev, wins, oris, 3, size, zj.DTYPE_F32, aa, max_prescale=4)
    per = exp.size // len(wins)
    for i in range(len(wins)):
        assert np.array_equal(got[i * per:(i + 1) * per], exp[i * per:(i + 1) * per]), (wins[i], oris[i], scales[i])


def test_null_orientation_is_the_prescaled_call_and_flip_composes(zj, ctx, torch, synth):
    W, H = 250, 70
    d, dev, cache = frame(zj, torch, synth, "420", False, W, H)
    wins = [(0, 0, 250, 70), (100, 7, 150, 63), (1, 1, 97, 50)]
    n, size = len(wins), (30, 16)
    base = oriented(zj, ctx, torch, d, dev, wins, None, 3, size, zj.DTYPE_U8, True, max_prescale=2)
    out = torch.full((base.size,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in dev]
    arr = lambda v: (C.c_void_p * n)(*([v] * n))
    win = (C.c_uint * (4 * n))(*[v for w in wins for v in w])
    sc, bi = (C.c_float * 3)(*SCALE), (C.c_float * 3)(*BIAS)
    rc = zj.lib().zj_decode_crops_resized_oriented_device(ctx.handle, C.byref(d), n, arr(p[0]), arr(p[1]), arr(p[2]), win, size[0],
                                                          size[1], zj.DTYPE_U8, zj.TENSOR_NCHW, sc, bi, None,
                                                          zj.RESIZE_BILINEAR_AA, 1, None, out.data_ptr(), None)
    assert rc == 0
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), base)
    ones = oriented(zj, ctx, torch, d, dev, wins, [1] * n, 3, size, zj.DTYPE_U8, True, max_prescale=2)
    assert np.array_equal(ones, base)
    # flip: a mirror of the output's columns, after everything else
    dwins = [(0, 0, 70, 250), (5, 100, 60, 150), (1, 1, 50, 97)]
    for aa in (False, True):
        plain = oriented(zj, ctx, torch, d, dev, dwins, [6, 5, 8], 3, size, zj.DTYPE_F32, aa)
        flipped = oriented(zj, ctx, torch, d, dev, dwins, [6, 5, 8], 3, size, zj.DTYPE_F32, aa, flips=[True] * n)
        shape = (n, 3, size[1], size[0])
        assert np.array_equal(flipped.view(np.float32).reshape(shape), plain.view(np.float32).reshape(shape)[..., ::-1])


# ---- 4. files --------------------------------------------------------------------------------------------------------
def file_case(zj, ctx, torch, data, entropy, o):
    opt = zj.ZuneJpegOptions()
    opt.entropy = entropy
    dec = zj.Decoder(opt, ctx)
    try:
        desc, info = dec.prepare(data)
        assert dec.orientation == o
        W, H = info.width, info.height
        n = W * H * 3
        buf = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert dec.finish_pixels_device(buf.data_ptr(), n) == n
        S = buf.cpu().numpy()[:n].reshape(H, W, 3).copy()
        dec.prepare(data)
        buf.fill_(FILL)
        torch.cuda.synchronize()
        ln, dw, dh = dec.finish_pixels_device(buf.data_ptr(), n, apply_orientation=True)
        a = buf.cpu().numpy()
        assert (ln, dw, dh) == (n, *om.oriented_size(o, W, H)) and (a[n:] == FILL).all()
        assert np.array_equal(a[:n].reshape(dh, dw, 3), om.orient(S, o))
        # a 700 x 500 window of the displayed image -> 224 x 224
        win = (dw - 700 - 3, 5, 700, 500) if dw >= 800 else (7, dh - 500 - 11, 700, 500)
        st = om.stored_window(o, W, H, win)
        crop = torch.empty((st[2] * st[3] * 3,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dec.prepare(data)
        dec.finish_pixels_crop_device(*st, crop.data_ptr(), crop.numel())
        assert np.array_equal(crop.cpu().numpy().reshape(st[3], st[2], 3), S[st[1]:st[1] + st[3], st[0]:st[0] + st[2]])
        img = om.orient(crop.cpu().numpy().reshape(st[3], st[2], 3), o)
        for aa in (False, True):
            exp = resize_ref(zj, ctx, torch, [img], 3, False, (224, 224), zj.DTYPE_F32, aa)
            out = torch.full((exp.size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dec.prepare(data)
            got = dec.finish_pixels_resized_crop_device(*win, 224, 224, zj.DTYPE_F32, zj.TENSOR_NCHW, out.data_ptr(), exp.size,
                                                        SCALE, BIAS, antialias=aa, apply_orientation=True)
            b = out.cpu().numpy()
            assert got == exp.size and np.array_equal(b[:exp.size], exp) and (b[exp.size:] == FILL).all()
    finally:
        dec.close()


@pytest.mark.parametrize("entropy", ["cpu", "gpu"])
@pytest.mark.parametrize("o", range(2, 9))
def test_baseline_file_with_each_orientation(zj, ctx, torch, o, entropy):
    data = om.splice(open(os.path.join(GOLD, "test-baseline.jpg"), "rb").read(), om.exif_segment(o, "<>"[o % 2]))
    file_case(zj, ctx, torch, data, zj.ENTROPY_CPU if entropy == "cpu" else zj.ENTROPY_GPU_ALWAYS, o)


def test_progressive_file_with_orientation_6(zj, ctx, torch):
    data = om.splice(open(os.path.join(GOLD, "test-progressive.jpg"), "rb").read(), om.exif_segment(6))
    file_case(zj, ctx, torch, data, zj.ENTROPY_CPU, 6)


def test_a_file_without_orientation_decodes_straight_into_the_output(zj, ctx, torch):
    data = open(os.path.join(GOLD, "test-baseline.jpg"), "rb").read()
    dec = zj.Decoder(None, ctx)
    desc, info = dec.prepare(data)
    n = info.width * info.height * 3
    a, b = (torch.full((n,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    assert dec.finish_pixels_device(a.data_ptr(), n) == n
    dec.prepare(data)
    assert dec.finish_pixels_device(b.data_ptr(), n, apply_orientation=True) == (n, info.width, info.height)
    assert torch.equal(a, b)
    dec.close()


# ---- 5. argument errors launch nothing -------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(zj, ctx, torch, synth):
    W, H = 96, 80
    d, dev, _ = frame(zj, torch, synth, "420", False, W, H)
    p = [t.data_ptr() for t in dev]
    out = torch.full((2 * 3 * 16 * 16,), FILL, dtype=torch.uint8, device="cuda")
    src = up(torch, np.zeros((8, 8, 3), np.uint8))
    torch.cuda.synchronize()

    def crops(wins, oris, desc=d):
        n = len(wins)
        ctx.decode_crops_resized_device(desc, [p[0]] * n, [p[1]] * n, [p[2]] * n, wins, 16, 16, zj.DTYPE_U8, zj.TENSOR_NCHW,
                                        out.data_ptr(), orientations=oris)

    for bad in (0, 9):
        with pytest.raises(zj.ZjError) as e:
            crops([(0, 0, 32, 32), (0, 0, 32, 32)], [1, bad])
        assert e.value.status == -1
        with pytest.raises(zj.ZjError) as e:
            ctx.orient_device([src.data_ptr()] * 2, [(8, 8)] * 2, 3, zj.LAYOUT_HWC, [6, bad], [out.data_ptr(), out.data_ptr() + 192])
        assert e.value.status == -1
    # inside the stored 96 x 80 frame, outside the displayed 80 x 96 one
    with pytest.raises(zj.ZjError) as e:
        crops([(0, 0, 32, 32), (60, 0, 30, 10)], [6, 6])
    assert e.value.status == -1
    crops([(0, 0, 32, 32), (60, 0, 30, 10)], [6, 1])  # (the same window of the frame as it is stored is one)
    ctx.sync()
    out.fill_(FILL)
    torch.cuda.synchronize()
    planes, qts = synth.make_frame(W, H, 2, 2, 3, seed=W + H)
    rgba = zj.FrameDesc.make(W, H, 2, 2, 3, zj.ColorSpace.RGBA, qts)
    with pytest.raises(zj.ZjError) as e:
        crops([(0, 0, 32, 32)], [6], rgba)
    assert e.value.status == -2
    with pytest.raises(zj.ZjError) as e:
        ctx.orient_device([src.data_ptr()], [(8, 8)], 4, zj.LAYOUT_HWC, [6], [out.data_ptr()])
    assert e.value.status == -1
    ctx.sync()
    assert (out.cpu().numpy() == FILL).all(), "something was launched after an argument error"
