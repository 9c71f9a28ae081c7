"""GPU: the tensor helpers with EXIF orientation (tensors.orient_to_tensor, orientations= on resize_to_tensor and
decode_resized_crops_to_tensor): equal to torch.rot90 / flip / transpose of the unoriented result, taken through the u8 crop
as DESIGN.md 3.8 defines it (orient first, then resize)."""
import importlib

import numpy as np
import pytest

import orient_model as om

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def zt():
    return importlib.import_module("zune-jpeg_amd.tensors")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)
    yield c
    c.close()


def torch_orient(torch, t, o, hdim, wdim):
    """EXIF orientation o of a tensor whose rows / columns are the dimensions hdim / wdim, in torch's own operations"""
    if o == 1:
        return t
    if o == 2:
        return t.flip(wdim)
    if o == 3:
        return torch.rot90(t, 2, (hdim, wdim))
    if o == 4:
        return t.flip(hdim)
    if o == 5:
        return t.transpose(hdim, wdim)
    if o == 6:
        return torch.rot90(t, -1, (hdim, wdim))   # 90 degrees clockwise
    if o == 7:
        return torch.rot90(t, 2, (hdim, wdim)).transpose(hdim, wdim)
    return torch.rot90(t, 1, (hdim, wdim))        # 8: 90 degrees counter-clockwise


def test_torch_orient_is_the_model(torch):
    S = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    for o in range(1, 9):
        assert np.array_equal(torch_orient(torch, torch.from_numpy(S), o, 0, 1).numpy(), om.orient(S, o))


@pytest.mark.parametrize("layout", ["HWC", "CHW", "HW"])
def test_orient_to_tensor(zj, zt, ctx, torch, layout):
    g = torch.Generator().manual_seed(3)
    shapes = {"HWC": (70, 131, 3), "CHW": (3, 70, 131), "HW": (70, 131)}
    imgs = [torch.randint(0, 256, shapes[layout], dtype=torch.uint8, generator=g).cuda() for _ in range(8)]
    wide = torch.randint(0, 256, (70, 200, 3), dtype=torch.uint8, generator=g).cuda()
    if layout == "HWC":
        imgs[3] = wide[:, 5:136]  # (rows strided)
    outs = zt.orient_to_tensor(ctx, imgs, list(range(1, 9)), "CHW" if layout == "CHW" else "HWC")
    torch.cuda.synchronize()
    hd, wd = (1, 2) if layout == "CHW" else (0, 1)
    for o, (im, out) in enumerate(zip(imgs, outs), 1):
        assert out.is_contiguous() and torch.equal(out, torch_orient(torch, im, o, hd, wd)), (layout, o)


@pytest.mark.parametrize("antialias", [False, True])
def test_resize_to_tensor_with_orientations(zj, zt, ctx, torch, antialias):
    g = torch.Generator().manual_seed(4)
    imgs = [torch.randint(0, 256, (90 + o, 150, 3), dtype=torch.uint8, generator=g).cuda() for o in range(1, 9)]
    oris = list(range(1, 9))
    kw = dict(dtype=torch.float32, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], antialias=antialias)
    got = zt.resize_to_tensor(ctx, imgs, (48, 40), orientations=oris, **kw)
    exp = zt.resize_to_tensor(ctx, [torch_orient(torch, im, o, 0, 1).contiguous() for im, o in zip(imgs, oris)], (48, 40), **kw)
    torch.cuda.synchronize()
    assert torch.equal(got, exp)


@pytest.mark.parametrize("antialias", [False, True])
def test_decode_resized_crops_to_tensor_with_orientations(zj, zt, ctx, torch, synth, antialias):
    W, H = 250, 70
    planes, qts = synth.make_frame(W, H, 2, 2, 3, seed=9)
    d = zj.FrameDesc.make(W, H, 2, 2, 3, zj.ColorSpace.RGB, qts)
    fr = tuple(torch.from_numpy(np.ascontiguousarray(p, np.int16)).cuda() for p in planes)
    full = zt.decode_to_tensor(ctx, d, list(fr))[0]  # [H, W, 3], the stored image
    torch.cuda.synchronize()
    oris = list(range(1, 9))
    wins, crops = [], []
    for o in oris:
        D = torch_orient(torch, full, o, 0, 1)
        dh, dw = D.shape[:2]
        win = (dw // 5, dh // 7, dw - dw // 5 - (o % 3), dh - dh // 7 - (o % 2))
        wins.append(win)
        crops.append(D[win[1]:win[1] + win[3], win[0]:win[0] + win[2]].contiguous())
    kw = dict(dtype=torch.float32, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], antialias=antialias)
    got = zt.decode_resized_crops_to_tensor(ctx, d, [fr] * 8, wins, (32, 24), orientations=oris, flips=[o % 2 == 0 for o in oris], **kw)
    exp = zt.resize_to_tensor(ctx, crops, (32, 24), flips=[o % 2 == 0 for o in oris], **kw)
    torch.cuda.synchronize()
    assert torch.equal(got, exp)
