"""CPU: the orientation kernel's phases (zune-jpeg_amd/csrc/zj_orient.h) run thread by thread (tests/emu_orient) against the
numpy definition (tests/orient_model.py): every orientation, channel count and layout, sizes around the tile side, tight and
padded pitches on both sides, destinations at all four byte alignments -- and a write map that shows every byte of every
destination row written exactly once and nothing else written at all."""
import itertools

import numpy as np
import pytest

import emu_orient_c as eo
import orient_model as om

POISON = 0xA5


def sides():
    T = eo.tile()
    return [1, 2, 3, 5, T - 1, T, T + 1, 2 * T + 3]


def stored_image(rng, w, h, channels, chw, pitch):
    """(buffer with 8 bytes of margin on both sides, the view the kernel is given, the image as [H, W(, C)] / [3, H, W])"""
    bpp, npl = (1, 3) if chw else (channels, 1)
    buf = rng.integers(0, 256, 16 + pitch * h * npl, dtype=np.uint8)
    body = buf[8:8 + pitch * h * npl]
    rows = body.reshape(npl, h, pitch)[:, :, :w * bpp]
    img = rows.reshape(3, h, w) if chw else (rows.reshape(h, w, channels) if channels == 3 else rows.reshape(h, w))
    return buf, body, np.ascontiguousarray(img)


def run_case(rng, cases, channels, chw):
    """cases: (w, h, o, in_pad, out_pad, align) -- one launch over all of them, checked against the model"""
    bpp, npl = (1, 3) if chw else (channels, 1)
    ins, keep, sizes, ipit, opit, offs, exps, oris = [], [], [], [], [], [], [], []
    at = 64
    for w, h, o, in_pad, out_pad, align in cases:
        dw, dh = om.oriented_size(o, w, h)
        ip, op = w * bpp + in_pad, dw * bpp + out_pad
        buf, body, img = stored_image(rng, w, h, channels, chw, ip)
        keep.append(buf)
        ins.append(body); sizes.append((w, h)); ipit.append(ip); opit.append(op); oris.append(o)
        at = (at + 3) // 4 * 4 + align
        offs.append(at)
        exps.append(om.orient_chw(img, o) if chw else om.orient(img, o))
        at += op * dh * npl + 32
    arena = np.full(at + 64, POISON, np.uint8)
    wmap, outside = eo.orient(ins, sizes, ipit, channels, chw, oris, arena, offs, opit)
    assert outside == 0, "a store fell outside the arena"
    want = np.zeros(arena.size, np.uint8)
    for (w, h, o, _, _, _), off, op, exp in zip(cases, offs, opit, exps):
        dw, dh = om.oriented_size(o, w, h)
        rows = arena[off:off + op * dh * npl].reshape(npl, dh, op)
        assert np.array_equal(rows[:, :, :dw * bpp].reshape(exp.shape), exp), (w, h, o, channels, chw)
        want[off:off + op * dh * npl].reshape(npl, dh, op)[:, :, :dw * bpp] = 1
    assert np.array_equal(wmap, want), "a byte of a destination row not written exactly once, or a byte outside the rows written"
    assert (arena[want == 0] == POISON).all()


@pytest.mark.parametrize("channels,chw", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("o", range(1, 9))
def test_every_size_around_the_tile(o, channels, chw):
    rng = np.random.default_rng(100 * o + channels + chw)
    S = sides()
    cases = []
    for i, (w, h) in enumerate(itertools.product(S, S)):
        # pitches: tight / padded on each side by turns (7: rows start at every alignment), destinations at all alignments
        cases.append((w, h, o, (0, 7, 0, 13)[i % 4], (0, 0, 5, 9)[(i // 4) % 4], i % 4))
    B = eo.batch()
    for k in range(0, len(cases), B):
        run_case(rng, cases[k:k + B], channels, chw)


@pytest.mark.parametrize("channels,chw", [(1, False), (3, False), (3, True)])
def test_every_alignment_of_source_and_destination(channels, chw):
    """one size just over the tile, every orientation, the four alignments of the destination times tight / odd pitches"""
    rng = np.random.default_rng(7 + channels)
    T = eo.tile()
    cases = [(T + 1, T - 1, o, in_pad, out_pad, align) for o in range(1, 9) for align in range(4)
             for in_pad, out_pad in ((0, 0), (1, 3), (2, 2), (3, 1))]
    run_case(rng, cases, channels, chw)


def test_a_mixed_launch_and_the_kernel_arguments():
    """images of every orientation and very different sizes in one launch: the grid is the largest image's, the workgroups
    beyond a smaller one do nothing; the launch's arguments stay under 4 KB and LDS is what DESIGN.md says"""
    rng = np.random.default_rng(11)
    T = eo.tile()
    cases = [(1, 1, 1, 0, 0, 1), (1, 67, 6, 0, 0, 3), (67, 1, 5, 3, 0, 2), (T - 1, T + 1, 8, 0, 1, 1), (T + 1, T - 1, 7, 5, 0, 0),
             (130, 3, 3, 0, 0, 3), (3, 130, 2, 0, 2, 1), (2 * T + 3, 5, 4, 1, 1, 2)]
    for channels, chw in ((1, False), (3, False), (3, True)):
        run_case(rng, cases, channels, chw)
    assert eo.batch() == 128 and T == 64
    assert eo.lib().zjeo_lds_bytes(3) == 12544 and eo.lib().zjeo_lds_bytes(1) == 4416
