"""The size / pitch / alignment matrix of the colour-matrix stage, shared by its CPU emulation test
(test_color_emu.py) and its GPU test (test_gpu_color.py): the matrices, and the layout of a call's images in one input buffer
and one output arena with the arena as the stage must leave it (tests/color_model.py).  TEST ONLY."""
import itertools

import numpy as np

import color_model as cm

WIDTHS = tuple(range(1, 18)) + (31, 32, 33, 47, 48, 49)   # around the 16-pixel run and its multiples
HEIGHTS = (1, 2, 3)
PADS = (0, 1, 13)             # pitch: tight, + 1, + 13
BASES = tuple(range(16))      # an image's first byte past a 16-byte boundary
GUARD = 64                    # bytes either side of every output that nothing may write
SENTINEL = 0xA5


def jitter():
    """brightness 1.8, contrast 1.6 about 128, saturation 2, hue 0.2 turns: clamps at both ends.  Written out so that this
    file does not depend on the package: tensors.color_matrix(1.8, 1.6, 2.0, 0.2) (test_color_emu.py compares the two)."""
    luma = np.asarray(cm.LUMA)
    t = np.array([cm.LUMA, (0.595716, -0.274453, -0.321263), (0.211456, -0.522591, 0.311135)])
    a = 2 * np.pi * 0.2
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    hue = np.linalg.inv(t) @ rot @ t
    sat = 2.0 * np.eye(3) + (1.0 - 2.0) * np.tile(luma, (3, 1))
    lin = hue @ sat @ (1.6 * 1.8 * np.eye(3))
    off = hue @ sat @ np.full(3, (1.0 - 1.6) * 128.0)
    return np.concatenate([lin, off[:, None]], axis=1)


MATRICES = (cm.IDENTITY, cm.BGR, cm.GRAY, jitter(), cm.NEGATIVE)
# the ends of what the stage takes: +-16 / +-4096 in every entry, and mixed signs beside entries of one unit of 1/65536 -- the
# largest 24-bit products and sums color_mad (zj_color.h) forms
EXTREMES = (np.array([[16, 16, 16, 4096]] * 3, float), np.array([[-16, -16, -16, -4096]] * 3, float),
            np.array([[16, -16, 16, -4096], [-16, 16, -16, 4096], [1 / 65536, -1 / 65536, 0.5 / 65536, 0.5]], float))
EXTREME_WIDTHS = (1, 15, 16, 17, 33)


def matrix():
    """(w, h, in_pad, out_pad, in_base, out_base) of every case: every width, height, pad and base, the input at another
    pad and another offset from a 16-byte boundary than the output"""
    out = []
    for w, h, p, base in itertools.product(WIDTHS, HEIGHTS, range(len(PADS)), BASES):
        out.append((w, h, PADS[(p + 1) % len(PADS)], PADS[p], (5 * base + 3) % 16, base))
    return out


def mixed_49(rng):
    """49 images of different sizes: one more than a launch takes"""
    sizes = [(1, 1), (700, 1), (1, 300), (258, 3), (53, 37)]
    while len(sizes) < 49:
        sizes.append((int(rng.integers(1, 80)), int(rng.integers(1, 12))))
    return [(w, h, int(rng.choice(PADS)), int(rng.choice(PADS)), int(rng.integers(0, 16)), int(rng.integers(0, 16))) for w, h in sizes]


class Layout:
    """cases laid out in one input buffer `src` and one output arena, both taken to start on a 16-byte boundary.  Per image:
    in_off / in_pitch (in `src`; in place: in the arena, the output's own place and pitch), out_off / out_pitch, sizes, q
    (its 12 integers: MATRICES in turn, from `first`).  `arena0` is the arena before the call -- SENTINEL everywhere, in
    place: the images where the outputs will be --, `want` the arena as the stage must leave it, `inside` the bytes of it
    that belong to an image, `src_inside` the bytes of `src` that do (in place: `inside`)."""

    def __init__(self, rng, cases, chw, in_place, first=0, matrices=MATRICES):
        self.cases, self.chw, self.in_place = cases, chw, in_place
        bpp, npl = (1, 3) if chw else (3, 1)
        self.in_off, self.in_pitch, self.out_off, self.out_pitch, self.sizes, self.q, self.m = [], [], [], [], [], [], []
        ia = oa = 0
        for i, (w, h, in_pad, out_pad, in_base, out_base) in enumerate(cases):
            op = w * bpp + out_pad
            ip = op if in_place else w * bpp + in_pad
            oa = (oa + GUARD + 15) // 16 * 16 + out_base
            self.out_off.append(oa); self.out_pitch.append(op)
            oa += op * h * npl + GUARD
            if in_place:
                self.in_off.append(self.out_off[-1])
            else:
                ia = (ia + 15) // 16 * 16 + in_base
                self.in_off.append(ia)
                ia += ip * h * npl
            self.in_pitch.append(ip)
            self.sizes.append((w, h))
            m = matrices[(first + i) % len(matrices)]
            self.m.append(m)
            self.q.append(cm.fixed(m))
        self.arena_len = oa + 16
        self.arena0 = np.full(self.arena_len, SENTINEL, np.uint8)
        self.inside = np.zeros(self.arena_len, bool)
        self.src = self.arena0 if in_place else rng.integers(0, 256, ia + 16, dtype=np.uint8)
        self.src_inside = self.inside if in_place else np.zeros(self.src.size, bool)
        images = []
        for i, (w, h) in enumerate(self.sizes):
            ip, io, op, oo = self.in_pitch[i], self.in_off[i], self.out_pitch[i], self.out_off[i]
            if in_place:
                a = rng.integers(0, 256, (npl, h, w * bpp), dtype=np.uint8)
                self.arena0[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp] = a
            else:
                a = self.src[io:io + ip * h * npl].reshape(npl, h, ip)[:, :, :w * bpp].copy()
                self.src_inside[io:io + ip * h * npl].reshape(npl, h, ip)[:, :, :w * bpp] = True
            images.append(a)
            self.inside[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp] = True
        self.want = self.arena0.copy()
        for i, (w, h) in enumerate(self.sizes):
            op, oo, a = self.out_pitch[i], self.out_off[i], images[i]
            img = a if chw else a.reshape(h, w, 3)
            got = cm.apply_fixed(self.q[i], img, chw)
            self.want[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp] = got.reshape(npl, h, w * bpp)
