"""The size / pitch / alignment matrix of the gray-to-RGB stage, shared by its CPU emulation test
(test_expand_emu.py) and its GPU test (test_gpu_gray_rgb.py), and the layout of a call's images in one input buffer and one
output arena.  TEST ONLY."""
import itertools

import numpy as np

WIDTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 49, 130)
HEIGHTS = (1, 2, 3, 9)
IN_PADS = (0, 5)            # input pitch: tight, w + 5
OUT_PADS = (0, 1, 3, 16)    # output pitch: tight, padded
BASES = (0, 1, 3)           # an image's first byte past a 16-byte boundary
GUARD = 64                  # bytes either side of every output that nothing may write
SENTINEL = 0xA5


def matrix():
    """(w, h, in_pad, out_pad, base) of every case"""
    return list(itertools.product(WIDTHS, HEIGHTS, IN_PADS, OUT_PADS, BASES))


def mixed_129(rng):
    """129 images of mixed sizes: two launches of one call"""
    return [(int(rng.choice(WIDTHS)), int(rng.choice(HEIGHTS)), int(rng.choice(IN_PADS)), int(rng.choice(OUT_PADS)),
             int(rng.choice(BASES))) for _ in range(129)]


class Layout:
    """cases laid out in one input buffer and one output arena, both taken to start on a 16-byte boundary: per image its
    input offset, input pitch, output offset, output pitch; `src` the input bytes (random), `want` the arena as the stage must
    leave it from an arena full of SENTINEL, `inside` the bytes of it that belong to an image"""

    def __init__(self, rng, cases, chw):
        self.cases, self.chw = cases, chw
        bpp, npl = (1, 3) if chw else (3, 1)
        self.in_off, self.in_pitch, self.out_off, self.out_pitch, self.sizes = [], [], [], [], []
        ia = oa = 0
        for w, h, in_pad, out_pad, base in cases:
            ip, op = w + in_pad, w * bpp + out_pad
            ia = (ia + 15) // 16 * 16 + base
            oa = (oa + GUARD + 15) // 16 * 16 + base
            self.in_off.append(ia); self.in_pitch.append(ip); self.out_off.append(oa); self.out_pitch.append(op)
            self.sizes.append((w, h))
            ia += ip * h
            oa += op * h * npl + GUARD
        self.src = rng.integers(0, 256, ia + 16, dtype=np.uint8)
        self.arena_len = oa + 16
        self.want = np.full(self.arena_len, SENTINEL, np.uint8)
        self.inside = np.zeros(self.arena_len, bool)
        for (w, h, _, _, _), io, ip, oo, op in zip(cases, self.in_off, self.in_pitch, self.out_off, self.out_pitch):
            g = self.src[io:io + ip * h].reshape(h, ip)[:, :w]
            rows = self.want[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp]
            mask = self.inside[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp]
            rows[...] = np.broadcast_to(g, (3, h, w)) if chw else np.repeat(g, 3, axis=1)[None]
            mask[...] = True
