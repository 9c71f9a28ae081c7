"""The size / pitch / alignment matrix of the CMYK-to-RGB stage, shared by its CPU emulation test
(test_cmyk_emu.py) and its GPU test (test_gpu_cmyk.py), the layout of a call's images in one input buffer and one output arena,
and the stage's definition in numpy.  TEST ONLY."""
import numpy as np

from expand_cases import BASES, GUARD, HEIGHTS, IN_PADS, OUT_PADS, SENTINEL, WIDTHS, matrix  # noqa: F401  (the same matrix)


def combine(a, k, inverted):
    """the definition: (a * k + 127) // 255 per channel, a [..., 3] or [3, ...] broadcast against k; not inverted: both
    complemented first"""
    a, k = a.astype(np.int32), k.astype(np.int32)
    if not inverted:
        a, k = 255 - a, 255 - k
    return ((a * k + 127) // 255).astype(np.uint8)


def mixed_129(rng):
    """129 images of mixed sizes: more than one launch of one call"""
    return [(int(rng.choice(WIDTHS)), int(rng.choice(HEIGHTS)), int(rng.choice(IN_PADS)), int(rng.choice(OUT_PADS)),
             int(rng.choice(BASES))) for _ in range(129)]


class Layout:
    """cases (w, h, in_pad, out_pad, base) laid out in one input buffer and one output arena, both taken to start on a 16-byte
    boundary.  Per image: k_off / k_pitch (in `src`), a_off / a_pitch (in `src`; in place: the output's own place in the
    arena), out_off / out_pitch (in the arena), inverted.  `arena0` is the arena before the call -- SENTINEL everywhere, in
    place: the images a where the outputs will be --, `want` the arena as the stage must leave it, `inside` the bytes of it
    that belong to an image."""

    def __init__(self, rng, cases, chw, in_place):
        self.cases, self.chw, self.in_place = cases, chw, in_place
        bpp, npl = (1, 3) if chw else (3, 1)
        self.k_off, self.k_pitch, self.a_off, self.a_pitch, self.out_off, self.out_pitch = [], [], [], [], [], []
        self.sizes, self.inverted = [], []
        ia = oa = 0
        for i, (w, h, in_pad, out_pad, base) in enumerate(cases):
            kp, op = w + in_pad, w * bpp + out_pad
            ap = op if in_place else w * bpp + in_pad
            ia = (ia + 15) // 16 * 16 + base
            self.k_off.append(ia); self.k_pitch.append(kp)
            ia += kp * h
            oa = (oa + GUARD + 15) // 16 * 16 + base
            self.out_off.append(oa); self.out_pitch.append(op)
            oa += op * h * npl + GUARD
            if in_place:
                self.a_off.append(self.out_off[-1])
            else:
                ia = (ia + 15) // 16 * 16 + (3 - base)   # (a at another offset from a 16-byte boundary than k and the output)
                self.a_off.append(ia)
                ia += ap * h * npl
            self.a_pitch.append(ap)
            self.sizes.append((w, h))
            self.inverted.append(int(rng.integers(0, 2)) if len(cases) > 2 else i & 1)
        self.src = rng.integers(0, 256, ia + 16, dtype=np.uint8)
        self.arena_len = oa + 16
        self.arena0 = np.full(self.arena_len, SENTINEL, np.uint8)
        self.want = self.arena0.copy()
        self.inside = np.zeros(self.arena_len, bool)
        for i, (w, h, _, _, _) in enumerate(cases):
            kp, ap, op, oo = self.k_pitch[i], self.a_pitch[i], self.out_pitch[i], self.out_off[i]
            k = self.src[self.k_off[i]:self.k_off[i] + kp * h].reshape(h, kp)[:, :w]
            if in_place:
                a = rng.integers(0, 256, (npl, h, w * bpp), dtype=np.uint8)
                self.arena0[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp] = a
            else:
                a = self.src[self.a_off[i]:self.a_off[i] + ap * h * npl].reshape(npl, h, ap)[:, :, :w * bpp]
            kk = np.broadcast_to(k, (3, h, w)) if chw else np.repeat(k, 3, axis=1)[None]
            self.want[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp] = combine(a, kk, self.inverted[i])
            self.inside[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp] = True
