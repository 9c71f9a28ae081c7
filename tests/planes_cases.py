"""The cases of the planes-to-RGB stage, shared by its CPU emulation test (test_planes_emu.py) and its GPU
test (test_gpu_sampling.py): the size / pitch / alignment matrix of tests/expand_cases.py, every case with a ratio pair and a
phase pair per component taken in turn from all 49 -- (rx, ry) in {1, 2, 4}^2 with every phase below them --, the layout of
a call's planes in one input buffer and its images in one output arena, and the stage in numpy.  TEST ONLY."""
import numpy as np

import expand_cases as ec
import oracle_np as onp

GUARD, SENTINEL = ec.GUARD, ec.SENTINEL
GEOS = [(rx, ry, px, py) for rx in (1, 2, 4) for ry in (1, 2, 4) for px in range(rx) for py in range(ry)]
assert len(GEOS) == 49


def with_geos(cases, phases=True, start=0):
    """(w, h, in_pad, out_pad, base, ((rx, ry, px, py) x 3)) of every case: component c of case k takes GEOS[(start + k) x
    (1, 3, 5)[c] + 11 c], so 49 consecutive cases (a width has 96) show every geometry to every component"""
    out = []
    for k, case in enumerate(cases):
        g = tuple(GEOS[((start + k) * m + 11 * c) % 49] for c, m in enumerate((1, 3, 5)))
        if not phases:
            g = tuple((rx, ry, 0, 0) for rx, ry, _, _ in g)
        out.append(tuple(case) + (g,))
    return out


def matrix(phases=True):
    return with_geos(ec.matrix(), phases)


def mixed_129(rng, phases=True):
    return with_geos(ec.mixed_129(rng), phases, start=int(rng.integers(0, 49)))


def plane_size(w, h, geo):
    """samples the image shows of a component: ceil((px + w) / rx) x ceil((py + h) / ry)"""
    rx, ry, px, py = geo
    return -(-(px + w) // rx), -(-(py + h) // ry)


def combine(planes, geos, w, h, stored_rgb):
    """u8 [h][w][3]: pixel (r, c) = colour(p_k[(py_k + r) // ry_k][(px_k + c) // rx_k])"""
    rep = []
    for p, (rx, ry, px, py) in zip(planes, geos):
        rep.append(p[np.ix_((py + np.arange(h)) // ry, (px + np.arange(w)) // rx)])
    if stored_rgb:
        return np.stack(rep, axis=-1)
    return onp.ycbcr_to_rgb_px(rep[0].astype(np.int16), rep[1].astype(np.int16), rep[2].astype(np.int16))


class Layout:
    """cases laid out in one input buffer and one output arena, both taken to start on a 16-byte boundary: per image and
    component the plane's offset and pitch, per image the output's offset and pitch; `src` the input bytes (random),
    `needed` the bytes of it that are samples an image shows (nothing else may be read), `want` the arena as the stage must
    leave it from an arena full of SENTINEL, `inside` the bytes of it that belong to an image"""

    def __init__(self, rng, cases, chw, stored_rgb):
        self.cases, self.chw = cases, chw
        bpp, npl = (1, 3) if chw else (3, 1)
        self.p_off, self.p_pitch, self.out_off, self.out_pitch, self.sizes, self.geos = [], [], [], [], [], []
        ia = oa = 0
        for w, h, in_pad, out_pad, base, geo in cases:
            offs, pits = [], []
            for c in range(3):
                pw, ph = plane_size(w, h, geo[c])
                ia = (ia + GUARD + 15) // 16 * 16 + (base + c) % 4 + 4 * (base % 2)
                offs.append(ia); pits.append(pw + in_pad)
                ia += (pw + in_pad) * (ph - 1) + pw
            op = w * bpp + out_pad
            oa = (oa + GUARD + 15) // 16 * 16 + base
            self.p_off.append(offs); self.p_pitch.append(pits); self.out_off.append(oa); self.out_pitch.append(op)
            self.sizes.append((w, h)); self.geos.append(geo)
            oa += op * h * npl + GUARD
        self.src = rng.integers(0, 256, ia + GUARD, dtype=np.uint8)
        self.needed = np.zeros(self.src.size, bool)
        self.arena_len = oa + 16
        self.want = np.full(self.arena_len, SENTINEL, np.uint8)
        self.inside = np.zeros(self.arena_len, bool)
        for (w, h, _, _, _, geo), offs, pits, oo, op in zip(cases, self.p_off, self.p_pitch, self.out_off, self.out_pitch):
            planes = []
            for c in range(3):
                pw, ph = plane_size(w, h, geo[c])
                idx = offs[c] + pits[c] * np.arange(ph)[:, None] + np.arange(pw)[None, :]
                self.needed[idx] = True
                planes.append(self.src[idx])
            e = combine(planes, geo, w, h, stored_rgb)
            rows = self.want[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp]
            mask = self.inside[oo:oo + op * h * npl].reshape(npl, h, op)[:, :, :w * bpp]
            rows[...] = e.transpose(2, 0, 1) if chw else e.reshape(1, h, 3 * w)
            mask[...] = True
