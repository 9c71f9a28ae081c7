"""The images of the tone stage's tests (test_tone_emu.py on the CPU, test_gpu_tone.py on the GPU): sizes around the
16-pixel run, and an arena that places each image at its own pitch and offset between guard bytes.  TEST ONLY."""
import numpy as np

WIDTHS, HEIGHTS = (1, 15, 16, 17, 37, 130), (1, 3)


class Arena:
    """images of their own sizes in one host buffer, each at its own pitch and at an offset 0..3 from a dword, the padding
    and the gaps full of `fill`: what a call reads, or what it writes"""

    def __init__(self, sizes, channels, chw, rng, fill, lo=0, hi=256, pads=(0, 1, 13, 3), data=True):
        self.channels, self.chw = channels, chw
        self.bpp, self.npl = (1, channels) if chw or channels == 1 else (channels, 1)
        self.sizes, self.off, self.pitch, self.img = list(sizes), [], [], []
        at = 64
        for i, (w, h) in enumerate(self.sizes):
            pitch = w * self.bpp + pads[i % len(pads)]
            at = (at + 15) // 16 * 16 + i % 4
            self.off.append(at)
            self.pitch.append(pitch)
            at += pitch * h * self.npl + 32
        self.buf = np.full(at + 64, fill, np.uint8)
        self.inside = np.zeros(self.buf.size, bool)
        for i, (w, h) in enumerate(self.sizes):
            a = rng.integers(lo, hi, (self.npl, h, w * self.bpp), dtype=np.uint8) if data else None
            self.img.append(a)
            v = self.view(self.buf, i)
            self.view(self.inside, i)[...] = True
            if data:
                v[...] = a

    def view(self, flat, i):
        w, h = self.sizes[i]
        return flat[self.off[i]:self.off[i] + self.pitch[i] * h * self.npl].reshape(self.npl, h, self.pitch[i])[:, :, :w * self.bpp]

    def image(self, i, flat=None):
        """image i as the model takes it: [h, w], [h, w, 3] or (chw) [3, h, w]"""
        a = self.img[i] if flat is None else self.view(flat, i)
        w, h = self.sizes[i]
        if self.channels == 1:
            return a.reshape(h, w)
        return a.reshape(3, h, w) if self.chw else a.reshape(h, w, 3)

    def put(self, flat, i, img):
        self.view(flat, i)[...] = np.asarray(img).reshape(self.npl, self.sizes[i][1], -1)


def permutations(rng, n, channels):
    """a random permutation table per image and channel: every entry is hit, and no two images share a table"""
    return np.stack([np.stack([rng.permutation(256).astype(np.uint8) for _ in range(channels)]) for _ in range(n)])


def stretches(rng, ar, values=(0, 7, 199)):
    """the arena's images refilled with stretches of equal neighbours along each row -- 1 to 40 pixels of one value per
    channel, so stretches end inside, at and across the 16-pixel runs -- for the histogram's one add per stretch"""
    for i, (w, h) in enumerate(ar.sizes):
        planes = []
        for _ in range(ar.channels * h):
            row = np.concatenate([np.full(int(rng.integers(1, 41)), rng.choice(values), np.uint8) for _ in range(w)])[:w]
            planes.append(row)
        a = np.stack(planes).reshape(ar.channels, h, w)                     # [c, h, w]
        img = a if ar.chw or ar.channels == 1 else a.transpose(1, 2, 0)     # HWC: [h, w, c]
        ar.img[i] = np.ascontiguousarray(img).reshape(ar.npl, h, w * ar.bpp)
        ar.view(ar.buf, i)[...] = ar.img[i]
    return ar
