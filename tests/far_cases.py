"""The geometry of the far-offset tests (test_far_offsets_emu.py on the CPU, test_gpu_far_offsets.py on the GPU): images of a
few thousand pixels whose rows lie so far apart that the byte offsets the kernels form -- row x pitch, plane x pitch x height
-- pass 2^31 and 2^32.  The buffers are gigabytes of memory that is never touched; the work is the image's.  No GPU and
nothing of the library here.  TEST ONLY.

  pitches    two per limit: the limit itself, at which the low 32 bits of row x pitch are exactly 0 at row 256 (stages) or
             4096 (decode paths), and a smaller one that is no power of two, so that a line falls inside a row's span
  heights    the smallest at which the last row (HWC) or the last plane (CHW) starts past 2^32 bytes
  widths     one that is no multiple of 16 and one longer than a single lane run; 48 / 37 for the aligned / ragged decode kernels
"""
import mmap

import numpy as np

STAGE_PITCH_MAX = 1 << 24    # zj_stage_pack.h: stage_pitch
OUT_PITCH_MAX = 1 << 20      # zj_geom.h: OUT_PITCH_MAX
LINE31, LINE32 = 1 << 31, 1 << 32

STAGE_PITCHES = (STAGE_PITCH_MAX, STAGE_PITCH_MAX - 4099)   # (the second one odd)
STAGE_H_HWC, STAGE_H_CHW = 258, 130
STAGE_WIDTHS = (37, 130)
OUT_H_HWC, OUT_H_CHW = 4100, 2050
OUT_WIDTHS = (48, 37)


def out_pitches(w):
    """the two output pitches of a decode path for rows of w pixels: zj_plan.h wants a multiple of 16 where w is one; the
    smaller one still puts row 4099 past 2^32"""
    return (OUT_PITCH_MAX, OUT_PITCH_MAX - (272 if w % 16 == 0 else 259))


def last_row_offset(pitch, h, planes=1):
    """the largest row offset an image of `planes` planes of h rows makes a kernel form"""
    return (planes * h - 1) * pitch


def lines(pitch, h, planes=1):
    """the rows (counted through the planes) on each side of the 2^31 and the 2^32 line, the first and the last"""
    n = planes * h
    rows = {0, n - 1}
    for line in (LINE31, LINE32):
        r = line // pitch
        rows |= {k for k in (r - 1, r, r + 1) if 0 <= k < n}
    return sorted(rows)


def crosses(pitch, h, planes=1, line=LINE32):
    """the premise of a test: a row of the image starts at or past `line`"""
    return last_row_offset(pitch, h, planes) >= line


def zeros(n, dtype=np.uint8):
    """n zero bytes that the system commits 4 KB at a time as they are touched.  np.zeros asks for transparent huge pages
    (madvise), under which every touched row would commit 2 MB: a 4 GB buffer of rows 2^20 apart would be resident whole."""
    assert np.dtype(dtype) == np.uint8
    m = mmap.mmap(-1, max(int(n), 1), flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
    m.madvise(mmap.MADV_NOHUGEPAGE)
    return np.frombuffer(m, np.uint8)[:int(n)]


class Far:
    """`planes` planes of h rows of row_bytes bytes, `pitch` apart, in a zero buffer that the system commits page by page
    as it is touched: buf the flat bytes, rows the [planes, h, row_bytes] view of the image's own"""

    def __init__(self, planes, h, row_bytes, pitch):
        assert row_bytes <= pitch
        self.planes, self.h, self.row_bytes, self.pitch = planes, h, row_bytes, pitch
        self.buf = zeros(planes * h * pitch)
        self.rows = self.view(self.buf)

    def view(self, flat):
        return flat.reshape(self.planes, self.h, self.pitch)[:, :, :self.row_bytes]

    def fill(self, rng):
        self.rows[...] = rng.integers(0, 256, self.rows.shape, dtype=np.uint8)
        return self

    @property
    def image_bytes(self):
        return self.planes * self.h * self.row_bytes

    def once(self, amap):
        """a write (or read) map over buf: every byte of the image counted once, and nothing else in the whole buffer"""
        return int(self.view(amap).min()) == 1 == int(self.view(amap).max()) and int(np.count_nonzero(amap)) == self.image_bytes

    def far_rows(self):
        return lines(self.pitch, self.h, self.planes)
