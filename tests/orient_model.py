"""The numpy definition of EXIF orientation: the two tables of the issue -- which stored pixel a displayed
one is, and which stored window a displayed window is -- and an EXIF reader, written without looking at the C++.
TEST ONLY."""
import struct

import numpy as np


def oriented_size(o, w, h):
    """(w, h) of the displayed image of a stored w x h one"""
    if not 1 <= o <= 8:
        raise ValueError(o)
    return (h, w) if o >= 5 else (w, h)


def orient(S, o):
    """S: [H, W] or [H, W, C] -> the displayed image D, built index by index from the table (D[r][c] = ...)"""
    H, W = S.shape[:2]
    dw, dh = oriented_size(o, W, H)
    r, c = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")
    sr, sc = {1: (r, c), 2: (r, W - 1 - c), 3: (H - 1 - r, W - 1 - c), 4: (H - 1 - r, c),
              5: (c, r), 6: (H - 1 - c, r), 7: (H - 1 - c, W - 1 - r), 8: (c, W - 1 - r)}[o]
    return np.ascontiguousarray(S[sr, sc])


def orient_chw(S, o):
    """[3, H, W]: every plane on its own"""
    return np.stack([orient(p, o) for p in S])


def stored_window(o, W, H, win):
    """the window (x, y, w, h) of D as a window of S (a stored frame of W x H); None: not a window of D"""
    x, y, w, h = win
    dw, dh = oriented_size(o, W, H)
    if w <= 0 or h <= 0 or x < 0 or y < 0 or x + w > dw or y + h > dh:
        return None
    return {1: (x, y, w, h), 2: (W - x - w, y, w, h), 3: (W - x - w, H - y - h, w, h), 4: (x, H - y - h, w, h),
            5: (y, x, h, w), 6: (y, H - x - w, h, w), 7: (W - y - h, H - x - w, h, w), 8: (W - y - h, x, h, w)}[o]


def exif_orientation(jpeg):
    """Orientation of a JPEG file's first Exif APP1 segment in front of SOS, 1 when there is nothing usable"""
    b = bytes(jpeg)
    if b[:2] != b"\xff\xd8":
        return 1
    p = 2
    while p + 4 <= len(b):
        if b[p] != 0xFF:
            p += 1
            continue
        m = b[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xDA:
            break
        ln = struct.unpack(">H", b[p + 2:p + 4])[0]
        if ln < 2:
            break
        seg = b[p + 4:p + 2 + ln]  # (cut by the buffer's end where the length lies)
        if m == 0xE1 and seg[:6] == b"Exif\0\0":
            return _tiff_orientation(seg[6:])
        p += 2 + ln
    return 1


def _tiff_orientation(t):
    try:
        e = {b"II*\0": "<", b"MM\0*": ">"}[t[:4]]
        ifd = struct.unpack(e + "I", t[4:8])[0]
        n = struct.unpack(e + "H", t[ifd:ifd + 2])[0]
        for i in range(n):
            ent = t[ifd + 2 + 12 * i:ifd + 14 + 12 * i]
            tag, typ, cnt = struct.unpack(e + "HHI", ent[:8])
            if tag == 0x0112:
                v = struct.unpack(e + "H", ent[8:10])[0]
                return v if typ == 3 and cnt == 1 and 1 <= v <= 8 else 1
    except (KeyError, struct.error):
        pass
    return 1


def exif_segment(value, order="<", before=(), after=(), ifd_offset=8, typ=3, count=1):
    """an APP1 Exif segment (marker included): IFD0 at ifd_offset with the entries `before` (tag, type, count, 4 value
    bytes), then Orientation = value (value None: no such entry), then `after`"""
    ents = list(before)
    if value is not None:
        ents.append((0x0112, typ, count, struct.pack(order + "HH", value, 0)))
    ents += list(after)
    tiff = {"<": b"II*\0", ">": b"MM\0*"}[order] + struct.pack(order + "I", ifd_offset) + b"\0" * (ifd_offset - 8)
    tiff += struct.pack(order + "H", len(ents))
    for tag, ty, cn, val in ents:
        tiff += struct.pack(order + "HHI", tag, ty, cn) + val
    tiff += struct.pack(order + "I", 0)
    payload = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def splice(jpeg, *segments):
    """the segments behind SOI"""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + b"".join(segments) + jpeg[2:]
