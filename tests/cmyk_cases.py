"""Four-component (Adobe CMYK / YCCK) JPEG files over given quantized coefficients, for the tests of ZJ_FLAG_CMYK_TO_RGB
(DESIGN.md 3.12): tools/jpeg_enc.py's bit writer, Huffman tables and progressive AC coder under a header writer of its own --
any component list (id, h, v, quantisation table), an optional Adobe APP14 segment -- and scans of up to four components,
baseline and progressive, with and without restart markers.  TEST ONLY.

Planes are given in MCU layout, per component [mcu_y * v][mcu_x * h][64] int16, natural order.  The decoder keeps component
4 in the layout of a one-component frame (k_plane_expected)."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import jpeg_enc as je  # noqa: E402

MODES = {"none": (1, 1), "h": (2, 1), "v": (1, 2), "hv": (2, 2)}
SIZES = ((16, 16), (33, 17), (48, 40), (100, 75))


def adobe_segment(transform, cut=False):
    """APP14: "Adobe", version 100, flags0, flags1, transform; cut: the segment ends in front of its flags"""
    payload = b"Adobe" + struct.pack(">HHHB", 100, 0, 0, transform)
    if cut:
        payload = payload[:8]
    return b"\xff\xee" + struct.pack(">H", len(payload) + 2) + payload


def components(hs, vs, ids=(1, 2, 3, 4), k_sampling=None):
    """(id, h, v, tq, huffman table) of a four-component frame: 1 and 4 at (hs, vs), 2 and 3 at (1, 1)"""
    kh, kv = k_sampling if k_sampling is not None else (hs, vs)
    return [(ids[0], hs, vs, 0, 0), (ids[1], 1, 1, 1, 1), (ids[2], 1, 1, 1, 1), (ids[3], kh, kv, 2, 0)]


def headers(w, h, comps, qts, progressive, restart=0, adobe=None, adobe_cut=False):
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xe0" + struct.pack(">H", 16) + b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    if adobe is not None:
        out += adobe_segment(adobe, adobe_cut)
    for t in sorted({c[3] for c in comps}):
        q = np.asarray(qts[min(t, len(qts) - 1)], np.int32).reshape(64)
        out += b"\xff\xdb" + struct.pack(">H", 67) + bytes([t]) + bytes(int(q[je.ZIGZAG[i]]) for i in range(64))
    out += (b"\xff\xc2" if progressive else b"\xff\xc0") + struct.pack(">HBHHB", 8 + 3 * len(comps), 8, h, w, len(comps))
    for cid, ch, cv, tq, _ in comps:
        out += bytes([cid, (ch << 4) | cv, tq])
    out += je._dht_segment()
    if restart:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart)
    return out


def sos(comps, which, ss, se, ah, al):
    seg = bytes([len(which)])
    for c in which:
        seg += bytes([comps[c][0], (comps[c][4] << 4) | comps[c][4]])
    seg += bytes([ss, se, (ah << 4) | al])
    return b"\xff\xda" + struct.pack(">H", len(seg) + 2) + seg


class Planes:
    def __init__(self, planes, w, h, comps):
        self.hmax, self.vmax = max(c[1] for c in comps), max(c[2] for c in comps)
        self.mcu_x, self.mcu_y = je._geometry(w, h, self.hmax, self.vmax)
        self.hv = [(c[1], c[2]) for c in comps]
        self.blocks = [np.asarray(p, np.int16).reshape(self.mcu_y * v, self.mcu_x * hh, 64).astype(np.int64)
                       for p, (hh, v) in zip(planes, self.hv)]
        self.w, self.h = w, h

    def mcu_blocks(self, which):
        for my in range(self.mcu_y):
            for mx in range(self.mcu_x):
                yield [(c, my * self.hv[c][1] + v, mx * self.hv[c][0] + hh) for c in which for v in range(self.hv[c][1])
                       for hh in range(self.hv[c][0])]

    def single_blocks(self, c):
        hs, vs = self.hv[c]
        cw, ch = -(-self.w * hs // self.hmax), -(-self.h * vs // self.vmax)
        for by in range(-(-ch // 8)):
            for bx in range(-(-cw // 8)):
                yield (c, by, bx)


def _put_dc(bw, diff):
    s = je._nbits(diff)
    bw.put(*je._dc_code(s))
    if s:
        bw.put(diff if diff >= 0 else diff + (1 << s) - 1, s)


def encode_baseline(planes, qts, w, h, hs, vs, restart=0, adobe=None, **kw):
    comps = components(hs, vs, **kw)
    P = Planes(planes, w, h, comps)
    out = headers(w, h, comps, qts, False, restart, adobe)
    out += sos(comps, [0, 1, 2, 3], 0, 63, 0, 0)
    bw = je.BitWriter()
    pred = [0] * 4
    for n, mcu in enumerate(P.mcu_blocks([0, 1, 2, 3])):
        if restart and n and n % restart == 0:
            je._emit_restart(bw, n // restart - 1)
            pred = [0] * 4
        for c, by, bx in mcu:
            blk = P.blocks[c][by, bx]
            _put_dc(bw, int(blk[0]) - pred[c])
            pred[c] = int(blk[0])
            run = 0
            for k in range(1, 64):
                v = int(blk[je.ZIGZAG[k]])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    bw.put(*je._ac_code(0xF0))
                    run -= 16
                s = je._nbits(v)
                bw.put(*je._ac_code((run << 4) | s))
                bw.put(v if v >= 0 else v + (1 << s) - 1, s)
                run = 0
            if run:
                bw.put(*je._ac_code(0))
    bw.flush()
    return bytes(out) + bytes(bw.out) + b"\xff\xd9"


def encode_progressive(planes, qts, w, h, hs, vs, restart=0, adobe=None, **kw):
    """DC of all four components (point transform 1), the AC bands of each component, then the refinement scans; restart:
    the interval in MCUs (interleaved scans) or blocks (scans of one component)"""
    comps = components(hs, vs, **kw)
    P = Planes(planes, w, h, comps)
    out = bytearray(headers(w, h, comps, qts, True, restart, adobe))
    allc = [0, 1, 2, 3]
    script = [(allc, 0, 0, 0, 1)] + [([c], 1, 5, 0, 2) for c in allc] + [([c], 6, 63, 0, 2) for c in allc]
    script += [([c], 1, 63, 2, 1) for c in allc] + [(allc, 0, 0, 1, 0)] + [([c], 1, 63, 1, 0) for c in allc]
    for which, ss, se, ah, al in script:
        out += sos(comps, which, ss, se, ah, al)
        bw = je.BitWriter()
        units = P.mcu_blocks(which) if len(which) > 1 else ([b] for b in P.single_blocks(which[0]))
        pred = [0] * 4
        enc = je._ProgAC(bw)
        for n, unit in enumerate(units):
            if restart and n and n % restart == 0:
                enc.flush_eobrun()
                je._emit_restart(bw, n // restart - 1)
                pred = [0] * 4
            for c, by, bx in unit:
                blk = P.blocks[c][by, bx]
                if ss == 0 and ah == 0:
                    t = int(blk[0]) >> al
                    _put_dc(bw, t - pred[c])
                    pred[c] = t
                elif ss == 0:
                    bw.put((int(blk[0]) >> al) & 1, 1)
                elif ah == 0:
                    enc.first(blk, ss, se, al)
                else:
                    enc.refine(blk, ss, se, al)
        enc.flush_eobrun()
        bw.flush()
        out += bw.out
    return bytes(out) + b"\xff\xd9"


def small_planes(w, h, hs, vs, seed=0, amp=40, dc=300):
    """Random sparse planes of a four-component frame in MCU layout.  The blocks outside the image keep a DC value (the
    interleaved scans code it) and no AC values (the scans of one component skip those blocks)."""
    rng = np.random.default_rng(seed)
    mcu_x, mcu_y = je._geometry(w, h, hs, vs)
    planes = []
    for ch, cv in ((hs, vs), (1, 1), (1, 1), (hs, vs)):
        bw, bh = mcu_x * ch, mcu_y * cv
        p = rng.integers(-amp, amp + 1, size=(bh, bw, 64))
        p[rng.random((bh, bw, 64)) < 0.75] = 0
        p[:, :, 0] = rng.integers(-dc, dc, size=(bh, bw))
        p[rng.random((bh, bw)) < 0.2, 1:] = 0
        cw, chh = -(-w * ch // hs), -(-h * cv // vs)
        p[-(-chh // 8):, :, 1:] = 0
        p[:, -(-cw // 8):, 1:] = 0
        planes.append(p.astype(np.int16).reshape(-1))
    return planes


def k_plane_expected(plane, w, h, hs, vs):
    """component 4 as the decoder keeps it: the blocks of a one-component frame, ceil(h / 8) x ceil(w / 8)"""
    mcu_x, mcu_y = je._geometry(w, h, hs, vs)
    return np.asarray(plane, np.int16).reshape(mcu_y * vs, mcu_x * hs, 64)[: -(-h // 8), : -(-w // 8)]


def bogus_frame(w, h, comps, qts):
    """headers up to and including a frame with any component list, an empty scan behind it: for the refusals"""
    return bytes(headers(w, h, comps, qts, False)) + sos(comps, list(range(min(len(comps), 4))), 0, 63, 0, 0) + b"\xff\xd9"


def file_tables(data):
    """the file's 8-bit quantisation tables by index, natural order, and the table index of each frame component"""
    zz = np.asarray(je.ZIGZAG)
    qt, tqs, at = {}, [], 2
    while at + 4 <= len(data) and data[at] == 0xFF and data[at + 1] != 0xDA:
        m, n = data[at + 1], (data[at + 2] << 8) | data[at + 3]
        seg = data[at + 4:at + 2 + n]
        if m == 0xDB:
            for o in range(0, len(seg), 65):
                q = np.zeros(64, np.int32)
                q[zz] = np.frombuffer(seg[o + 1:o + 65], np.uint8)
                qt[seg[o] & 15] = q
        if m in (0xC0, 0xC2):
            tqs = [seg[6 + 3 * c + 2] for c in range(seg[5])]
        at += 2 + n
    return qt, tqs
