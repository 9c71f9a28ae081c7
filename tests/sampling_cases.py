"""Three-component JPEG files of ANY sampling over given quantized coefficients, for the tests of ZJ_FLAG_ANY_SAMPLING
(DESIGN.md 3.13): the header writer, scan headers and MCU walk of tests/cmyk_cases.py (they take any component list) under
tools/jpeg_enc.py's bit writer and tables -- any three (h, v) pairs, any ids, with or without an Adobe APP14 segment, baseline
and progressive, with and without restart markers.  TEST ONLY.

Planes are given in MCU layout, per component [mcu_y * v][mcu_x * h][64] int16, natural order.  The decoder keeps every
component of a non-standard file in the layout of a one-component frame of the component's own size (plane_expected).

Also here: the MODEL of such a file's image in numpy -- clamped IDCT per component, box replication, the
full decode's colour arithmetic -- and smooth-plus-noise content for the comparisons with Pillow."""
import numpy as np

import cmyk_cases as cc
import oracle_np as onp

je = cc.je

# the non-standard samplings under test: 4:1:1, 4:1:0, 1x4, chroma that is not (1,1), luma below the maximum
SAMPLINGS = (((4, 1), (1, 1), (1, 1)), ((4, 2), (1, 1), (1, 1)), ((1, 4), (1, 1), (1, 1)), ((2, 2), (2, 1), (2, 1)),
             ((2, 2), (1, 2), (1, 2)), ((2, 1), (1, 1), (2, 1)), ((1, 1), (2, 2), (2, 2)))
SIZES = ((16, 16), (33, 17), (48, 40), (100, 75))
STANDARD = (((1, 1), (1, 1), (1, 1)), ((2, 1), (1, 1), (1, 1)), ((1, 2), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1)))


def name(samp):
    return "".join("%d%d" % hv for hv in samp)


def components(samp, ids=(1, 2, 3)):
    """(id, h, v, tq, huffman table) of a three-component frame"""
    return [(ids[i], samp[i][0], samp[i][1], min(i, 1), min(i, 1)) for i in range(3)]


def maxima(samp):
    return max(hv[0] for hv in samp), max(hv[1] for hv in samp)


def ratios(samp):
    hm, vm = maxima(samp)
    return tuple((hm // h, vm // v) for h, v in samp)


def comp_size(w, h, samp, i):
    """samples of component i: ceil(W h_i / h_max) x ceil(H v_i / v_max)"""
    hm, vm = maxima(samp)
    return -(-w * samp[i][0] // hm), -(-h * samp[i][1] // vm)


def mcu_blocks(w, h, samp, i):
    """blocks of component i's plane in MCU layout: (rows, columns)"""
    hm, vm = maxima(samp)
    mcu_x, mcu_y = je._geometry(w, h, hm, vm)
    return mcu_y * samp[i][1], mcu_x * samp[i][0]


def _ac_baseline(bw, blk):
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


def encode(planes, qts, w, h, samp, progressive=False, restart=0, adobe=None, ids=(1, 2, 3), jfif=True):
    """the file: baseline -- one interleaved scan; progressive -- DC of all components (point transform 1), two AC bands and
    a refinement per component, the DC refinement, the last AC refinement (14 scans).  restart: the interval in MCUs
    (interleaved scans) or blocks (scans of one component).  Every component uses Huffman table min(index, 1).  jfif=False
    leaves the JFIF APP0 segment out, as libjpeg does when it writes RGB samples (with the segment libjpeg, and so Pillow,
    reads the samples as YCbCr whatever an Adobe segment says)."""
    comps = components(samp, ids)
    P = cc.Planes(planes, w, h, comps)
    out = bytearray(cc.headers(w, h, comps, qts, progressive, restart, adobe))
    if not jfif:
        assert out[2:4] == b"\xff\xe0" and out[4:6] == b"\x00\x10"
        del out[2:20]
    allc = [0, 1, 2]
    if not progressive:
        script = [(allc, 0, 63, 0, 0)]
    else:
        script = [(allc, 0, 0, 0, 1)] + [([c], 1, 5, 0, 2) for c in allc] + [([c], 6, 63, 0, 2) for c in allc]
        script += [([c], 1, 63, 2, 1) for c in allc] + [(allc, 0, 0, 1, 0)] + [([c], 1, 63, 1, 0) for c in allc]
    for which, ss, se, ah, al in script:
        out += cc.sos(comps, which, ss, se, ah, al)
        bw = je.BitWriter()
        units = P.mcu_blocks(which) if len(which) > 1 else ([b] for b in P.single_blocks(which[0]))
        pred = [0] * 3
        enc = je._ProgAC(bw)
        for n, unit in enumerate(units):
            if restart and n and n % restart == 0:
                enc.flush_eobrun()
                je._emit_restart(bw, n // restart - 1)
                pred = [0] * 3
            for c, by, bx in unit:
                blk = P.blocks[c][by, bx]
                if not progressive:
                    cc._put_dc(bw, int(blk[0]) - pred[c])
                    pred[c] = int(blk[0])
                    _ac_baseline(bw, blk)
                elif ss == 0 and ah == 0:
                    t = int(blk[0]) >> al
                    cc._put_dc(bw, t - pred[c])
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


def small_planes(w, h, samp, seed=0, amp=40, dc=300):
    """Random sparse planes in MCU layout.  The blocks outside a component's own size keep a DC value (the interleaved
    scans code it) and no AC values (the scans of one component skip those blocks)."""
    rng = np.random.default_rng(seed)
    planes = []
    for i in range(3):
        bh, bw = mcu_blocks(w, h, samp, i)
        p = rng.integers(-amp, amp + 1, size=(bh, bw, 64))
        p[rng.random((bh, bw, 64)) < 0.75] = 0
        p[:, :, 0] = rng.integers(-dc, dc, size=(bh, bw))
        p[rng.random((bh, bw)) < 0.2, 1:] = 0
        cw, ch = comp_size(w, h, samp, i)
        p[-(-ch // 8):, :, 1:] = 0
        p[:, -(-cw // 8):, 1:] = 0
        planes.append(p.astype(np.int16).reshape(-1))
    return planes


def plane_expected(plane, w, h, samp, i):
    """component i as the decoder keeps it for a non-standard file: ceil(ch / 8) x ceil(cw / 8) blocks"""
    bh, bw = mcu_blocks(w, h, samp, i)
    cw, ch = comp_size(w, h, samp, i)
    return np.asarray(plane, np.int16).reshape(bh, bw, 64)[: -(-ch // 8), : -(-cw // 8)]


# ---- the model ---------------------------------------------------------------------------------------
def samples(blocks, qt):
    """S: the clamped 8-point IDCT of a plane [bh][bw][64] with its table, the DC-only shortcut clamped too: u8 [8 bh][8 bw]"""
    bh, bw = blocks.shape[:2]
    px = np.clip(onp.idct_blocks(blocks.reshape(-1, 64), qt), 0, 255).astype(np.uint8)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


def combine(S, rat, x, y, w, h, stored_rgb=False):
    """E over the stored window: E[r][c] = colour(S_0[(y + r) // ry_0][(x + c) // rx_0], ...), u8 [h][w][3]"""
    rows, cols = np.arange(y, y + h), np.arange(x, x + w)
    rep = [S[i][np.ix_(rows // rat[i][1], cols // rat[i][0])] for i in range(3)]
    if stored_rgb:
        return np.stack(rep, axis=-1)
    return onp.ycbcr_to_rgb_px(rep[0].astype(np.int16), rep[1].astype(np.int16), rep[2].astype(np.int16))


def model_image(planes_kept, qts3, samp, x, y, w, h, stored_rgb=False):
    """planes_kept: the three planes as the decoder keeps them ([bh][bw][64]); qts3: each component's table"""
    S = [samples(np.asarray(planes_kept[i]), qts3[i]) for i in range(3)]
    return combine(S, ratios(samp), x, y, w, h, stored_rgb)


# ---- smooth-plus-noise content ----------------------------------------------------------------------------------------
_K = np.arange(8)
_DCT = np.cos((2 * _K[None, :] + 1) * _K[:, None] * np.pi / 16) * np.where(_K[:, None] == 0, np.sqrt(0.125), 0.5)


def content(w, h, seed=0):
    """three full-resolution float planes 0..255: smooth gradients and waves plus a little noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for c in range(3):
        a, b, ph = rng.uniform(0.02, 0.12, 2).tolist() + [rng.uniform(0, 6.28)]
        p = 128 + (60 - 15 * c) * np.sin(a * xx + ph) * np.cos(b * yy) + (xx - w / 2) * 0.3 * (1 - c) + rng.normal(0, 3, (h, w))
        out.append(np.clip(p, 0, 255))
    return out


def quantised_planes(img, w, h, samp, qts3):
    """MCU-layout planes of the content: each component box-averaged to its own resolution, edge-replicated to the MCU
    grid, forward DCT, divided by its table and rounded"""
    planes = []
    for i in range(3):
        rx, ry = ratios(samp)[i]
        cw, ch = comp_size(w, h, samp, i)
        p = np.pad(img[i], ((0, ch * ry - h), (0, cw * rx - w)), mode="edge").reshape(ch, ry, cw, rx).mean(axis=(1, 3))
        bh, bw = mcu_blocks(w, h, samp, i)
        p = np.pad(p, ((0, 8 * bh - ch), (0, 8 * bw - cw)), mode="edge") - 128.0
        blk = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        coef = np.einsum("ky,abyx,lx->abkl", _DCT, blk, _DCT)
        q = np.asarray(qts3[i], np.float64).reshape(8, 8)
        planes.append(np.rint(coef / q).astype(np.int16).reshape(-1))
    return planes


def flat_tables(a=4, b=6):
    return [np.full(64, a, np.int32), np.full(64, b, np.int32)]
