"""Frames for the block-guard tests (test_guard_emu.py, test_gpu_guard.py): every arm of classify_block (zj_device.h) at its
limit -- DC-only blocks with the shortcut values 0, 255 and, planted, outside a byte (the tile redo); class-1 blocks whose
guard bound is GUARD_LIMIT or the largest value below it that the table admits, with pass-1 results at the end of an i16; and
class-2 blocks from one weight above the limit up to full-range noise -- side by side in every wave, under tables that move
the limit to different coefficient sizes, one set with a different table per component.  What the inputs reach is stated by
assert_cases() from numpy, emu_c.classify and oracle_np._pass alone: no kernel under test has a say in it.  The expected
bytes are the oracle's, each computed once and shared.  TEST ONLY."""
import functools
import importlib
import zlib

import numpy as np

import chroma_bytes_cases as cb
import emu_c
import oracle_c as oc
import oracle_np as onp
from test_packed_idct import scaled

MODES = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "440": (1, 2)}
TWC = {"420": 16, "422": 16, "444": 64, "440": 32}      # chroma block columns of a tile (zj_device.h: TileWidth, colour outputs)
YBR = {"420": 4, "422": 2, "444": 1, "440": 2}          # luma block rows of a strip (Cfg::YBR)
CBR = {"420": 2, "422": 2, "444": 1, "440": 1}          # chroma block rows of a strip (Cfg::CBR)
# 4:2:0 / 4:2:2: two full 256-pixel tiles and a narrow one, two strips, both halo seams; one full tile and a narrow one; the
# same with a ragged row end.  4:4:4 (512-pixel tiles, 8-row strips) and 4:4:0 (256-pixel tiles, 16-row strips): two tiles,
# two strips, and the ragged width of the same layout.
SHAPES = {"420": [(528, 64), (272, 48), (530, 64), (270, 48)], "422": [(528, 64), (272, 48), (530, 64), (270, 48)],
          "444": [(528, 16), (530, 16)], "440": [(272, 32), (270, 32)]}
KINDS = ["rgb", "ycbcr", "gray", "rgba", "chw", "plain"]
FLAG_PLAIN, FLAG_CLAMP_DC, FLAG_EDGE_REP = 1, 2, 4       # zj_frame_desc.flags == the oracle's extension bits
FLAG_SETS = [0, FLAG_CLAMP_DC, FLAG_EDGE_REP, FLAG_CLAMP_DC | FLAG_EDGE_REP]
PATTERN = (1, 2, 1, 0, 2, 1, 2, 1)                       # classes along a block row (shifted by 3 per row): 12.5 / 50 / 37.5 %
FLAT_EXACT = (1, 2, 3, 16)                               # the flat tables that divide the limit: dequantised 5904 itself


def limit():
    return emu_c.guard_limit()


@functools.lru_cache(maxsize=None)
def _table_sets():
    flat = lambda v: np.full(64, v, np.int32)
    zeroed = scaled(50).copy()
    zeroed[5:] = 0
    sets = {"q50": [scaled(50)] * 3, "q10": [scaled(10)] * 3, "q50z": [zeroed] * 3,
            "cross": [flat(1), flat(255), flat(16)]}
    for v in (1, 2, 3, 16, 255):
        sets[f"flat{v}"] = [flat(v)] * 3
    for s in sets.values():
        for q in s:
            q.setflags(write=False)
    return sets


TABLE_NAMES = ["q50", "q10", "flat1", "flat2", "flat3", "flat16", "flat255", "q50z", "cross"]


def tables(name):
    return _table_sets()[name]


@functools.lru_cache(maxsize=None)
def matrix_entries():
    """max |entry| of the butterfly's 8 x 8 matrix per INPUT row k (what a coefficient of row k is multiplied by at most)"""
    m = np.zeros((8, 8), np.int64)
    for k in range(8):
        e = [np.array([1 if i == k else 0], np.int32) for i in range(8)]
        m[:, k] = [int(v[0]) for v in onp._pass(e, np.int32(0))]
    return tuple(int(v) for v in np.abs(m).max(axis=0))


def weights(q):
    """the guard's weight of each of the 64 positions (build_table): the largest table entry of rows 0-3 (wt) or rows 4-7 (wb)
    of the position's column pair"""
    q = np.asarray(q, np.int64).reshape(8, 8)
    wt = q[:4].reshape(4, 4, 2).max(axis=(0, 2))
    wb = q[4:].reshape(4, 4, 2).max(axis=(0, 2))
    w = np.zeros((8, 8), np.int64)
    w[:4] = np.repeat(wt, 2)[None, :]
    w[4:] = np.repeat(wb, 2)[None, :]
    return w.reshape(64)


def bound(coeff, q):
    """the guard's own quantity per block: max over the four column pairs of sum |c| * weight"""
    a = np.abs(np.asarray(coeff).reshape(-1, 64).astype(np.int64)) * weights(q)[None, :]
    return a.reshape(-1, 8, 4, 2).sum(axis=(1, 3)).max(axis=1)


def classes(coeff, q):
    c = np.asarray(coeff).reshape(-1, 64)
    full = np.any(c[:, 1:] != 0, axis=1)
    return np.where(full, np.where(bound(c, q) <= limit(), 1, 2), 0).astype(np.int32)


def reach(coeff, q):
    """largest |pass-1 result >> 10| per block, from the reference's butterfly"""
    c = np.asarray(coeff, np.int16).reshape(-1, 64)
    with np.errstate(over="ignore"):
        deq = (c.astype(np.int32) * np.asarray(q, np.int32)[None, :]).reshape(-1, 8, 8)
        o = onp._pass([deq[:, k, :] for k in range(8)], 512)
        tmp = np.stack([v >> np.int32(10) for v in o], axis=1)
    return np.abs(tmp.astype(np.int64)).reshape(-1, 64).max(axis=1)


def attainable(q):
    """(the largest guard bound <= the limit, the largest |pass-1 result >> 10|) that ANY class-1 block of this table can have.
    A pair's bounds are the sums wt * a + wb * b: flat 255 stops at 23 * 255 = 5865, scaled(10) below the limit too.  A
    column's pass-1 result is linear in its coefficients under one budget, so its maximum sits on a single position."""
    lim, w, q = limit(), weights(q), np.asarray(q, np.int64)
    best = 0
    for jj in range(4):
        wt, wb = int(w[2 * jj]), int(w[32 + 2 * jj])
        if wt == 0 and wb == 0:
            continue
        for b in range(0, lim // wb + 1 if wb else 1):
            a = (lim - wb * b) // wt if wt else 0
            if a + b > 0:
                best = max(best, wt * a + wb * b)
    ent = matrix_entries()
    top = max((ent[p // 8] * (lim // int(w[p])) * int(q[p]) + 512) >> 10 for p in range(1, 64) if w[p] > 0)
    return best, top


# ---- block generators: lists of (block, tag) -------------------------------------------------------------------------------
def _dc(q, rng, cap=None):
    """a random DC inside the reference's range that leaves pair 0 most of its budget"""
    q0, w0 = int(q[0]), int(weights(q)[0])
    m = min(1016 // q0, (limit() // 4) // w0) if cap is None else cap
    return int(rng.integers(-m, m + 1))


def single(q, rng=None):
    """one non-zero AC coefficient at each position (of non-zero weight), just below, at and just above the limit"""
    rng = rng or np.random.default_rng(1)
    w, lim, out = weights(q), limit(), []
    for pos in range(1, 64):
        wgt = int(w[pos])
        if wgt == 0:
            continue
        dc = _dc(q, rng)
        budget = lim - (int(w[0]) * abs(dc) if (pos % 8) // 2 == 0 else 0)   # DC is a coefficient of pair 0
        cmax = budget // wgt
        for v in (cmax - 1, cmax, cmax + 1, -cmax, -(cmax + 1)):
            b = np.zeros(64, np.int16)
            b[0], b[pos] = dc, v
            out.append((b, "single"))
    return out


def _peak_row(q, j):
    """the row of column j where a whole budget gives the largest pass-1 result under this table"""
    w, ent, lim = weights(q), matrix_entries(), limit()
    rows = [k for k in range(1, 8) if w[8 * k + j] > 0]
    return max(rows, key=lambda k: ent[k] * (lim // int(w[8 * k + j])) * int(q[8 * k + j])) if rows else None


def worst_columns(q):
    """a column pair's whole budget on row 1 (matrix entry 5683) of each column, both signs; the same on the row that
    reaches furthest under this table; and the budget spread over the column with alternating signs"""
    w, lim, out = weights(q), limit(), []
    for j in range(8):
        wt, wb = int(w[j]), int(w[32 + j])
        for k in sorted({1, _peak_row(q, j) or 1}):
            wgt = int(w[8 * k + j])
            if wgt == 0:
                continue
            for sgn in (1, -1):
                b = np.zeros(64, np.int16)
                b[8 * k + j] = sgn * (lim // wgt)
                out.append((b, "worst"))
        cs = lim // (4 * (wt + wb)) if wt + wb else 0
        if cs:
            for sgn in (1, -1):
                b = np.zeros(64, np.int16)
                for k in range(8):
                    b[8 * k + j] = sgn * cs * (1 if k % 2 else -1)
                out.append((b, "worst"))
    return out


def dense(q, rng):
    """all four column pairs at the limit at once, each budget on row 1 or on the table's furthest-reaching row of one of the
    pair's columns: a pass-2 row sees four inputs near +32 766, four near -32 766, or alternating ones"""
    w, lim, out = weights(q), limit(), []
    signs = [(1, 1, 1, 1), (-1, -1, -1, -1), (1, -1, 1, -1), (-1, 1, -1, 1)]
    signs += [tuple(int(v) for v in rng.choice([-1, 1], 4)) for _ in range(2)]
    for cols in ((0, 2, 4, 6), (1, 3, 5, 7), (0, 3, 4, 7), (1, 2, 5, 6)):
        for sg in signs:
            for peak in (False, True):
                b = np.zeros(64, np.int16)
                for j, s in zip(cols, sg):
                    k = (_peak_row(q, j) or 1) if peak else 1
                    wgt = int(w[8 * k + j])
                    if wgt:
                        b[8 * k + j] = s * (lim // wgt)
                if b.any():
                    out.append((b, "dense"))
    return out


def near(q, rng, n):
    """random blocks whose bound lands within two weights of the limit: a pair's budget over 1..16 of its sixteen positions"""
    w, lim, out = weights(q), limit(), []
    pairs = [jj for jj in range(4) if w[2 * jj] or w[32 + 2 * jj]]
    for i in range(n):
        jj = pairs[i % len(pairs)]
        pos = [8 * k + 2 * jj + h for k in range(8) for h in (0, 1)]
        pos = [p for p in pos if p != 0 and w[p] > 0]
        wp = int(max(w[p] for p in pos))
        b = np.zeros(64, np.int16)
        if jj != 0:
            b[0] = _dc(q, rng, cap=min(1016 // int(q[0]), 500 // int(w[0])))
        target = lim + int(rng.integers(-wp, 2 * wp + 1))
        chosen = [pos[t] for t in rng.permutation(len(pos))[:int(rng.integers(1, len(pos) + 1))]]
        left = target
        for t, p in enumerate(chosen):
            share = left if t == len(chosen) - 1 else int(rng.integers(0, left + 1))
            c = share // int(w[p])
            b[p] = c * (1 if rng.integers(2) else -1)
            left -= c * int(w[p])
        if b[1:].any():
            out.append((b, "near"))
    return out


def limit_blocks(q):
    """per column pair: the block whose bound is the largest the pair's two weights can form below or at the limit (the limit
    itself wherever they divide it), on rows 1 and 5 of the pair's first column; and the one a top-row step above it"""
    w, lim, out = weights(q), limit(), []
    for jj in range(4):
        wt, wb = int(w[2 * jj]), int(w[32 + 2 * jj])
        best = None
        for nb in range(0, lim // wb + 1 if wb else 1):
            na = (lim - wb * nb) // wt if wt else 0
            if na + nb > 0 and (best is None or wt * na + wb * nb > best[0]):
                best = (wt * na + wb * nb, na, nb)
        if best is None:
            continue
        for extra in (0, 1):
            b = np.zeros(64, np.int16)
            b[8 + 2 * jj], b[40 + 2 * jj] = best[1], -best[2]
            if extra:
                b[(8 if wt else 40) + 2 * jj + 1] = 1
            out.append((b, "limit"))
    return out


@functools.lru_cache(maxsize=None)
def dc_for(side, q0):
    """(dc, shortcut value): the DC of a DC-only block whose shortcut value (chroma_bytes_cases.shortcut_value: an i16 wrapping
    product) is the closest to a byte's end that this quantiser can form -- "hi" / "lo" from outside (256 and -1 where it
    can), "top" / "bottom" from inside (255 and 0 where it can: a quantiser of 80 has 16-fold products and stops at 254)"""
    dc = np.arange(-32768, 32768, dtype=np.int64)
    prod = (dc * q0) & 0xFFFF
    val = (np.where(prod >= 0x8000, prod - 0x10000, prod) >> 3) + 128
    want = {"hi": lambda: val[val > 255].min(), "lo": lambda: val[val < 0].max(),
            "top": lambda: val[val <= 255].max(), "bottom": lambda: val[val >= 0].min()}[side]()
    idx = np.nonzero(val == want)[0]
    i = idx[np.argmin(np.abs(dc[idx]))]
    return int(dc[i]), int(val[i])


def dc_only(q, rng):
    q0 = int(q[0])
    out = []
    for v in ("bottom", "top"):
        b = np.zeros(64, np.int16)
        b[0] = dc_for(v, q0)[0]
        assert cb.shortcut_value(b[0], q0) == dc_for(v, q0)[1]
        out.append((b, "dc"))
    for _ in range(5):
        b = np.zeros(64, np.int16)
        b[0] = int(rng.integers(-(1024 // q0), 1016 // q0 + 1))
        out.append((b, "dc"))
    out.append((np.zeros(64, np.int16), "zero"))
    return out


def full_range(rng, n=8):
    return [(rng.integers(-32768, 32768, 64).astype(np.int16), "full") for _ in range(n)]


class Pool:
    """every generator's blocks under one table: blocks, their class and bound, and per class the indices in an order that
    takes the generators in turn"""

    def __init__(self, q):
        rng = np.random.default_rng(zlib.crc32(np.asarray(q, np.int32).tobytes()))
        items = single(q, rng) + worst_columns(q) + dense(q, rng) + near(q, rng, 96) + limit_blocks(q) + dc_only(q, rng) + full_range(rng)
        self.q = np.asarray(q, np.int32)
        self.blocks = np.array([b for b, _ in items], np.int16)
        self.tags = np.array([t for _, t in items])
        self.cls = classes(self.blocks, q)
        self.bound = bound(self.blocks, q)
        self.by = []
        for c in range(3):
            groups = [list(np.nonzero((self.cls == c) & (self.tags == t))[0]) for t in dict.fromkeys(self.tags)]
            groups = [g for g in groups if g]
            self.by.append([g[i] for i in range(max(len(g) for g in groups)) for g in groups if i < len(g)])


@functools.lru_cache(maxsize=None)
def _pool(qkey):
    return Pool(np.array(qkey, np.int32))


def pool(q):
    return _pool(tuple(int(v) for v in q))


# ---- frames ---------------------------------------------------------------------------------------------------------------
def plants(mode, w, h):
    """(component, block row, block column, "hi" | "lo") of the DC-only blocks whose shortcut value is no byte.  The
    horizontally sub-sampled modes take the chroma blocks of chroma_bytes_cases.plants -- an ordinary block of a tile, and a
    block a tile sees through its halo column only -- except 4:2:0 at 48 rows: its one strip has two tiles, each the other's
    halo neighbour, so there a luma block of the narrow tile is planted and the full tile stays with the packed code.
    4:4:4 / 4:4:0 have no byte chroma and no halo: luma blocks of tile 0, strip 0."""
    hs, vs = MODES[mode]
    if hs == 1:
        return [(0, 0, 5, "lo"), (0, 0, 9, "hi")]
    if mode == "420" and h < 64:
        return [(0, 1, 2 * ((w + 15) // 16) - 1, "hi")]
    return [(c, r, col, "hi" if v > 255 else "lo") for (c, r, col, v) in cb.plants(w, h, hs, vs)]


def strips(mode, h):
    """strips a launch covers: two MCU rows each where the chroma is sub-sampled horizontally (an odd last one is dropped)"""
    hs, vs = MODES[mode]
    mcu_y = (h + 8 * vs - 1) // (8 * vs)
    return mcu_y // 2 if hs == 2 else mcu_y


def redo_tiles(mode, w, h):
    """{(strip, tile)} the planted blocks send to the wide code under an RGB-family output without ZJ_FLAG_CLAMP_DC: the tile
    of a planted luma block; the tile of a planted chroma block and the tiles that have it as their halo column (byte chroma:
    the horizontally sub-sampled modes)"""
    hs, vs = MODES[mode]
    cbw = (w + 8 * hs - 1) // (8 * hs)
    twc = TWC[mode]
    ntiles = (cbw + twc - 1) // twc
    out = set()
    for (comp, brow, col, _) in plants(mode, w, h):
        if comp == 0:
            out.add((brow // YBR[mode], col // (twc * hs)))
            continue
        strip = brow // CBR[mode]
        for t in range(ntiles):
            cb0 = t * twc
            nvalid = min(twc, cbw - cb0)
            left = cb0 - 1 if cb0 > 0 else cbw - 1
            right = cb0 + nvalid if cb0 + nvalid < cbw else 0
            if cb0 <= col < cb0 + nvalid or col in (left, right):
                out.add((strip, t))
    return {(s, t) for (s, t) in out if s < strips(mode, h)}


def all_tiles(mode, w, h):
    hs, _ = MODES[mode]
    cbw = (w + 8 * hs - 1) // (8 * hs)
    return {(s, t) for s in range(strips(mode, h)) for t in range((cbw + TWC[mode] - 1) // TWC[mode])}


def tile_rect(mode, w, h, strip, tile):
    """(x, y, width, height) of a tile's pixels inside the frame"""
    hs, _ = MODES[mode]
    tw, sh = TWC[mode] * hs * 8, YBR[mode] * 8
    x, y = tile * tw, strip * sh
    return x, y, min(tw, w - x), min(sh, h - y)


@functools.lru_cache(maxsize=None)
def _frame(name, mode, w, h, seed):
    synth = importlib.import_module("zune-jpeg_amd.synth")
    hs, vs = MODES[mode]
    qts = tables(name)
    planes, tags = [], []
    for c in range(3):
        br, bc = synth.plane_blocks(w, h, hs, vs, c)
        p = pool(qts[c])
        cur = [0, 37 * seed + 11 * c, 37 * seed + 11 * c]   # (the few DC-only blocks start with the ends of the byte range)
        plane = np.zeros((br * bc, 64), np.int16)
        tag = np.empty(br * bc, dtype=object)
        for r in range(br):
            for col in range(bc):
                k = PATTERN[(col + 3 * r) % len(PATTERN)]
                i = p.by[k][cur[k] % len(p.by[k])]
                cur[k] += 1
                plane[r * bc + col] = p.blocks[i]
                tag[r * bc + col] = p.tags[i]
        planes.append(plane)
        tags.append(tag)
    for (comp, brow, col, side) in plants(mode, w, h):
        bc = synth.plane_blocks(w, h, hs, vs, comp)[1]
        planes[comp][brow * bc + col] = 0
        planes[comp][brow * bc + col, 0] = dc_for(side, int(qts[comp][0]))[0]
        tags[comp][brow * bc + col] = "plant"
    planes = [p.reshape(-1) for p in planes]
    for p in planes:
        p.setflags(write=False)
    return planes, qts, tags


def frame(name, mode, w, h, seed=0):
    """(planes, qts) of a frame under the table set `name`; the planes are read-only and shared"""
    return _frame(name, mode, w, h, seed)[:2]


def block_tags(name, mode, w, h, seed=0):
    """per component the generator ("single", "worst", "dense", "near", "limit", "dc", "zero", "full", "plant") of every block"""
    return _frame(name, mode, w, h, seed)[2]


def luma_blocks(name, mode, w, h, tag, redone, seed=0):
    """(block row, block column) of the class-1 luma blocks of generator `tag` that lie inside the frame, in a launched strip,
    in a tile that is / is not redone"""
    synth = importlib.import_module("zune-jpeg_amd.synth")
    hs, vs = MODES[mode]
    planes, qts, tags = _frame(name, mode, w, h, seed)
    br, bc = synth.plane_blocks(w, h, hs, vs, 0)
    cls = classes(planes[0], qts[0])
    redo = redo_tiles(mode, w, h)
    out = []
    for r in range(min(br, strips(mode, h) * YBR[mode])):
        for col in range(bc):
            if tags[0][r * bc + col] == tag and cls[r * bc + col] == 1 and 8 * col < w and 8 * r < h \
                    and ((r // YBR[mode], col // (TWC[mode] * hs)) in redo) == redone:
                out.append((r, col))
    return out


def windows(name, mode, w, h):
    """crop windows (x, y, w, h): the whole frame; inside a redone tile; inside a tile that is not; across the seam between two
    such tiles; one pixel of a `worst_columns` block that the packed code decodes"""
    redo = redo_tiles(mode, w, h)
    keep = all_tiles(mode, w, h) - redo
    seam = [(s, t) for (s, t) in sorted(redo) if (s, t + 1) in keep or (s, t - 1) in keep]
    assert redo and keep and seam, (mode, w, h, redo, keep)
    s, t = seam[0]
    n = (s, t + 1) if (s, t + 1) in keep else (s, t - 1)
    rx, ry, rw, rh = tile_rect(mode, w, h, s, t)
    nx, ny, nw, nh = tile_rect(mode, w, h, *n)
    edge = max(rx, nx)                                     # the column where the two tiles meet
    lo, hi = max(edge - 21, 0), min(edge + 19, w)
    r, col = luma_blocks(name, mode, w, h, "worst", False)[0]
    inside = lambda x, y, ww, hh: (x + min(3, ww - 1), y + min(1, hh - 1), max(1, min(ww - 3, 37)), max(1, min(hh - 1, 11)))
    return [(0, 0, w, h), inside(rx, ry, rw, rh), inside(nx, ny, nw, nh), (lo, ry + 2, hi - lo, min(rh - 2, 9)),
            (min(8 * col + 3, w - 1), min(8 * r + 5, h - 1), 1, 1)]


def kind_of(kind):
    """(the oracle's colour space, the oracle's extension bits, zj_frame_desc.flags bits, out_layout) of an output kind"""
    cs = {"rgb": oc.RGB, "ycbcr": oc.YCBCR, "gray": oc.GRAYSCALE, "rgba": oc.RGBA, "chw": oc.RGB, "plain": oc.RGB}[kind]
    return cs, (oc.EXT_PLAIN if kind in ("rgba", "chw", "plain") else 0), (FLAG_PLAIN if kind == "plain" else 0), int(kind == "chw")


@functools.lru_cache(maxsize=None)
def expected(name, mode, w, h, kind="rgb", flags=0, seed=0):
    """the oracle's bytes: rows (h, row bytes), or (3, h, w) for `chw`"""
    hs, vs = MODES[mode]
    planes, qts = frame(name, mode, w, h, seed)
    cs, ext, _, _ = kind_of(kind)
    rc, exp = oc.decode_planes(oc.make_frame(w, h, hs, vs, 3, cs, qts), planes, ext=flags | ext)
    assert rc == 0, (name, mode, w, h, kind, flags, rc)
    exp = np.ascontiguousarray(exp.reshape(h, w, 3).transpose(2, 0, 1)) if kind == "chw" else exp.reshape(h, -1)
    exp.setflags(write=False)
    return exp


def crop_of(exp, kind, x, y, w, h):
    """a window of expected(): (h, w * bytes per pixel), or (3, h, w) for `chw`"""
    if kind == "chw":
        return exp[:, y:y + h, x:x + w]
    bpp = {"gray": 1, "rgba": 4}.get(kind, 3)
    return exp[y:y + h, x * bpp:(x + w) * bpp]


def predicted_stats(name, mode, w, h, seed=0):
    """(DC-only, class-1, class-2 blocks, tiles redone) of one fused RGB launch: the classes of the blocks of the launched
    strips (the halo columns have a wave of their own and are not classified), and redo_tiles()"""
    synth = importlib.import_module("zune-jpeg_amd.synth")
    hs, vs = MODES[mode]
    planes, qts = frame(name, mode, w, h, seed)
    n = [0, 0, 0]
    for c in range(3):
        bc = synth.plane_blocks(w, h, hs, vs, c)[1]
        rows = strips(mode, h) * (YBR[mode] if c == 0 else CBR[mode])
        cls = classes(planes[c].reshape(-1, 64)[:rows * bc], qts[c])
        for k in range(3):
            n[k] += int((cls == k).sum())
    return n[0], n[1], n[2], len(redo_tiles(mode, w, h))


# ---- what the inputs reach ------------------------------------------------------------------------------------------------
_REPORT = None


def assert_cases(verbose=True):
    """Conditions on the INPUTS, from numpy, emu_c.classify and oracle_np._pass.  Returns (and prints) per table the class-1
    bound reached, the smallest class-2 bound and the largest |pass-1 result >> 10| among class-1 blocks, and per frame shape
    the class mix."""
    global _REPORT
    if _REPORT is not None:
        return _REPORT
    lim = limit()
    report = {"tables": {}, "mix": {}}
    seen = {}
    for name in TABLE_NAMES:
        for q in tables(name):
            key = tuple(int(v) for v in q)
            if key in seen:
                continue
            p = pool(q)
            assert np.array_equal(p.cls, emu_c.classify(p.blocks, q)), (name, "classify_block disagrees with the bound in numpy")
            assert np.array_equal(p.cls == 0, ~np.any(p.blocks[:, 1:] != 0, axis=1))
            best, top = attainable(q)
            one, two = p.cls == 1, p.cls == 2
            wmin = int(weights(q)[weights(q) > 0].min())
            got1, got2, far = int(p.bound[one].max()), int(p.bound[two].min()), int(reach(p.blocks[one], q).max())
            flat = len(set(key)) == 1
            # a class-1 block AT the limit -- for the tables whose pair weights cannot sum to 5904 (flat 255, scaled(10)) at the
            # largest bound they can form -- and a class-2 block within one weight above the limit
            assert got1 == best and (best == lim or not (flat and key[0] in FLAT_EXACT)), (name, got1, best)
            assert lim < got2 <= lim + wmin, (name, got2, wmin)
            # pass-1 results at the end of an i16: 5683 * 5904 + 512 >> 10 = 32 766 where the table divides the limit; 32 000
            # for every table that can reach it at all (one whose only non-zero entries are in row 0 stops at 4096 * 5904 >> 10)
            floor = 32700 if flat and key[0] in FLAT_EXACT else (32000 if top >= 32000 else top)
            assert far >= floor and far <= 32767, (name, far, floor, top)
            seen[key] = dict(table=name, class1_bound=got1, limit_attainable=best, class2_bound=got2, reach=far, reach_attainable=top,
                             blocks=(int((p.cls == 0).sum()), int(one.sum()), int(two.sum())))
    report["tables"] = {v["table"]: v for v in seen.values()}
    for name in TABLE_NAMES:
        for mode, shapes in SHAPES.items():
            for (w, h) in shapes:
                for seed in (0, 1):
                    planes, qts = frame(name, mode, w, h, seed)
                    tags = block_tags(name, mode, w, h, seed)
                    mix = []
                    for c in range(3):
                        cls = classes(planes[c], qts[c])
                        frac = [float((cls == k).mean()) for k in range(3)]
                        assert min(frac) >= 0.10, (name, mode, w, h, c, frac)
                        mix.append(frac)
                    report["mix"][(name, mode, w, h, seed)] = mix
                    for (comp, brow, col, side) in plants(mode, w, h):      # planted as described: DC-only, no byte
                        hs, vs = MODES[mode]
                        bc = (w + 8 * hs - 1) // (8 * hs) * (hs if comp == 0 else 1)
                        blk = planes[comp].reshape(-1, 64)[brow * bc + col]
                        v = cb.shortcut_value(blk[0], qts[comp][0])
                        assert not blk[1:].any() and not 0 <= v <= 255 and tags[comp][brow * bc + col] == "plant", (name, mode, comp, v)
                    for comp in range(3):                                     # the in-range ends of the shortcut
                        b = planes[comp].reshape(-1, 64)
                        vals = {cb.shortcut_value(v, qts[comp][0]) for v in b[~b[:, 1:].any(axis=1), 0]}
                        ends = {dc_for("bottom", int(qts[comp][0]))[1], dc_for("top", int(qts[comp][0]))[1]}
                        assert ends <= vals and min(ends) == 0 and max(ends) >= 254, (name, mode, w, h, comp, ends)
                    redo, keep = redo_tiles(mode, w, h), all_tiles(mode, w, h) - redo_tiles(mode, w, h)
                    assert redo and keep, (mode, w, h, redo)
                    if seed == 0:   # a tile the packed code keeps holds worst-column and dense blocks
                        assert luma_blocks(name, mode, w, h, "worst", False) and luma_blocks(name, mode, w, h, "dense", False), (name, mode, w, h)
                        assert len(windows(name, mode, w, h)) == 5
    # redo_tiles() for the shapes whose sets are easy to state by hand
    assert redo_tiles("420", 528, 64) == {(0, 0), (1, 0), (1, 1)} and redo_tiles("420", 272, 48) == {(0, 1)}
    assert redo_tiles("422", 272, 48) == {(0, 0), (1, 0), (1, 1)} and redo_tiles("444", 528, 16) == {(0, 0)}
    assert redo_tiles("440", 270, 32) == {(0, 0)}
    # the cross-component set: the same coefficients change class under another component's table
    qs = tables("cross")
    planes, _ = frame("cross", "420", 528, 64)
    for c in range(3):
        own = classes(planes[c], qs[c])
        for o in range(3):
            if o == c:
                continue
            other = classes(planes[c], qs[o])
            if qs[c][0] < qs[o][0]:
                assert ((own == 1) & (other == 2)).sum() >= 8, (c, o)
            else:
                assert ((own == 2) & (other == 1)).sum() >= 8, (c, o)
    if verbose:
        print(f"guard cases: GUARD_LIMIT {lim}")
        for k, v in report["tables"].items():
            print(f"  table {k:9s} class-1 bound {v['class1_bound']} (attainable {v['limit_attainable']}), smallest class-2 bound "
                  f"{v['class2_bound']}, reach {v['reach']} (attainable {v['reach_attainable']}), pool 0/1/2 {v['blocks']}")
        allmix = np.array([m for v in report["mix"].values() for m in v])
        print(f"  class mix over {len(report['mix'])} frames x 3 components: DC-only {allmix[:, 0].min():.3f}..{allmix[:, 0].max():.3f}, "
              f"packed {allmix[:, 1].min():.3f}..{allmix[:, 1].max():.3f}, wide {allmix[:, 2].min():.3f}..{allmix[:, 2].max():.3f}")
    _REPORT = report
    return report
