"""Frames for the interior-tile tests (test_interior_emu.py, test_gpu_interior.py): the smallest shapes at which the interior
form of the colour rounds (Cfg::INTERIOR, interior_tile in zune-jpeg_amd/csrc/zj_device.h) can go wrong, the oracle's bytes for
every output kind -- each computed once and shared -- and the predicate stated on its own.  TEST ONLY."""
import functools

import numpy as np

import oracle_c as oc

MODES = {"h": (2, 1), "hv": (2, 2)}
KINDS = ["rgb", "ycbcr", "rgba", "plain"]
FLAG_PLAIN, FLAG_EDGE_REP = 1, 4          # zj_frame_desc.flags == the oracle's extension bits
TILE_PX = 256                             # pixels of a tile row in both modes (16 chroma block columns)
THREADS = {"hv": 256, "h": 192}           # threads of a workgroup: 12 * 16 + 8 and 8 * 16 + 8 blocks, one lane each, whole waves
CHROMA_Q0 = 8                             # DC quantiser of the chroma tables: shortcut value == dc + 128

# (name, mode, width, height, flags, padded rows, planted block)
#   768 x 64: three tiles, two whole strips -- tile 1 is interior;  512 x 64: a first and a last tile, no interior one;
#   768 x 48: the second strip is cut short -- three MCU rows, and the reference drops an odd last one (mcu.rs:145-156), so
#   the strip is never launched;  768 x 56: four MCU rows, the second strip is launched with 24 of its 32 rows inside the
#   frame, and its tile 1 must take the general rounds;  752 x 64: a narrow last tile (15 groups), tile 1 still interior;
#   1024 x 32 with replicated edges: no tile may take the interior rounds (and without the flag tiles 1 and 2 do);
#   padded rows; a DC-only Cb block with the shortcut value 256 in tile 1 of strip 0 (chroma block column 20: no other
#   tile's halo column), so that the tile the predicate admits is redone by the wide code;  4:2:2: its rounds are not full.
CASES = [
    ("768x64", "hv", 768, 64, 0, False, None),
    ("512x64", "hv", 512, 64, 0, False, None),
    ("768x48", "hv", 768, 48, 0, False, None),
    ("768x56", "hv", 768, 56, 0, False, None),
    ("752x64", "hv", 752, 64, 0, False, None),
    ("1024x32-edge-rep", "hv", 1024, 32, FLAG_EDGE_REP, False, None),
    ("1024x32", "hv", 1024, 32, 0, False, None),
    ("768x64-padded", "hv", 768, 64, 0, True, None),
    ("768x64-redo", "hv", 768, 64, 0, False, (1, 0, 20, 256)),
    ("768x32-422", "h", 768, 32, 0, False, None),
]
CASE_IDS = [c[0] for c in CASES]


def out_pitch(width, kind):
    """Padded rows: 2432 bytes for the three-byte outputs of a 768-pixel row (2304 bytes); an RGBA row is 3072 bytes, so
    its padded pitch is the next multiple of 128 after it"""
    return 3200 if kind == "rgba" else 2432


def geometry(w, h, mode):
    """(tiles per row, strips launched, rows per strip) of a frame: a strip is two MCU rows, an odd last MCU row is dropped"""
    hs, vs = MODES[mode]
    mcu_x = (w + 8 * hs - 1) // (8 * hs)
    mcu_y = (h + 8 * vs - 1) // (8 * vs)
    return (mcu_x * 8 * hs + TILE_PX - 1) // TILE_PX, mcu_y // 2, 16 * vs


def interior(w, h, mode, flags, strip, tile):
    """The predicate, stated without the kernel's variables: a tile takes the interior rounds when it has a tile on either
    side in its row, all rows of its strip are inside the frame, the launch does not replicate the chroma edges, and the
    tile's items (one per 16 pixels of each row) fill every round of the workgroup's threads."""
    tiles, _, sh = geometry(w, h, mode)
    items = sh * (TILE_PX // 16)
    return items % THREADS[mode] == 0 and 0 < tile < tiles - 1 and (strip + 1) * sh <= h and not flags & FLAG_EDGE_REP


@functools.lru_cache(maxsize=None)
def frame(w, h, mode, plant=None, seed=0):
    """(planes, qts): dense low-quality blocks and in-range DC-only chroma; plant = (component, chroma block row, column,
    shortcut value) makes that block DC-only with that value.  The planes are read-only and shared."""
    import importlib
    synth = importlib.import_module("zune-jpeg_amd.synth")
    hs, vs = MODES[mode]
    rng = np.random.default_rng(20261020 + 7 * w + 3 * h + 2 * hs + vs + 1000 * seed)
    qts = [q.copy() for q in synth.quant_tables(10)]
    qts[1][0] = qts[2][0] = CHROMA_Q0
    keep = 0.6 * np.exp(-np.arange(64) / 10.0)
    planes = []
    for c in range(3):
        br, bc = synth.plane_blocks(w, h, hs, vs, c)
        n = br * bc
        zz = rng.integers(-3, 4, size=(n, 64)) * (rng.random((n, 64)) < keep[None, :])
        zz[:, 0] = rng.integers(-12, 13, size=n) if c == 0 else rng.integers(-128, 128, size=n)
        zz[rng.random(n) < (0.4 if c else 0.3), 1:] = 0
        nat = np.zeros((n, 64), np.int16)
        nat[:, synth.UN_ZIGZAG] = zz.astype(np.int16)
        planes.append(nat)
    if plant is not None:
        comp, brow, col, value = plant
        bc = synth.plane_blocks(w, h, hs, vs, comp)[1]
        blk = planes[comp][brow * bc + col]
        blk[:] = 0
        blk[0] = value - 128                                           # q0 = 8: (dc * 8) >> 3 == dc
    planes = [p.reshape(-1) for p in planes]
    for p in planes:
        p.setflags(write=False)
    return planes, qts


def colorspace(kind):
    return {"rgb": oc.RGB, "ycbcr": oc.YCBCR, "rgba": oc.RGBA, "plain": oc.RGB}[kind]


def desc_flags(kind, flags):
    return flags | (FLAG_PLAIN if kind == "plain" else 0)


@functools.lru_cache(maxsize=None)
def expected(w, h, mode, kind, flags, plant=None, seed=0):
    """The oracle's bytes as rows (h, width x components): the reference's own placement for RGB / YCbCr, its
    plain-placement restatement for `plain` and RGBA"""
    hs, vs = MODES[mode]
    planes, qts = frame(w, h, mode, plant, seed)
    ext = flags | (oc.EXT_PLAIN if kind in ("rgba", "plain") else 0)
    rc, exp = oc.decode_planes(oc.make_frame(w, h, hs, vs, 3, colorspace(kind), qts), planes, ext=ext)
    assert rc == 0, (w, h, mode, kind, flags, rc)
    exp = exp.reshape(h, -1)
    exp.setflags(write=False)
    return exp


def redo_tiles(w, h, mode, plant):
    """{(strip, tile)} the planted block sends to the wide code: the tile that holds it (the cases plant away from the halo)"""
    if plant is None:
        return set()
    _, brow, col, _ = plant
    return {(brow // 2, col // 16)}
