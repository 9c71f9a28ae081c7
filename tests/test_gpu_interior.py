"""GPU: the interior form of the fused kernel's colour rounds (Cfg::INTERIOR, interior_tile in zune-jpeg_amd/csrc/zj_device.h)
through zj_decode_planes_device -- batches of two frames at the shapes of tests/interior_cases.py, byte for byte against the
oracle, padded rows included -- and through one scattered launch (zj_decode_frames_device) of two 768 x 64 frames."""
import ctypes as C
import importlib

import numpy as np
import pytest

import interior_cases as cases

pytestmark = pytest.mark.gpu
FILL = 0xAA


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def ctx(zj):
    c = zj.Context(zj.BACKEND_HIP, 0)  # no GPU -> raises; nothing falls back to the CPU
    yield c
    c.close()


def _upload(zj, ctx, arrays, out_bytes):
    bufs = [ctx.device_alloc(a.nbytes) for a in arrays] + [ctx.device_alloc(out_bytes)]
    for a, b in zip(arrays, bufs):
        ctx.h2d(b, a)
    zj.lib().zj_device_memset(ctx.handle, bufs[-1], FILL, out_bytes)
    return bufs


def _check_rows(got, exp, what):
    """got: (height, pitch) from the device; exp: the oracle's rows.  The padding of every row keeps the fill."""
    row = exp.shape[1]
    bad = np.argwhere(got[:, :row] != exp)
    assert bad.size == 0, (what, len(bad), bad[:8].tolist())
    assert (got[:, row:] == FILL).all(), (what, "the padding of a row was written")


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_batches_of_two_on_the_device_match_oracle(zj, ctx, case, kind):
    name, mode, w, h, flags, padded, plant = case
    hs, vs = cases.MODES[mode]
    frames = [cases.frame(w, h, mode, plant, seed) for seed in (0, 1)]   # two different frames, the same tables
    qts = frames[0][1]
    pitch = cases.out_pitch(w, kind) if padded else 0
    desc = zj.FrameDesc.make(w, h, hs, vs, 3, cases.colorspace(kind), qts, flags=cases.desc_flags(kind, flags), out_pitch=pitch)
    out_len = zj.lib().zj_out_len(C.byref(desc))
    cat = [np.concatenate([f[0][c] for f in frames]) for c in range(3)]
    bufs = _upload(zj, ctx, cat, 2 * out_len)
    try:
        ctx.decode_planes_device(desc, 2, bufs[0], bufs[1], bufs[2], bufs[3])
        ctx.sync()
        got = np.empty(2 * out_len, np.uint8)
        ctx.d2h(got, bufs[3])
    finally:
        for b in bufs:
            ctx.device_free(b)
    got = got.reshape(2, h, -1)
    for seed in (0, 1):
        _check_rows(got[seed], cases.expected(w, h, mode, kind, flags, plant, seed), (name, kind, seed))


@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_scattered_launch_of_two_frames_matches_oracle(zj, ctx, kind):
    """two 768 x 64 frames, each an allocation of its own, handed over in descending address order so that the launch cannot
    take the strided form: the frames' addresses travel in the kernel arguments"""
    w, h, mode = 768, 64, "hv"
    frames = [cases.frame(w, h, mode, None, seed) for seed in (0, 1)]
    desc = zj.FrameDesc.make(w, h, 2, 2, 3, cases.colorspace(kind), frames[0][1], flags=cases.desc_flags(kind, 0))
    out_len = zj.lib().zj_out_len(C.byref(desc))
    sets = [_upload(zj, ctx, list(f[0]), out_len) for f in frames]
    try:
        order = sorted(range(2), key=lambda i: -sets[i][0])   # luma planes at falling addresses: not a strided batch
        ctx.decode_frames_device(desc, [sets[i][0] for i in order], [sets[i][1] for i in order], [sets[i][2] for i in order],
                                 [sets[i][3] for i in order])
        ctx.sync()
        for i in range(2):
            got = np.empty(out_len, np.uint8)
            ctx.d2h(got, sets[i][3])
            _check_rows(got.reshape(h, -1), cases.expected(w, h, mode, kind, 0, None, i), (kind, i))
    finally:
        for s in sets:
            for b in s:
                ctx.device_free(b)
