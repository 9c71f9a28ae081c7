"""CPU: which path every file of a batch takes in the three file-batch calls of zj_jpeg.cpp and the oriented crop-tensor
one -- a shared *_mixed_host call with its neighbours, its own single-file call, or a status
and no call at all.  The GPU tests cannot see this: both paths give the same bytes by design, so a slip that sends every
file through its own call would pass them and cost only the speed the batch calls exist for.

The front-end is built over stand-ins that launch nothing and record their calls (tests/route_stub).  A mixed run is read
from (d_out - base) / img and nframes of the *_mixed_host call, a single-file path from the d_out of its last stage.
Order matters too: the files that go alone are finished while the batch is classified, the runs afterwards, and a run whose
call fails sends its files through the single-file call, in order, before the next run starts."""
import ctypes as C
import io

import numpy as np
import pytest

import cmyk_cases as cc
import orient_model as om
import route_stub_c as rs
import sampling_cases as sc

OK, ARG, HIP, UNSUP = 0, rs.status("ZJ_ERR_ARG"), rs.status("ZJ_ERR_HIP"), rs.status("ZJ_ERR_UNSUPPORTED")
FLAGS = rs.flag("ZJ_FLAG_GRAY_TO_RGB") | rs.flag("ZJ_FLAG_CMYK_TO_RGB") | rs.flag("ZJ_FLAG_ANY_SAMPLING")
CS_RGB, CS_GRAY, CS_YCBCR, HWC, CHW, F32, NCHW, BILINEAR, FILL = 0, 1, 2, 0, 1, 0, 0, 0, 0
W, H = 64, 48            # every file (stored size; the turned one is shown 48 x 64)
OW, OH = 16, 16          # every output
IMG = 3 * OW * OH * 4    # bytes of one image of the output: 3 channels of float32
CTX = C.c_void_p(0x1000)  # (the front-end never looks inside its context)
# the batch: index -> kind
I420, I444, IGRAY, ICMYK, I422, I411, ICUT, ITURNED, INULL = range(9)
N = 9


def pillow_file(mode, subsampling=None):
    from PIL import Image
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.stack([xx * 4, yy * 5, (xx + yy) * 2], axis=2).astype(np.uint8)
    im = Image.fromarray(rgb).convert(mode)
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=90, **({} if subsampling is None else {"subsampling": subsampling}))
    return buf.getvalue()


class Decoders:
    """n decoders of one option set, each with its file prepared; None in a file's place: a null slot"""

    def __init__(self, files, out_layout=HWC, entropy=None, colorspace=CS_RGB, flags=FLAGS):
        L = rs.lib()
        self.files = [None if f is None else np.frombuffer(f, np.uint8).copy() for f in files]  # (alive while the decoders are)
        self.handles, self.prepared = [], []
        for k, f in enumerate(self.files):
            if f is None:
                self.handles.append(None)
                self.prepared.append(None)
                continue
            o = rs.Options()
            o.out_colorspace, o.out_layout, o.flags, o.num_threads = colorspace, out_layout, flags, 1
            o.entropy = entropy[k] if entropy else 0
            d = L.zj_decoder_new(C.byref(o))
            assert d
            self.handles.append(d)
            self.prepared.append(None)
        self.array = (C.c_void_p * len(files))(*self.handles)
        self.prepare()

    def prepare(self):
        """every file prepared (again: a call that fails leaves its error in the decoder until the next file)"""
        for k, (d, f) in enumerate(zip(self.handles, self.files)):
            if d:
                self.prepared[k] = rs.lib().zj_decoder_prepare(d, f.ctypes.data, f.size, None, None)

    def close(self):
        for d in self.handles:
            if d:
                rs.lib().zj_decoder_free(d)


@pytest.fixture(scope="module")
def batch(synth):
    qts = synth.quant_tables(85)
    f420 = pillow_file("RGB", 2)
    samp411 = ((4, 1), (1, 1), (1, 1))
    files = [None] * N
    files[I420] = f420
    files[I444] = pillow_file("RGB", 0)
    files[IGRAY] = pillow_file("L")
    files[ICMYK] = cc.encode_baseline(cc.small_planes(W, H, 1, 1, seed=3), qts, W, H, 1, 1, adobe=0)
    files[I422] = pillow_file("RGB", 1)
    files[I411] = sc.encode(sc.small_planes(W, H, samp411, seed=4), qts, W, H, samp411)
    files[ICUT] = f420[:f420.index(b"\xff\xdb") + 20]  # (ends inside its first quantisation table)
    files[ITURNED] = om.splice(f420, om.exif_segment(6))
    ds = Decoders(files)
    assert [rc == OK for rc in ds.prepared[:INULL]] == [k != ICUT for k in range(INULL)], ds.prepared
    assert rs.lib().zj_decoder_orientation(ds.handles[ITURNED]) == 6
    yield ds
    ds.close()


def expected(kinds, failing_runs=()):
    """The routing events of a batch whose file k is "m" (mixed), "s" (its own call, which reaches its last stage) or "-"
    (no event: a status from the checks, a null slot, or an own call that is refused in front of every stage).
    failing_runs: the 1-based numbers of the *_mixed_host calls that fail."""
    ev = [("single", k) for k, c in enumerate(kinds) if c == "s"]
    k0, run = 0, 0
    while k0 < len(kinds):
        if kinds[k0] != "m":
            k0 += 1
            continue
        k1 = k0
        while k1 < len(kinds) and kinds[k1] == "m":
            k1 += 1
        run += 1
        ev.append(("mixed", k0, k1 - k0))
        if run in failing_runs:
            ev += [("single", k) for k in range(k0, k1)]
        k0 = k1
    return ev


def events(last_stages):
    """the recorded routing: ("mixed", first file, nframes) and ("single", file) in call order.  Every other stage of a
    single-file call writes into the context's buffer, not into the batch's output."""
    ev = []
    for name, file, nframes in rs.log():
        if name.endswith("_mixed_host"):
            ev.append(("mixed", file, nframes))
        elif file >= 0:
            assert name in last_stages, (name, file)
            ev.append(("single", file))
    return ev


def run(call, ds, n, *args, fail_nth=0, scan_rc=OK, out_cap=None, img=IMG):
    """call(ds, n, ctx, *args, d_out, out_cap, rcs) recorded: (the call's status, rcs, the log's events are read after).
    img: bytes of one image of the call's output (0: a size that has none)"""
    ds.prepare()
    out = np.zeros(n * IMG, np.uint8)
    rcs = (C.c_int * n)(*([77] * n))
    rs.begin(out.ctypes.data, img, n, fail_nth, scan_rc)
    rc = call(ds.array, n, CTX, *args, out.ctypes.data, n * IMG if out_cap is None else out_cap, rcs)
    assert not out.any()  # (nothing writes)
    return rc, list(rcs)


def u32(vals):
    return (C.c_uint * len(vals))(*vals)


def resized(ds, n, windows, max_prescale_log2=0, apply_orientation=1, size=(OW, OH), **kw):
    return run(rs.lib().zj_decoder_finish_pixels_resized_crop_batch_device, ds, n, u32(windows), size[0], size[1], F32, NCHW, None, None, None,
               BILINEAR, max_prescale_log2, apply_orientation, **kw)


def crop_tensor(ds, n, origins, oriented, size=(OW, OH), **kw):
    L = rs.lib()
    f = L.zj_decoder_finish_pixels_crop_tensor_batch_oriented_device if oriented else L.zj_decoder_finish_pixels_crop_tensor_batch_device
    return run(f, ds, n, u32(origins), size[0], size[1], F32, NCHW, None, None, None, **kw)


def warped(ds, n, matrices, apply_orientation=1, edge=FILL, size=(OW, OH), **kw):
    m = (C.c_double * (6 * n))(*[v for mk in matrices for v in mk])
    return run(rs.lib().zj_decoder_finish_pixels_warped_batch_device, ds, n, m, apply_orientation, size[0], size[1], F32, NCHW, None, None, None,
               edge, **kw)


def whole_windows():
    return [v for k in range(N) for v in ((0, 0, H, W) if k == ITURNED else (0, 0, W, H))]


INSIDE = (1.0, 0.0, 8.0, 0.0, 1.0, 8.0)        # the output sees the frame's pixels 8..24
OUTSIDE = (1.0, 0.0, 1000.0, 0.0, 1.0, 1000.0)  # ... nothing of the frame
RESIZE_LAST = {"zjint_resize_one"}
TENSOR_LAST = {"zjint_crop_tensor_frame", "zjint_to_tensor_one"}
WARP_LAST = {"zjint_warp_one"}


def kinds_of(**over):
    base = {I420: "m", I444: "m", IGRAY: "m", ICMYK: "s", I422: "m", I411: "s", ICUT: "-", ITURNED: "m", INULL: "-"}
    base.update({globals()[k]: v for k, v in over.items()})
    return [base[k] for k in range(N)]


def test_resized_batch(batch):
    rc, rcs = resized(batch, N, whole_windows())
    assert rc == OK and rcs == [OK, OK, OK, OK, OK, OK, ARG, OK, ARG]
    # gray shown as RGB and the turned file are mixed; the damaged file gets resized_checks' status and reaches no stub
    assert events(RESIZE_LAST) == expected(kinds_of()) == [("single", ICMYK), ("single", I411), ("mixed", 0, 3), ("mixed", I422, 1),
                                                           ("mixed", ITURNED, 1)]
    # a window the checks refuse: that status, no call, and the run is split there
    wins = whole_windows()
    wins[4 * I444 + 2] = 0
    rc, rcs = resized(batch, N, wins)
    assert rc == OK and rcs == [OK, ARG, OK, OK, OK, OK, ARG, OK, ARG]
    assert events(RESIZE_LAST) == expected(kinds_of(I444="-"))
    # max_prescale_log2 out of range: every file through its own call, which refuses it in front of every stage
    rc, rcs = resized(batch, N, whole_windows(), max_prescale_log2=4)
    assert rc == OK and rcs == [ARG] * N and rs.log() == []
    # with a prescale the same routing
    rc, rcs = resized(batch, N, whole_windows(), max_prescale_log2=3)
    assert rc == OK and events(RESIZE_LAST) == expected(kinds_of())


def test_resized_batch_failed_runs(batch):
    for nth in (1, 2, 3):
        rc, rcs = resized(batch, N, whole_windows(), fail_nth=nth)
        assert rc == OK and rcs == [OK, OK, OK, OK, OK, OK, ARG, OK, ARG]
        assert events(RESIZE_LAST) == expected(kinds_of(), failing_runs=(nth,))
    assert expected(kinds_of(), failing_runs=(1,))[2:6] == [("mixed", 0, 3), ("single", 0), ("single", 1), ("single", 2)]


@pytest.mark.parametrize("oriented", [False, True])
def test_crop_tensor_batch(batch, oriented):
    origins = [8, 8] * N
    rc, rcs = crop_tensor(batch, N, origins, oriented)
    assert rc == OK and rcs == [OK, OK, OK, OK, OK, OK, ARG, OK, ARG]
    # gray shown as RGB goes alone here; the turned file only when its orientation is applied; the damaged file's own call
    # refuses it in front of every stage
    kinds = kinds_of(IGRAY="s", ITURNED="s" if oriented else "m")
    assert events(TENSOR_LAST) == expected(kinds)
    names = {file: name for name, file, _ in rs.log() if file >= 0 and not name.endswith("_mixed_host")}
    assert names == {k: "zjint_to_tensor_one" for k in (IGRAY, ICMYK, I411) + ((ITURNED,) if oriented else ())}
    # a window outside the frame: the single-file call, which refuses it
    origins[2 * I444] = W - 8
    rc, rcs = crop_tensor(batch, N, origins, oriented)
    assert rc == OK and rcs == [OK, ARG, OK, OK, OK, OK, ARG, OK, ARG]
    kinds[I444] = "-"
    assert events(TENSOR_LAST) == expected(kinds)
    # a failed run: its files through the fused single-file kernel, in order
    origins[2 * I444] = 8
    kinds[I444] = "m"
    rc, rcs = crop_tensor(batch, N, origins, oriented, fail_nth=1)
    assert rc == OK and rcs == [OK, OK, OK, OK, OK, OK, ARG, OK, ARG]
    assert events(TENSOR_LAST) == expected(kinds, failing_runs=(1,))
    assert [n for n, f, _ in rs.log() if f in (I420, I444) and not n.endswith("_mixed_host")] == ["zjint_crop_tensor_frame"] * 2


@pytest.mark.parametrize("apply_orientation", [0, 1])
def test_warped_batch(batch, apply_orientation):
    rc, rcs = warped(batch, N, [INSIDE] * N, apply_orientation)
    assert rc == OK and rcs == [OK, OK, OK, OK, OK, OK, ARG, OK, ARG]
    assert events(WARP_LAST) == expected(kinds_of())  # (the turned file is mixed either way)
    # an output that sees nothing of the frame: the single-file call, which fills it
    ms = [INSIDE] * N
    ms[I444] = ms[ITURNED] = OUTSIDE
    rc, rcs = warped(batch, N, ms, apply_orientation)
    assert rc == OK and rcs == [OK, OK, OK, OK, OK, OK, ARG, OK, ARG]
    assert events(WARP_LAST) == expected(kinds_of(I444="s", ITURNED="s"))
    # a matrix the warp does not take, an unknown edge mode: not plain, the single-file call refuses
    ms[I444] = (float("nan"), 0.0, 0.0, 0.0, 1.0, 0.0)
    rc, rcs = warped(batch, N, ms, apply_orientation)
    assert rc == OK and rcs == [OK, ARG, OK, OK, OK, OK, ARG, OK, ARG]
    assert events(WARP_LAST) == expected(kinds_of(I444="-", ITURNED="s"))
    rc, rcs = warped(batch, N, [INSIDE] * N, apply_orientation, edge=7)
    assert rc == OK and rcs == [ARG] * N and rs.log() == []
    rc, rcs = warped(batch, N, [INSIDE] * N, apply_orientation, fail_nth=2)
    assert rc == OK and events(WARP_LAST) == expected(kinds_of(), failing_runs=(2,))


def test_prologue(batch):
    calls = [lambda ds, n, **kw: resized(ds, n, whole_windows()[:4 * n], **kw),
             lambda ds, n, **kw: crop_tensor(ds, n, [8, 8] * n, False, **kw),
             lambda ds, n, **kw: crop_tensor(ds, n, [8, 8] * n, True, **kw),
             lambda ds, n, **kw: warped(ds, n, [INSIDE] * n, **kw)]
    f420 = bytes(batch.files[I420])
    other = Decoders([f420, f420, f420], out_layout=CHW)
    ycc = Decoders([f420], colorspace=CS_YCBCR)
    try:
        mixed_layouts = Decoders([None, None, None])
        mixed_layouts.array = (C.c_void_p * 3)(batch.handles[I420], other.handles[1], batch.handles[I444])
        mixed_spaces = Decoders([None, None, None])  # (a null slot in front: the first decoder sets the colour space)
        mixed_spaces.array = (C.c_void_p * 3)(None, batch.handles[I420], ycc.handles[0])
        nulls = Decoders([None, None])
        for call in calls:
            rc, rcs = call(batch, N, out_cap=N * IMG - 1)  # (too small for n images)
            assert rc == ARG and rcs == [77] * N and rs.log() == []
            rc, rcs = call(mixed_layouts, 3)
            assert rc == ARG and rcs == [77] * 3 and rs.log() == []
            rc, rcs = call(mixed_spaces, 3)
            assert rc == ARG and rcs == [77] * 3 and rs.log() == []
            rc, rcs = call(nulls, 2)                       # (no decoder at all)
            assert rc == ARG and rcs == [77] * 2 and rs.log() == []
    finally:
        other.close()
        ycc.close()


def test_an_output_without_bytes(batch):
    """img == 0 -- a size or dtype that has no output -- is no error of the call: every file goes through its own call, which
    says why and reaches no stage; out_cap is not looked at"""
    for size in ((0, OH), (OW, 0)):
        for out_cap in (N * IMG, 0):
            rc, rcs = resized(batch, N, whole_windows(), size=size, img=0, out_cap=out_cap)
            assert rc == OK and rcs == [ARG] * N and rs.log() == []
            for oriented in (False, True):
                rc, rcs = crop_tensor(batch, N, [8, 8] * N, oriented, size=size, img=0, out_cap=out_cap)
                assert rc == OK and rcs == [ARG] * N and rs.log() == []
            rc, rcs = warped(batch, N, [INSIDE] * N, size=size, img=0, out_cap=out_cap)
            assert rc == OK and rcs == [ARG] * N and rs.log() == []


def test_planar_decoders(batch):
    """CHW decoders: the resized call takes them in its mixed runs; the crop-tensor call (a non-HWC layout) and the warped call
    (not plain) send every file through its own call, which refuses the layout in front of every stage"""
    files = [bytes(batch.files[k]) for k in (I420, I444, I422)]
    ds = Decoders(files, out_layout=CHW)
    try:
        rc, rcs = resized(ds, 3, [0, 0, W, H] * 3)
        assert rc == OK and rcs == [OK] * 3 and events(RESIZE_LAST) == [("mixed", 0, 3)]
        for oriented in (False, True):
            rc, rcs = crop_tensor(ds, 3, [8, 8] * 3, oriented)
            assert rc == OK and rcs == [UNSUP] * 3 and rs.log() == []
        rc, rcs = warped(ds, 3, [INSIDE] * 3)
        assert rc == OK and rcs == [UNSUP] * 3 and rs.log() == []
    finally:
        ds.close()


def test_files_the_checks_refuse_get_their_status_and_no_call(batch):
    """A YCbCr decoder with the three flags: a gray, a four-component and a 4:1:1 file are prepared, and resized_checks refuses
    each (the flags give RGB).  In the resized and the warped call -- where such a file IS plain -- that is the file's status,
    nothing is called for it, and it splits the run; the crop-tensor call's pre-check hands it to the single-file call."""
    ks = (I420, IGRAY, I444, ICMYK, I411, I422)
    ds = Decoders([bytes(batch.files[k]) for k in ks], colorspace=CS_YCBCR)
    try:
        assert ds.prepared == [OK] * 6
        want = [OK, UNSUP, OK, UNSUP, UNSUP, OK]
        runs = [("mixed", 0, 1), ("mixed", 2, 1), ("mixed", 5, 1)]
        rc, rcs = resized(ds, 6, [0, 0, W, H] * 6)
        assert rc == OK and rcs == want and rs.log() == [("zjint_crops_resized_mixed_host", f, n) for _, f, n in runs]
        for ao in (0, 1):
            rc, rcs = warped(ds, 6, [INSIDE] * 6, ao)
            assert rc == OK and rcs == want and rs.log() == [("zjint_crops_warped_mixed_host", f, n) for _, f, n in runs]
        for oriented in (False, True):
            rc, rcs = crop_tensor(ds, 6, [8, 8] * 6, oriented)
            assert rc == OK and rcs == want and rs.log() == [("zjint_crops_tensor_mixed_host", f, n) for _, f, n in runs]
    finally:
        ds.close()


def test_gray_file_without_the_flag(batch):
    """An RGB decoder WITHOUT ZJ_FLAG_GRAY_TO_RGB.  The front-end gives a one-component file a GRAYSCALE descriptor whatever
    the decoder asks for (fill_info), so `zero_output(fd) && !gray_to_rgb(fd)` -- the all-zero output that goes single in the
    resized and warped calls -- is false for every descriptor a decoder makes: that branch cannot be reached through these
    entry points, and the file is mixed there.  The crop-tensor pre-check (one component, a non-GRAYSCALE decoder) sends it to
    the single-file call, which refuses it.
    Not reachable either: a frame orient_size refuses in the warped call.  The orientation it gets is 1..8 and a parsed
    frame is 1..65535 a side, so it never fails for a prepared file."""
    ds = Decoders([bytes(batch.files[k]) for k in (I420, IGRAY, I444)], flags=0)
    try:
        assert ds.prepared == [OK] * 3
        rc, rcs = resized(ds, 3, [0, 0, W, H] * 3)
        assert rc == OK and rcs == [OK] * 3 and events(RESIZE_LAST) == [("mixed", 0, 3)]
        rc, rcs = warped(ds, 3, [INSIDE] * 3)
        assert rc == OK and rcs == [OK] * 3 and events(WARP_LAST) == [("mixed", 0, 3)]
        for oriented in (False, True):
            rc, rcs = crop_tensor(ds, 3, [8, 8] * 3, oriented)
            assert rc == OK and rcs == [OK, UNSUP, OK] and events(TENSOR_LAST) == [("mixed", 0, 1), ("mixed", 2, 1)]
    finally:
        ds.close()


def test_scan_left_for_the_device(batch):
    """a decoder whose entropy stage is left for the device is never in a mixed run and splits its neighbours'; its status
    is the entropy stage's"""
    L = rs.lib()
    f420 = bytes(batch.files[I420])
    ds = Decoders([f420, f420, f420], entropy=[0, 2, 0])
    try:
        assert ds.prepared == [OK, OK, OK]
        assert [L.zj_decoder_scan_blob(d, None, None) for d in ds.handles] == [ARG, OK, ARG]  # (only the second holds a scan)
        for scan_rc in (OK, HIP):
            alone = ["s" if scan_rc == OK else "-"]
            want_rcs = [OK, scan_rc, OK]
            rc, rcs = resized(ds, 3, [0, 0, W, H] * 3, scan_rc=scan_rc)
            assert rc == OK and rcs == want_rcs and events(RESIZE_LAST) == expected(["m"] + alone + ["m"])
            assert "zjint_scan_to_planes" in [n for n, _, _ in rs.log()]
            for oriented in (False, True):
                rc, rcs = crop_tensor(ds, 3, [8, 8] * 3, oriented, scan_rc=scan_rc)
                assert rc == OK and rcs == want_rcs and events(TENSOR_LAST) == expected(["m"] + alone + ["m"])
            rc, rcs = warped(ds, 3, [INSIDE] * 3, scan_rc=scan_rc)
            assert rc == OK and rcs == want_rcs and events(WARP_LAST) == expected(["m"] + alone + ["m"])
    finally:
        ds.close()
