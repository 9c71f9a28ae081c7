"""CPU: the MODEL of an odd-sampled file's image (tests/sampling_cases.py: clamped IDCT per component, box
replication, the full decode's colour arithmetic), over the planes the front-end yields, against Pillow's decode of the same
file.  Smooth-plus-noise content, flat tables 4 / 6, at 100 x 75 and 33 x 17.

Pillow (libjpeg) replicates boxes for every ratio but 2, so the ratio-4 samplings (4,1), (4,2), (1,4) must agree with it as
well as a 4:4:4 file of the same content does -- the bound is that file's largest difference in the same test plus 1, chroma
being quantised from other samples.  Ratio-2 components go through libjpeg's triangle filter there and through boxes here: a
known deviation (5 to 8 on this content), printed, not asserted.  profiles/any_sampling.txt holds the figures."""
import importlib
import io

import numpy as np
import pytest

import sampling_cases as sc

RATIO4 = sc.SAMPLINGS[:3]
SIZES = ((100, 75), (33, 17))


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


def model_and_pillow(zj, data, samp, w, h, qts):
    from PIL import Image
    o = zj.ZuneJpegOptions()
    o.flags = zj.FLAG_ANY_SAMPLING
    d = zj.Decoder(o)
    d.prepare(data)
    kept = []
    for c in range(3):
        p = d.plane(c)
        cw, ch = sc.comp_size(w, h, samp, c)
        kept.append(p[: -(-ch // 8), : -(-cw // 8)])  # (a standard file keeps the MCU layout: cut to the component's own blocks)
    e = sc.model_image(kept, [qts[0], qts[1], qts[1]], samp, 0, 0, w, h, stored_rgb=d.stored_rgb)
    pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert pil.shape == e.shape
    return int(np.abs(e.astype(np.int32) - pil.astype(np.int32)).max())


@pytest.mark.parametrize("wh", SIZES)
def test_ratio_4_files_agree_with_pillow_as_444_does(zj, wh, capsys):
    w, h = wh
    qts = sc.flat_tables()
    img = sc.content(w, h, seed=w)
    figures = {}
    for samp in (sc.STANDARD[0],) + tuple(sc.SAMPLINGS):
        data = sc.encode(sc.quantised_planes(img, w, h, samp, [qts[0], qts[1], qts[1]]), qts, w, h, samp)
        figures[sc.name(samp)] = model_and_pillow(zj, data, samp, w, h, qts)
    with capsys.disabled():
        print("\nmodel against Pillow, %d x %d, largest difference:" % wh, figures)
    bound = figures[sc.name(sc.STANDARD[0])] + 1
    for samp in RATIO4:
        assert figures[sc.name(samp)] <= bound, (sc.name(samp), figures)


@pytest.mark.parametrize("wh", SIZES)
def test_a_stored_rgb_file_agrees_with_pillow_as_444_does(zj, wh):
    w, h = wh
    qts = sc.flat_tables()
    img = sc.content(w, h, seed=w)
    samp = sc.STANDARD[0]
    planes = sc.quantised_planes(img, w, h, samp, [qts[0], qts[1], qts[1]])
    bound = model_and_pillow(zj, sc.encode(planes, qts, w, h, samp), samp, w, h, qts) + 1
    data = sc.encode(planes, qts, w, h, samp, adobe=0, ids=tuple(b"RGB"), jfif=False)
    assert model_and_pillow(zj, data, samp, w, h, qts) <= bound
