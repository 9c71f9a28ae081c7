"""CPU: the launch-group planner of the resized-crop calls (zune-jpeg_amd/csrc/zj_rzgroup.h) with gray-to-RGB frames
 at caps of a few KB: random mixes of gray-expanded, turned and colour frames.  Every image starts on a 16-byte
boundary and overlaps no other of its group, a group's bytes stay within the cap unless the group is one frame, the scratch
need is the largest group's, and a call without a gray frame is placed exactly as the planner placed it before there were
any (tests/emu_crop_mixed: zjem_rz_groups, which builds its frames without the member)."""
import numpy as np
import pytest

import emu_crop_mixed_c as em
import emu_rzgroup_c as er


def image_bytes(w, h, ch):
    return (w * h * ch + 15) // 16 * 16


def random_call(rng, n, gray_share):
    sizes = [(int(rng.integers(1, 60)), int(rng.integers(1, 40))) for _ in range(n)]
    oris = [int(rng.integers(1, 9)) if rng.random() < 0.4 else 1 for _ in range(n)]
    gray = [1 if rng.random() < gray_share else 0 for _ in range(n)]
    return sizes, oris, gray


def displayed(w, h, o):
    return (h, w) if o >= 5 else (w, h)


@pytest.mark.parametrize("chw", [False, True], ids=["HWC", "CHW"])
@pytest.mark.parametrize("cap", [2048, 4096, 20000])
def test_random_mixes_of_gray_turned_and_colour_frames(cap, chw):
    rng = np.random.default_rng(cap + chw)
    bpp = 1 if chw else 3
    for trial in range(60):
        n = int(rng.integers(1, 40))
        sizes, oris, gray = random_call(rng, n, (0.0, 0.1, 0.5, 1.0)[trial % 4])
        need, groups = er.groups(sizes, oris, gray, 3, chw, cap)
        what = f"cap {cap}, chw {chw}, sizes {sizes}, orientations {oris}, gray {gray}"
        assert [p["f"] for _, fr in groups for p in fr] == list(range(n)), what
        cost = [image_bytes(w, h, 1) * (1 if o == 1 else 2) + image_bytes(w, h, 3) if g else
                image_bytes(w, h, 3) * (1 if o == 1 else 2) for (w, h), o, g in zip(sizes, oris, gray)]
        for gbytes, fr in groups:
            idx = [p["f"] for p in fr]
            assert gbytes == sum(cost[f] for f in idx), what
            assert len(idx) == 1 or gbytes <= cap, what
            if idx[-1] + 1 < n:
                assert gbytes + cost[idx[-1] + 1] > cap, what  # (greedy: the next frame would not have fit)
            spans = []
            for p in fr:
                (w, h), o, g = sizes[p["f"]], oris[p["f"]], gray[p["f"]]
                dw, dh = displayed(w, h, o)
                assert p["turned"] == (o != 1) and p["expand"] == bool(g), what
                assert p["crop"][1:] == (w, h, w * (1 if g else bpp)), what
                assert p["read"][1:] == (dw, dh, dw * bpp), what
                assert p["gray"][1:] == (dw, dh, dw * (1 if g else bpp)), what
                if o == 1:
                    assert p["gray"] == (p["crop"] if g else p["read"]), what
                if not g:
                    assert p["gray"] == p["read"], what
                    if o == 1:
                        assert p["read"] == p["crop"], what
                images = {p["crop"]: 1 if g else 3, p["gray"]: 1 if g else 3, p["read"]: 3}
                for (off, iw, ih, _), ch in images.items():
                    assert off % 16 == 0, what
                    spans.append((off, off + iw * ih * ch))
            spans.sort()
            for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                assert a1 <= b0, what
            assert spans[-1][1] <= gbytes, what
        assert need == max(g for g, _ in groups), what


@pytest.mark.parametrize("channels,chw", [(3, False), (3, True), (1, False)])
def test_a_call_without_gray_frames_is_placed_as_before(channels, chw):
    """the same frames through the planner as the callers without gray frames reach it (RzFrame of three members), with the
    member 0, and -- one channel -- with the member set, which a 1-channel call ignores"""
    rng = np.random.default_rng(3 + channels + chw)
    for trial in range(40):
        n = int(rng.integers(1, 40))
        sizes, oris, _ = random_call(rng, n, 0)
        cap = int(rng.choice([2048, 4096, 20000]))
        need0, groups0 = em.rz_groups(sizes, oris, channels, chw, cap)
        want = [(b, [(f, c, r) for f, c, r in fr]) for b, fr in groups0]
        for gray in (None, [0] * n) + (([1] * n,) if channels == 1 else ()):
            need, groups = er.groups(sizes, oris, gray, channels, chw, cap)
            got = [(b, [(p["f"], p["crop"], p["read"]) for p in fr]) for b, fr in groups]
            assert need == need0 and got == want, (sizes, oris, channels, chw, cap)
            assert not any(p["expand"] for _, fr in groups for p in fr)


def test_a_lone_gray_frame_over_the_cap_is_a_group_of_its_own():
    need, groups = er.groups([(8, 8), (100, 100), (8, 8)], [1, 6, 1], [1, 1, 0], 3, False, 4096)
    assert [[p["f"] for p in fr] for _, fr in groups] == [[0], [1], [2]]
    assert need == 2 * image_bytes(100, 100, 1) + image_bytes(100, 100, 3)
    # the third region lies behind the crops and the turned images
    p = groups[1][1][0]
    assert p["crop"][0] == 0 and p["gray"][0] == image_bytes(100, 100, 1) and p["read"][0] == 2 * image_bytes(100, 100, 1)
