"""CPU: the launch groups of the resized-crop calls (zj_rzgroup.h: rz_group_next, rz_scratch_need)
-- the library's own planner, reached through tests/emu_crop_mixed at caps of a few KB, against a model written here from
the rule: greedy and in order, a frame that alone exceeds the cap forms a group of its own, a turned frame (orientation
other than 1) counts its bytes twice, every image starts on a 16-byte boundary."""
import numpy as np
import pytest

import emu_crop_mixed_c as em

RZ_GROUP_CAP = 256 << 20
LAYOUTS = [(1, False), (3, False), (3, True)]  # channels, CHW


def image_bytes(w, h, ch):
    return (w * h * ch + 15) // 16 * 16


def model_groups(sizes, oris, ch, cap):
    """lists of frame indices"""
    groups, total = [[]], 0
    for f, ((w, h), o) in enumerate(zip(sizes, oris)):
        cost = image_bytes(w, h, ch) * (1 if o == 1 else 2)
        if groups[-1] and total + cost > cap:
            groups.append([])
            total = 0
        groups[-1].append(f)
        total += cost
    return groups


def frame_lists(cap, ch, count, seed):
    """`count` lists of 1..14 crops of 1 x 1 up to about 1.5 x cap bytes (sizes log-uniform: most lists hold groups of several
    frames, most lists a frame or two near or above the cap), orientations 1..8 mixed, half of them 1"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(1, 15))
        sizes, oris = [], []
        for _ in range(n):
            pixels = max(1, int(np.exp(rng.uniform(0, np.log(1.5 * cap / ch)))))
            w = max(1, min(pixels, int(np.exp(rng.uniform(0, np.log(pixels))))))
            sizes.append((w, max(1, pixels // w)))
            oris.append(1 if rng.random() < 0.5 else int(rng.integers(2, 9)))
        out.append((sizes, oris))
    out[0] = ([(1, 1)], [1])
    out[1] = ([(1, 1)] * 3, [6, 1, 3])
    return out


@pytest.mark.parametrize("cap", [4096, 65536])
@pytest.mark.parametrize("ch,chw", LAYOUTS)
def test_groups_and_regions_follow_the_rule(cap, ch, chw):
    bpp = 1 if chw else ch
    multi = crossing_turned = 0
    for sizes, oris in frame_lists(cap, ch, 60, seed=cap + 10 * ch + chw):
        n = len(sizes)
        need, groups = em.rz_groups(sizes, oris, ch, chw, cap)
        what = f"cap {cap}, {ch} channels, chw {chw}, sizes {sizes}, orientations {oris}"
        # the groups partition [0, n) in order, and are the model's
        assert [f for _, fr in groups for f, _, _ in fr] == list(range(n)), what
        assert [[f for f, _, _ in fr] for _, fr in groups] == model_groups(sizes, oris, ch, cap), what
        cost = [image_bytes(w, h, ch) * (1 if o == 1 else 2) for (w, h), o in zip(sizes, oris)]
        for g, (gbytes, fr) in enumerate(groups):
            idx = [f for f, _, _ in fr]
            assert gbytes == sum(cost[f] for f in idx), what
            # within the cap unless a single frame; maximal: the next frame would not have fit
            assert len(idx) == 1 or gbytes <= cap, what
            if idx[-1] + 1 < n:
                assert gbytes + cost[idx[-1] + 1] > cap, what
            multi += len(idx) > 1
            crossing_turned += g > 0 and any(oris[f] != 1 for f in idx)
            regions, first_end, second_start = [], 0, None
            for f, crop, read in fr:
                (w, h), o = sizes[f], oris[f]
                assert crop[1:] == (w, h, w * bpp), what
                regions.append((crop[0], crop[0] + image_bytes(w, h, ch)))
                first_end = max(first_end, regions[-1][1])
                if o == 1:
                    assert read == crop, what
                    continue
                dw, dh = (h, w) if o >= 5 else (w, h)  # orient_size: 5..8 transpose
                assert read[1:] == (dw, dh, dw * bpp), what
                regions.append((read[0], read[0] + image_bytes(dw, dh, ch)))
                second_start = read[0] if second_start is None else min(second_start, read[0])
            # 16-byte aligned, pairwise disjoint, inside the group's bytes; the second region behind the first
            assert all(a % 16 == 0 for a, _ in regions), what
            regions.sort()
            assert all(e0 <= a1 for (_, e0), (a1, _) in zip(regions, regions[1:])), what
            assert regions[0][0] == 0 and regions[-1][1] <= gbytes, what
            assert second_start is None or second_start >= first_end, what
        assert need == max(gbytes for gbytes, _ in groups), what
    # (the inputs do reach what the test is about: groups of several frames, turned frames in a group that is not the first)
    assert multi >= 30 and crossing_turned >= 15, (multi, crossing_turned)


def test_the_large_gpu_cases_form_two_groups_at_the_library_cap():
    """tests/test_gpu_resize.py's six windows of 4096 x 4096 (the last 4095 x 4093) and tests/test_gpu_mixed.py's frames of
    9600 x 9600 and 9600 x 9400, RGB: the two cases that reach a second group on the GPU"""
    six = [(4096, 4096)] * 5 + [(4095, 4093)]
    need, groups = em.rz_groups(six, [1] * 6, 3, False)
    assert [[f for f, _, _ in fr] for _, fr in groups] == [[0, 1, 2, 3, 4], [5]]
    assert need == 5 * 4096 * 4096 * 3 <= RZ_GROUP_CAP
    assert em.rz_groups(six, [1] * 6, 3, False, RZ_GROUP_CAP) == (need, groups)  # (cap 0 is the library's)
    need, groups = em.rz_groups([(9600, 9600), (9600, 9400)], [1, 1], 3, False)
    assert [[f for f, _, _ in fr] for _, fr in groups] == [[0], [1]]
    assert need == 9600 * 9600 * 3 > RZ_GROUP_CAP
