"""CPU: the conversion-edge cases (tests/convert_cases.py) keep their edges.  For every stage whose store ends in
zj_resize.h's conversions, the stage's numpy model gives the value v of every element of every launch that
test_convert_edges_emu.py and test_gpu_convert_edges.py run; the classifier must then find every edge class of every dtype at
least MIN times, in the three-channel launches and in the one-channel ones.  A class a stage cannot reach at all is listed in
UNREACHABLE with its reason, and the test fails if it turns out to be reached.  A condition on the inputs: checked with the
models alone, no kernel and no emulation of a conversion runs here."""
import numpy as np
import pytest

import convert_cases as cc
import resize_model as rm

MIN = 8
# stage -> {class: why no input of the stage reaches it}
UNREACHABLE = {
    "to_tensor": {"u8_exact_half": "v = px << 16, one of 256 values: the low 16 bits are zero, never 0x8000"},
    "crop_tensor": {"u8_exact_half": "v = px << 16, one of 256 values: the low 16 bits are zero, never 0x8000"},
}
ALL = [c for dt in (cc.F32, cc.F16, cc.BF16, cc.U8) for c in cc.CLASSES[dt]]
_COUNTS = {}


def counts(stage, channels):
    if (stage, channels) not in _COUNTS:
        _COUNTS[stage, channels] = cc.stage_counts(stage, channels)  # (raises on a NaN in any model output)
    return _COUNTS[stage, channels]


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("dtype", [cc.F32, cc.F16, cc.BF16, cc.U8], ids=["f32", "f16", "bf16", "u8"])
@pytest.mark.parametrize("stage", cc.STAGES)
def test_every_reachable_class_is_reached(stage, dtype, channels):
    got = counts(stage, channels)
    classes = cc.CLASSES[dtype] + (cc.BICUBIC_CLASSES if stage == "resize_bicubic" and dtype == cc.U8 else [])
    for k in classes:
        if k in UNREACHABLE.get(stage, {}):
            assert got[k] == 0, f"{stage}: {k} is listed as unreachable ({UNREACHABLE[stage][k]}) but {got[k]} elements reach it"
        else:
            assert got[k] >= MIN, f"{stage} C {channels}: only {got[k]} elements in class {k}"


def test_the_unreachable_table_names_real_stages_and_classes():
    for stage, table in UNREACHABLE.items():
        assert stage in cc.STAGES and set(table) <= set(ALL + cc.BICUBIC_CLASSES)


def test_every_factor_is_finite_and_survives_float32():
    for name, (sc, bi) in cc.SETS.items():
        sc, bi = np.asarray(sc, np.float32), np.asarray(bi, np.float32)
        assert np.isfinite(sc).all() and np.isfinite(bi).all(), name
        assert rm.factors(3, sc, bi)[0].all(), name  # (no s = scale * 2^-16 rounds to zero: |scale| >= 2^-133)


def test_the_outputs_have_a_lead_whole_groups_a_tail_and_a_half_filled_pair():
    for (ow, oh) in cc.OUTS:
        assert ow % 2 == 1 and ow % 8 != 0
    assert any(ow > 16 for ow, _ in cc.OUTS) and any(ow < 8 for ow, _ in cc.OUTS)


def test_the_classifier_on_hand_made_values():
    """one element per class, from its definition"""
    one = lambda v, s, b: {k for k, n in cc.classify(np.array([[[v]]]), [s], [b]).items() if n}
    assert "half_largest_finite" in one(255 << 16, 65504.0 / 255, 0.0)
    assert {"half_inf_from_finite"} <= one(255 << 16, 256.94118, 0.0)          # 65520: the tie that rounds to inf
    assert {"half_subnormal", "half_subnormal_tie", "half_subnormal_inexact"} <= one(3 << 16, 2.0 ** -25, 0.0)  # 1.5 x 2^-24
    assert {"half_zero_from_nonzero"} <= one(1 << 16, 2.0 ** -25, 0.0)         # 2^-25 ties to even: zero
    assert {"half_smallest_normal_rounded_up"} <= one(1 << 16, -2.0 ** -30, 2.0 ** -14)
    assert {"half_tie", "bf16_tie"} <= one(1 << 16, 1.0, 2048.0) | one(128 << 16, 2.0 ** -7, 256.0)
    assert {"f32_negzero", "half_negzero", "bf16_negzero"} <= one(0, -1.0, -0.0)
    assert {"f32_zero_from_cancellation"} <= one(255 << 16, 1.0, -255.0)
    assert {"f32_inf"} <= one(255 << 16, 3.0e38, 0.0)
    assert {"bf16_inf_from_finite"} <= one((255 << 16) + 0x8000, 2.0 ** 120, 0.0)  # 255.5 x 2^120: a tie, up to 2^128
    assert {"f32_product_subnormal", "f32_sum_subnormal", "bf16_subnormal"} <= one(1 << 16, 2.0 ** -130, 0.0)
    assert {"bf16_zero_from_nonzero"} <= one(1 << 10, 2.0 ** -133, 0.0)         # 2^-139, below half of bf16's 2^-133
    assert {"fma_differs"} <= one(77 << 16, 1 / (255 * 0.229), -0.485 / 0.229) | one(78 << 16, 1 / (255 * 0.229), -0.485 / 0.229) \
        | one(79 << 16, 1 / (255 * 0.229), -0.485 / 0.229) | one(80 << 16, 1 / (255 * 0.229), -0.485 / 0.229)
    assert {"u8_exact_half"} <= one(0x18000, 1.0, 0.0)
    assert one(128 << 16, 1.0, 0.0) == set()


def test_the_bf16_model_is_nearest_even_at_its_edges():
    """resize_model.bf16_bits against the rounding written out in float64"""
    ys = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.0e38, 3.39e38, -3.39e38, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134,
                   -0.0, 2.0 ** -126 - 2.0 ** -134], np.float32)
    want = [0x3F80, 0x3F80, 0x3F82, 0x7F62, 0x7F7F, 0xFF7F, 0x0001, 0x0000, 0x0002, 0x8000, 0x0080]
    assert rm.bf16_bits(ys).tolist() == want
