"""CPU proof of the order-free inputs (tests/orderfree.py): no GPU involved.

The builders assert their own exactness condition in integer arithmetic (every sum of |terms| below 2^24 units of the layer's
granularity, every operand equal to its bf16 rounding).  Here that condition is checked against its consequence: the exact
fp32 oracle (fmaf chains in its own canonical order) and the float64 checker of the bf16 mode (another order, another
precision) both land on the builder's exact value - the oracle bit for bit - and the outputs are far from degenerate.
"""
import numpy as np
import pytest

import orderfree
from oracle import ora
from oracle.ora_bf16 import refine_bf16_ref, saliency_bf16_ref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ora_sigmoid(logits):
    """The oracle's canonical sigmoid, element by element (one call per distinct logit)."""
    u, inv = np.unique(logits, return_inverse=True)
    return np.array([ora.sigmoid(v) for v in u], np.float32)[inv].reshape(logits.shape)


@pytest.mark.parametrize("grid,frames,hidden", [(28, 2, 256), (14, 1, 128), (5, 3, 256)])
def test_selector_inputs_are_order_free(grid, frames, hidden):
    feat, sd, logits, bounds = orderfree.selector_case(grid, grid, frames, hidden)
    print(f"G={grid} hs={hidden}: conv3x3 {bounds['conv3x3']} units of 2^-7, conv1x1 {bounds['conv1x1']} units of 2^-12")
    assert bounds["conv3x3"] < 1 << 24 and bounds["conv1x1"] < 1 << 24
    # the exact oracle reaches the exact logit (its sigmoid applied to the builder's logit gives the same bits) ...
    sal = ora.selector_saliency(feat, sd)
    np.testing.assert_array_equal(bits(sal), bits(ora_sigmoid(logits)))
    # ... and so does the float64 checker, up to the ulp of its own float64 sigmoid
    assert np.abs(saliency_bf16_ref(feat, sd) - sal).max() < 1.2e-7
    # not degenerate: the sigmoid is exercised over its range, and the map has structure
    assert np.abs(logits).max() < 8.0 and logits.min() < -1.0 and logits.max() > 1.5
    if grid >= 14:
        assert np.unique(sal).size > 100, np.unique(sal).size


def test_selector_builder_refuses_operands_that_do_not_survive_bf16():
    feat, sd, _, _ = orderfree.selector_case(1, 5, 1)
    bad = feat.copy()
    bad[0, 2, 2, 7] = np.float32(1.0 + 2.0 ** -9)
    with pytest.raises(AssertionError):
        orderfree.selector_exact(bad, sd)


@pytest.mark.parametrize("grid,frames,K", [(28, 3, 500), (17, 2, 100), (40, 1, 1)])
def test_refiner_inputs_are_order_free(grid, frames, K):
    feat, kp, sd, x, o, desc, bounds = orderfree.refiner_case(grid, grid, frames, K)
    print(f"G={grid} K={K}: {bounds}")
    assert max(bounds["input_proj"], bounds["output_proj"], bounds["norm_squares"]) < 1 << 24 and bounds["hidden_max"] <= 256
    # keypoints: integer and half-integer coordinates, both kinds present, some on the zero padding
    assert np.array_equal(kp * 2, np.rint(kp * 2))
    if K >= 100:
        assert np.any(kp != np.floor(kp)) and np.any(kp == np.floor(kp))
    if grid == 17:      # G - 1 a power of two: every coordinate survives the round trip, -0.5 and G - 0.5 included
        assert kp.min() == -0.5 and kp.max() == grid - 0.5
    # the oracle's fp32 gather equals the exact one bit for bit, and its depth-0 MLP the exact descriptors
    np.testing.assert_array_equal(bits(ora.gather(feat, kp).reshape(-1, 384)), bits(x))
    np.testing.assert_array_equal(bits(ora.refine(x, sd, n_blocks=0)), bits(desc))
    # pre-normalisation outputs of the float64 checker are the exact integers; its descriptors differ by float64-vs-fp32
    # rounding of the square root and the division only
    assert np.abs(refine_bf16_ref(x, sd, n_blocks=0) - desc).max() < 1.2e-7
    if K >= 100:
        assert np.unique(o).size > 60 and np.unique(desc).size > 0.5 * desc.size / 10
        assert np.abs(o).max() > 30 and (x != 0).mean() > 0.5


def test_refiner_pre_normalisation_outputs_match_the_float64_checker_exactly():
    _, _, sd, x, o, _, _ = orderfree.refiner_case(7, 28, 2, 200)
    f8 = np.float64
    hid = np.maximum(x.astype(f8) @ sd["input_proj.weight"].astype(f8).T + sd["input_proj.bias"], 0)
    want = hid @ sd["output_proj.weight"].astype(f8).T + sd["output_proj.bias"]
    np.testing.assert_array_equal(o.astype(f8), want)
    # the same through the checker: normalised rows times their float64 norm give the integers back
    ref = refine_bf16_ref(x, sd, n_blocks=0).astype(f8) * np.sqrt((want * want).sum(-1, keepdims=True))
    assert np.abs(ref - want).max() < 1e-4 and np.array_equal(np.rint(ref), want)


def test_order_free_inputs_see_two_swapped_weights_that_the_tolerance_passes():
    """Emulated fault (CPU): two neighbouring input channels of ONE hidden channel swapped at one tap of conv.0.weight - what one
    wrong index in the packer's fragment order does.  On the synthetic weights of test_gpu_bf16_mode.py the saliency moves by
    6e-5, inside that test's 2e-4; on the order-free inputs the oracle's bits change in hundreds of cells, so a kernel that has
    to return the oracle's bits cannot carry it."""
    import synth
    from oracle.ora_bf16 import saliency_bf16_f32acc
    n, a, b = 155, 162, 163

    def swapped(sd):
        w = sd["conv.0.weight"].copy()
        w[n, [a, b], 1, 1] = w[n, [b, a], 1, 1]
        return {**sd, "conv.0.weight": w}
    sd = synth.selector_state(0)
    feat = ora.bn_tokens(synth.tokens(48, 28, 3))[0].reshape(3, 28, 28, 384)
    d = np.abs(saliency_bf16_f32acc(feat, swapped(sd)) - saliency_bf16_ref(feat, sd)).max()
    print("synthetic weights: the swap moves the saliency by", d)
    assert 1e-5 < d < 2e-4
    feat, sd, _, _ = orderfree.selector_case(28, 28, 3)
    moved = int((bits(ora.selector_saliency(feat, swapped(sd))) != bits(ora.selector_saliency(feat, sd))).sum())
    print("order-free inputs: cells whose bits change:", moved, "of", feat.shape[0] * 28 * 28)
    assert moved > 100

