"""The border-class tiling of the fp32 saliency conv (csrc/selector.hip) against the CPU oracle, bit for bit: the tiles that leave
out the taps that only multiply zero padding, at the frame counts where their pooling over frames changes shape, and against the
frame-crossing halo tiling it replaces (SSLAM_CONV_BORDER = 0, in rounds of 4 big tiles: SSLAM_CONV_TAIL = 4).

G = 28 (the flagship grid) and G = 14 are the grids the form is enabled for in the throughput range; G = 40 plans but keeps the
per-frame tiling, G = 12 does not plan.  One oracle run per grid, over 33 frames; a launch of n frames is its first n."""
import numpy as np
import pytest

import synth
from oracle import ora

pytestmark = pytest.mark.gpu

F32_MIN_NORMAL = np.float32(np.finfo(np.float32).tiny)
MAX_FRAMES = 33
# 1: every class tile partly empty, no partner frame.  2, 3: class and leftover tiles across a frame boundary.  13: a left / right tile
# on three frames (G = 28: pooled side cells 256 .. 287 are frames 9, 10, 11).  33: 165 big tiles and every kind.
FRAMES = (1, 2, 3, 13, 33)
ORDERS = {"border": {}, "off": {"SSLAM_CONV_BORDER": 0}}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def hip(T):
    from sslam_amd import lib
    lib.lib()
    return lib


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), f"{what}: {len(bad)}/{got.size} cells differ; first (frame, y, x) {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def run(T, hip, knob, feat, sd, order):
    knob("SSLAM_CONV_LATENCY_ROWS", 0)
    knob("SSLAM_CONV_TAIL", 4)
    for name, value in ORDERS[order].items():
        knob(name, value)
    w1p = dev(T, hip.pack_conv3x3(sd["conv.0.weight"]))
    sal = hip.selector_saliency(dev(T, feat), w1p, dev(T, sd["conv.0.bias"]), dev(T, sd["conv.2.weight"].reshape(-1)),
                                dev(T, sd["conv.2.bias"]), 256)
    return sal.cpu().numpy()


_cases = {}


def case(grid):
    """(features of 33 frames, selector, the oracle's saliency), computed once per grid."""
    if grid not in _cases:
        feat = synth._normal(synth._rng(7100 + grid), (MAX_FRAMES, grid, grid, synth.C_FEAT), 1.0, 0.0)
        sd = synth.selector_state(0)
        _cases[grid] = (feat, sd, ora.selector_saliency(feat, sd))
    return _cases[grid]


def test_the_grids_are_the_ones_the_form_takes(hip):
    assert hip.selector_border_plan(MAX_FRAMES, 28)[0] and hip.selector_border_plan(MAX_FRAMES, 14)[0]
    assert not hip.selector_border_plan(MAX_FRAMES, 12)[0]
    own = hip.selector_border_owners(13, 28, "left")[8]                    # pooled cells 256 .. 287 of the left class
    assert sorted(set(own[:, 0].tolist())) == [9, 10, 11] and (own[:, 2] == 0).all()


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("grid", [28, 14])
def test_border_tiling_equals_the_oracle(T, hip, knob, grid, frames, order):
    feat, sd, want = case(grid)
    assert_bits(run(T, hip, knob, feat[:frames], sd, order), want[:frames], f"G {grid} x {frames}, {order}")


@pytest.mark.parametrize("grid,frames", [(40, 3), (12, 5)])
def test_a_grid_the_form_does_not_take_is_unchanged(T, hip, knob, grid, frames):
    """G = 40 keeps the per-frame tiling, G = 12 (100 interior cells) the frame-crossing halo kernel."""
    feat = synth._normal(synth._rng(7200 + grid), (frames, grid, grid, synth.C_FEAT), 1.0, 0.0)
    sd = synth.selector_state(0)
    want = ora.selector_saliency(feat, sd)
    got = run(T, hip, knob, feat, sd, "border")
    assert_bits(got, want, f"G {grid}")
    assert_bits(run(T, hip, knob, feat, sd, "off"), got, f"G {grid}, SSLAM_CONV_BORDER = 0")


@pytest.mark.parametrize("features", ["zero", "ordinary"])
def test_a_bias_of_minus_zero(T, hip, knob, features):
    """The one accumulator a skipped step could change: -0 + (+0) is +0.  b1 = -0.0 everywhere; on all-zero features every hidden
    value is a zero of either sign, which the ReLU maps to +0: the saliency bits do not move."""
    feat, sd, _ = case(28)
    feat = np.zeros_like(feat[:3]) if features == "zero" else feat[:3]
    sd = dict(sd)
    sd["conv.0.bias"] = np.full_like(sd["conv.0.bias"], -0.0)
    assert np.signbit(sd["conv.0.bias"]).all()
    want = ora.selector_saliency(feat, sd)
    for order in ORDERS:
        assert_bits(run(T, hip, knob, feat, sd, order), want, f"b1 = -0, {features} features, {order}")


def test_border_cells_at_the_ends_of_the_range(T, hip, knob):
    """Border cells hold +-3e38, the smallest normal and subnormals; three quarters of the conv weights are negative, so that sums
    overflow to -inf, meet +inf and turn NaN inside the chain.  conv.2 is positive: a logit is finite or +inf, never inf - inf."""
    feat, sd, _ = case(28)
    feat = feat[:3].copy()
    rng = synth._rng(7300)
    border = np.ones((28, 28), bool)
    border[1:-1, 1:-1] = False
    n = int(border.sum()) * 3 * synth.C_FEAT
    ends = np.array([3e38, -3e38, F32_MIN_NORMAL, -F32_MIN_NORMAL, 2.0 ** -140, -2.0 ** -149, 2.0 ** -127, 1.0], np.float32)
    feat[:, border] = ends[rng.integers(0, ends.size, n)].reshape(3, -1, synth.C_FEAT)
    sd = dict(sd)
    w = sd["conv.0.weight"]
    sd["conv.0.weight"] = np.where(rng.random(w.shape) < 0.75, -np.abs(w), w).astype(np.float32)
    sd["conv.2.weight"] = np.abs(sd["conv.2.weight"]) + np.float32(1e-3)
    want = ora.selector_saliency(feat, sd)
    assert np.isfinite(want).all() and (want == 1.0).any() and ((want > 0) & (want < 1)).any()
    for order in ORDERS:
        assert_bits(run(T, hip, knob, feat, sd, order), want, f"range ends, {order}")
