"""Bounds of the bf16 descriptor kernel for n_blocks >= 1, taken from the reference side alone.

With LayerNorm-folded layers the activations are no longer order-free: an fp32 accumulator that differs from the float64 one
in its last bits can round to the other bf16 neighbour, and one such flip moves a unit descriptor by ~1e-3.  Flips are real
and cannot be excluded row by row, so the tests look at STRUCTURE (oracle/ora_bf16.py: refine_error_structure) and bound each
figure by the same figure of a CPU emulation that accumulates in fp32 (refine_bf16_f32acc, two summation orders, the worse
kept) against the float64 checker on the same inputs.  No figure here comes from a GPU.

TABLE holds the CPU figures as measured; tests/test_bf16_bounds.py recomputes them and fails if the table has drifted from
what the reference gives.  tests/test_gpu_bf16_structure.py asserts  device figure <= MARGIN x table figure:
  * x4 on the medians: they sit at a few fp32 ulps of a unit descriptor's elements (1e-8); x4 stays five orders of magnitude
    below the 1e-3 of one flip, so a tile, column or wave slab that is wrong by more than rounding cannot hide;
  * x3 on the hit shares and the maximum: counts of rare events (tens of rows in 500..2000; one tile has 64), and the device's
    order is a third one.  A share bound above TILE_SHARE_CAP would stop seeing a wrong tile, so none is used: at depth 8 the
    worst 64-row tile of the reference alone has 0.36 of its rows flipped and x3 is past 1, so there the per-tile share is not
    asserted (bound() gives None) and the share over MORE ROWS holds instead - the worst group of four consecutive tiles
    (256 rows; reference 0.24-0.29, bound 0.73-0.86).  The four-tile share is asserted at every depth.  Said plainly: at depth 8
    ONLY THE TILE MEDIAN guards a single tile - one tile with every row flipped inside an otherwise clean group of four gives
    0.25 over the 256 rows, below the bound; its median, at 1e-3 against a bound of 4e-8, cannot pass.
"""
from __future__ import annotations

import numpy as np

import synth
from oracle import ora
from oracle.ora_bf16 import refine_bf16_f32acc, refine_bf16_ref, refine_error_structure

MARGIN = {"tile_median": 4.0, "column_median": 4.0, "slab_median": 4.0, "rows_hit": 3.0, "tile_rows_hit": 3.0, "tile4_rows_hit": 3.0, "max": 3.0}
TILE_SHARE_CAP = 0.9
COS_MIN, NORM_TOL = 0.999, 1e-5          # model-level drift against the exact oracle (unchanged)

# (grid, K, frames, n_blocks): rows -> 64-row tiles: 1500 -> 24 (ragged), 500 -> 8 (ragged), 576 -> 9, 832 -> 13, 1024 -> 16,
# 1984 -> 31
CASES = [(28, 500, 3, 1), (28, 500, 3, 2), (28, 500, 3, 3), (28, 500, 3, 8), (28, 500, 1, 2), (28, 192, 3, 2), (40, 416, 2, 2),
         (40, 1024, 1, 2), (40, 992, 2, 2), (40, 992, 2, 8)]

# CPU figures (worse of the two emulated orders), written by `python tests/bf16_bounds.py`
TABLE = {
    (28, 500, 3, 1): {"tile_median": 3.73e-09, "column_median": 7.45e-09, "slab_median": 3.73e-09, "rows_hit": 0.0173, "tile_rows_hit": 0.0714, "tile4_rows_hit": 0.0273, "max": 0.000786, "cos_min_ref": 0.99997},
    (28, 500, 3, 2): {"tile_median": 3.73e-09, "column_median": 1.49e-08, "slab_median": 3.73e-09, "rows_hit": 0.0407, "tile_rows_hit": 0.109, "tile4_rows_hit": 0.0625, "max": 0.00114, "cos_min_ref": 0.99996},
    (28, 500, 3, 3): {"tile_median": 5.47e-09, "column_median": 1.49e-08, "slab_median": 3.73e-09, "rows_hit": 0.0613, "tile_rows_hit": 0.125, "tile4_rows_hit": 0.0977, "max": 0.00139, "cos_min_ref": 0.99993},
    (28, 500, 3, 8): {"tile_median": 9.31e-09, "column_median": 1.49e-08, "slab_median": 7.45e-09, "rows_hit": 0.209, "tile_rows_hit": 0.359, "tile4_rows_hit": 0.242, "max": 0.00281, "cos_min_ref": 0.99978},
    (28, 500, 1, 2): {"tile_median": 3.73e-09, "column_median": 1.49e-08, "slab_median": 3.73e-09, "rows_hit": 0.046, "tile_rows_hit": 0.109, "tile4_rows_hit": 0.0625, "max": 0.00114, "cos_min_ref": 0.99996},
    (28, 192, 3, 2): {"tile_median": 3.73e-09, "column_median": 1.49e-08, "slab_median": 3.73e-09, "rows_hit": 0.0503, "tile_rows_hit": 0.109, "tile4_rows_hit": 0.0664, "max": 0.000931, "cos_min_ref": 0.99996},
    (40, 416, 2, 2): {"tile_median": 3.73e-09, "column_median": 1.49e-08, "slab_median": 3.73e-09, "rows_hit": 0.0361, "tile_rows_hit": 0.0781, "tile4_rows_hit": 0.0469, "max": 0.000953, "cos_min_ref": 0.99995},
    (40, 1024, 1, 2): {"tile_median": 3.73e-09, "column_median": 1.49e-08, "slab_median": 3.73e-09, "rows_hit": 0.0352, "tile_rows_hit": 0.0625, "tile4_rows_hit": 0.0469, "max": 0.000953, "cos_min_ref": 0.99996},
    (40, 992, 2, 2): {"tile_median": 3.73e-09, "column_median": 1.49e-08, "slab_median": 3.73e-09, "rows_hit": 0.0353, "tile_rows_hit": 0.0938, "tile4_rows_hit": 0.0469, "max": 0.00109, "cos_min_ref": 0.99995},
    (40, 992, 2, 8): {"tile_median": 7.45e-09, "column_median": 1.49e-08, "slab_median": 7.45e-09, "rows_hit": 0.2, "tile_rows_hit": 0.344, "tile4_rows_hit": 0.285, "max": 0.00259, "cos_min_ref": 0.99978},
}


# saliency of the pipeline test's four frames (synth.token_sequence(4, 28), synthetic weights): largest difference of the
# fp32-accumulate emulation (saliency_bf16_f32acc, worse of its two orders) from the float64 checker; margin as for "max"
SALIENCY_MAX_CPU = 6.3e-07


def saliency_reference_max(n=4, grid=28):
    from oracle.ora_bf16 import saliency_bf16_f32acc, saliency_bf16_ref
    feat = ora.bn_tokens(synth.token_sequence(n, grid))[0].reshape(n, grid, grid, 384)
    sd = synth.selector_state(0)
    ref = saliency_bf16_ref(feat, sd)
    return max(float(np.abs(saliency_bf16_f32acc(feat, sd, order) - ref).max()) for order in (0, 1))


def inputs(grid, K, frames, n_blocks):
    """Synthetic weights and the natural keypoints of the grid -> (feat, keypoints, gathered rows x, refiner state dict)."""
    sd = synth.refiner_state(0, n_blocks=n_blocks)
    feat = ora.bn_tokens(synth.tokens(30 + grid, grid, frames))[0].reshape(frames, grid, grid, 384)
    kp = ora.select_keypoints(ora.selector_saliency(feat, synth.selector_state(0)), K)[0]
    return feat, kp, ora.gather(feat, kp).reshape(-1, 384), sd


def reference_figures(grid, K, frames, n_blocks):
    """-> (figures: the worse of the two emulated orders per statistic; min cosine of the float64 checker against the exact oracle)."""
    _, _, x, sd = inputs(grid, K, frames, n_blocks)
    ref = refine_bf16_ref(x, sd, n_blocks)
    per_order = [refine_error_structure(refine_bf16_f32acc(x, sd, n_blocks, order), ref) for order in (0, 1)]
    cos = float((ref.astype(np.float64) * ora.refine(x, sd, n_blocks)).sum(-1).min())
    return {k: max(p[k] for p in per_order) for k in per_order[0]}, cos


def bound(case, stat):
    """MARGIN x the CPU figure; None where a share bound would exceed TILE_SHARE_CAP (the per-tile share at depth 8): such a
    figure is not asserted, and the four-tile share - never None, see test_bf16_bounds.py - holds in its place."""
    b = MARGIN[stat] * TABLE[case][stat]
    return None if stat.endswith("rows_hit") and b > TILE_SHARE_CAP else b


# ---- rows on which the folded LayerNorm is ill-conditioned ------------------------------------------------------------
# The kernel takes the variance in one fp32 pass, q / 384 - mean^2, where the exact oracle takes two: the subtraction cancels
# log2(ratio^2) bits, ratio = mean / std of the 384 activations.  The rows are made by the weights: input_proj.weight is zero but
# for column 0, and input_proj.bias is the wanted activation pattern - an all-zero input row feeds ReLU(bias) to the first
# LayerNorm whatever else is in the launch; column 0 holds -bias, so the input row e_0 feeds (almost) zeros: two kinds of rows
# with very different statistics side by side in one tile.
ILL_RATIOS = [1, 3, 10, 30, 100, 300, 1000, 3000, 10000, 30000, 100000, 1000000]
ILL_KINDS = ["ordinary", "constant", "all_zero"] + [f"ratio_{r}" for r in ILL_RATIOS]


def ill_conditioned(kind, n_blocks=2, rows=150):
    """-> (x (rows, 384): a shuffled mix of all-zero rows and e_0 rows, state dict, mask of the all-zero rows)."""
    sd = dict(synth.refiner_state(0, n_blocks=n_blocks))
    rng = np.random.Generator(np.random.PCG64(97_000))
    ordinary = (rng.random(384) * 2 - 1) * 0.1
    noise = rng.standard_normal(384)
    noise = (noise - noise.mean()) / noise.std()
    if kind == "ordinary":
        bias = ordinary
    elif kind == "constant":
        bias = np.full(384, 3.0)
    elif kind == "all_zero":
        bias = -1.0 - np.abs(ordinary)
    else:
        bias = float(kind.split("_")[1]) + noise
    bias = bias.astype(np.float32)
    W = np.zeros((384, 384), np.float32)
    W[:, 0] = -bias
    sd["input_proj.weight"], sd["input_proj.bias"] = W, bias
    zero_row = rng.random(rows) < 0.5
    zero_row[:2] = [True, False]
    x = np.zeros((rows, 384), np.float32)
    x[~zero_row, 0] = 1.0
    return x, sd, zero_row


def ill_ratio(sd):
    """mean / std (float64) of ReLU(bias): what an all-zero input row feeds to the first LayerNorm."""
    X = np.maximum(sd["input_proj.bias"].astype(np.float64), 0)
    return float(X.mean() / X.std()) if X.std() > 0 else float("inf")


# CPU figures of the rows above at depth 2, written by `python tests/bf16_bounds.py` and pinned by tests/test_bf16_bounds.py:
# kind -> (mean / std of the activations; largest |fp32-accumulate emulation - float64 checker| over the ill-conditioned rows,
# worse of the two orders; the same over the near-zero rows; smallest cosine of the float64 checker against the exact oracle
# over the ill-conditioned rows)
ILL_TABLE = {
    "ordinary": (0.7326, 4.47e-08, 4.47e-08, 0.999982),
    "constant": (float("inf"), 0.000509, 4.47e-08, 0.999994),
    "all_zero": (float("inf"), 4.47e-08, 2.98e-08, 0.999987),
    "ratio_1": (1.23, 4.47e-08, 2.98e-08, 0.999989),
    "ratio_3": (3, 2.98e-08, 4.47e-08, 0.999993),
    "ratio_10": (10, 4.47e-08, 4.47e-08, 0.999992),
    "ratio_30": (30, 2.98e-08, 4.47e-08, 0.999995),
    "ratio_100": (100, 0.000251, 4.47e-08, 0.999994),
    "ratio_300": (300, 0.000334, 2.98e-08, 0.999992),
    "ratio_1000": (1000, 6.04e-05, 4.47e-08, 0.999997),
    "ratio_3000": (3000, 2.98e-08, 2.98e-08, 0.999995),
    "ratio_10000": (1e+04, 2.98e-08, 5.66e-05, 0.999998),
    "ratio_30000": (3e+04, 2.98e-08, 0.000279, 0.999998),
    "ratio_100000": (1e+05, 5.96e-08, 0.000231, 0.999998),
    "ratio_1000000": (9.993e+05, 2.98e-08, 2.98e-08, 0.999998),
}
ILL_ONE_FLIP = 2 * 5.09e-4      # twice the largest figure above: no row of any kind is further from the checker than one flip


def ill_reference_figures(kind):
    x, sd, zero_row = ill_conditioned(kind)
    ref = refine_bf16_ref(x, sd, 2)
    d = np.maximum(*(np.abs(refine_bf16_f32acc(x, sd, 2, order).astype(np.float64) - ref).max(-1) for order in (0, 1)))
    cos = (ref.astype(np.float64) * ora.refine(x, sd, 2)).sum(-1)
    return ill_ratio(sd), float(d[zero_row].max()), float(d[~zero_row].max()), float(cos[zero_row].min())


if __name__ == "__main__":
    for case in CASES:
        fig, cos = reference_figures(*case)
        print(f"    {case}: {{" + ", ".join(f'"{k}": {v:.3g}' for k, v in fig.items()) + f', "cos_min_ref": {cos:.5f}}},', flush=True)
    for kind in ILL_KINDS:
        r, d_ill, d_zero, cos = ill_reference_figures(kind)
        print(f'    "{kind}": ({r:.4g}, {d_ill:.3g}, {d_zero:.3g}, {cos:.6f}),', flush=True)
