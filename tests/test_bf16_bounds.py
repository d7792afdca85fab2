"""CPU tests of the reference-alone bounds of the bf16 descriptor kernel (tests/bf16_bounds.py): no GPU involved.

  * the fp32-accumulate checker (oracle/ora_bf16.py: refine_bf16_f32acc, two orders) against the float64 checker on the same
    inputs: equal up to fp32 ulps except where a bf16 rounding flips;
  * the table the GPU test imports holds what the reference gives today, and the bounds it yields are no looser at depth 2 than
    the ones test_gpu_bf16_mode.py has always asserted (rows_hit < 0.15, max < 5e-3).
"""
import numpy as np
import pytest

import bf16_bounds as B
from oracle import ora
from oracle.ora_bf16 import refine_bf16_f32acc, refine_bf16_ref, refine_error_structure


@pytest.mark.parametrize("n_blocks", [0, 1, 2])
def test_f32_accumulate_checker_tracks_the_float64_checker(n_blocks):
    _, _, x, sd = B.inputs(28, 200, 2, n_blocks)
    ref = refine_bf16_ref(x, sd, n_blocks)
    a, b = (refine_bf16_f32acc(x, sd, n_blocks, order) for order in (0, 1))
    assert a.dtype == np.float32 and not np.array_equal(a, b), "the two orders must really differ"
    for got in (a, b):
        s = refine_error_structure(got, ref)
        print(n_blocks, s)
        assert np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(-1)) - 1).max() < 1e-6
        # most rows see no flip: there the two checkers agree to a few ulps of a unit descriptor's elements
        assert s["tile_median"] < 3e-8 and s["column_median"] < 6e-8 and s["slab_median"] < 3e-8
        if n_blocks == 0:
            # hidden activations straddle no LayerNorm: flips are rarer still, and each costs less
            assert s["rows_hit"] < 0.05 and s["max"] < 2e-3
        else:
            assert s["rows_hit"] < 0.15 and s["max"] < 5e-3


def test_order_free_inputs_need_no_tolerance_in_either_order():
    import orderfree
    _, _, sd, x, _, desc, _ = orderfree.refiner_case(3, 17, 2, 150)
    for order in (0, 1):
        np.testing.assert_array_equal(refine_bf16_f32acc(x, sd, 0, order).view(np.uint32), desc.view(np.uint32))


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: "G%d_K%d_x%d_depth%d" % c)
def test_table_is_what_the_reference_gives(case):
    fig, cos = B.reference_figures(*case)
    tab = B.TABLE[case]
    print(case, fig, cos)
    for k in ("tile_median", "column_median", "slab_median"):
        # medians are quantised to half ulps of the descriptor elements: the table may not be above the next step
        assert fig[k] <= tab[k] * 1.01 and tab[k] <= fig[k] * 2.01, (k, fig[k], tab[k])
    for k, slack in (("rows_hit", 0.005), ("tile_rows_hit", 2.0 / 64), ("tile4_rows_hit", 4.0 / 256)):
        # one row is 1 / rows of the overall share, 1 / 64 of a tile's and 1 / 256 of four tiles': a last-bit difference
        # between two hosts' float64 dot products may move a flip
        assert abs(fig[k] - tab[k]) <= slack, (k, fig[k], tab[k])
    assert abs(fig["max"] - tab["max"]) <= 0.1 * tab["max"], (fig["max"], tab["max"])
    assert abs(cos - tab["cos_min_ref"]) < 2e-5 and cos > B.COS_MIN


def test_bounds_are_no_looser_than_the_old_ones_and_cannot_hide_a_tile():
    for case in B.CASES:
        depth = case[3]
        # no share bound above the cap: the per-tile share is asserted up to depth 3 and left out at depth 8 (x3 is past 1),
        # where the share over four tiles - asserted in every case - holds
        assert (B.bound(case, "tile_rows_hit") is None) == (depth == 8)
        assert B.bound(case, "tile4_rows_hit") is not None and B.bound(case, "rows_hit") is not None
        assert all(b is None or b <= B.TILE_SHARE_CAP for b in (B.bound(case, k) for k in ("tile_rows_hit", "tile4_rows_hit", "rows_hit")))
        # a tile, column or wave slab wrong by 1e-5 of a unit descriptor's element (a hundredth of one flip) must show
        assert max(B.bound(case, k) for k in ("tile_median", "column_median", "slab_median")) < 1e-6
        if depth <= 2:          # (the GPU test keeps the old rows_hit < 0.15 as well where 3 x the CPU share comes out at 0.151)
            assert B.bound(case, "max") < 5e-3, case
    # at the shape of the old test the new bounds are the tighter ones
    assert B.bound((28, 500, 3, 2), "rows_hit") < 0.15 and B.bound((28, 500, 3, 2), "max") < 5e-3
    # every depth the issue names, and the tile counts 8, 9, 13, 24 and 31
    assert {c[3] for c in B.CASES} == {1, 2, 3, 8}
    assert {(c[1] * c[2] + 63) // 64 for c in B.CASES} >= {8, 9, 13, 24, 31}


def test_saliency_bound_is_what_the_reference_gives():
    m = B.saliency_reference_max()
    print("saliency: fp32-accumulate emulation against the float64 checker, max", m)
    assert abs(m - B.SALIENCY_MAX_CPU) <= 0.15 * B.SALIENCY_MAX_CPU
    # two hundred times below the 2e-4 the saliency has been held to so far: one wrong operand of 3456 moves it by about that
    assert B.MARGIN["max"] * B.SALIENCY_MAX_CPU < 2e-6



@pytest.mark.parametrize("kind", B.ILL_KINDS)
def test_ill_conditioned_rows_on_the_reference_alone(kind):
    """The CPU column of DESIGN.md's operating range of the folded LayerNorm: the fp32-accumulate emulation (one-pass variance,
    like the kernel) against the float64 checker, and the checker against the exact oracle, on the rows that
    tests/test_gpu_bf16_structure.py::test_refine_bf16_ill_conditioned_rows sends to the device."""
    ratio, d_ill, d_zero, cos = B.ill_reference_figures(kind)
    t_ratio, _, _, t_cos = B.ILL_TABLE[kind]
    print(f"{kind}: mean/std {ratio:.4g}, emulation - checker {d_ill:.3g} (near-zero rows {d_zero:.3g}), checker . oracle {cos:.6f}")
    assert ratio == t_ratio or abs(ratio - t_ratio) <= 1e-3 * t_ratio
    # a flip may move between two hosts' dot products, so the differences are held to one flip, not to the table's digits
    assert max(d_ill, d_zero) <= B.ILL_ONE_FLIP < B.bound((28, 500, 3, 2), "max")
    assert abs(cos - t_cos) < 2e-5 and cos > B.COS_MIN


def test_structure_bounds_see_one_scaled_tile_that_the_old_bounds_pass():
    """Emulated faults (CPU; the fp32-accumulate emulation stands in for the kernel): the rows of ONE 64-row tile scaled by 1.002
    (a) where the descriptors are stored, after the normalisation, and (b) at the ReLU output of input_proj, before the tile is
    written as bf16 - there the final normalisation and the LayerNorms cancel the scale itself and only the moved bf16 roundings
    remain.  The bounds test_gpu_bf16_mode.py::test_gather_refine_bf16 has always asserted (median < 1e-7, rows_hit < 0.15,
    max < 5e-3, cos > 0.999) pass both - (a) is caught there by |norm - 1| < 1e-5 alone, (b) by nothing; the structured bounds
    fail the tile median, the per-tile share and the four-tile share of both."""
    case = (28, 500, 3, 2)
    _, _, x, sd = B.inputs(*case)
    ref, exact = refine_bf16_ref(x, sd, 2), ora.refine(x, sd, 2)
    tile = slice(192, 256)

    def scale_tile(X):
        X = X.copy()
        X[tile] *= np.float32(1.002)
        return X
    clean = refine_bf16_f32acc(x, sd, 2)
    stored = clean.copy()
    stored[tile] *= np.float32(1.002)
    hidden = refine_bf16_f32acc(x, sd, 2, after_input_proj=scale_tile)
    for name, desc in (("clean", clean), ("stored", stored), ("hidden", hidden)):
        d = np.abs(desc - ref)
        old_ok = np.median(d) < 1e-7 and np.mean(d.max(-1) > 1e-5) < 0.15 and d.max() < 5e-3 and (desc * exact).sum(-1).min() > 0.999
        norm_ok = np.abs(np.sqrt((desc.astype(np.float64) ** 2).sum(-1)) - 1).max() < 1e-5
        fig = refine_error_structure(desc, ref)
        failed = {k for k in fig if B.bound(case, k) is not None and fig[k] > B.bound(case, k)}
        print(name, old_ok, norm_ok, fig, failed)
        assert old_ok, name
        assert norm_ok == (name != "stored")
        assert failed == (set() if name == "clean" else {"tile_median", "tile_rows_hit", "tile4_rows_hit"}), (name, failed)

