"""GPU tests of the bf16 descriptor kernel with its LayerNorm-folded layers (n_blocks >= 1), and of the bf16 pipeline stage by stage.

bf16 roundings of the activations flip for real once a LayerNorm sits between two GEMMs, so these are tolerance tests - but the
tolerance is on STRUCTURE, and every bound is the same figure measured on the CPU by the reference alone (tests/bf16_bounds.py:
an fp32-accumulate emulation against the float64 checker, two orders, with a stated margin; pinned by tests/test_bf16_bounds.py).
One 64-row tile in eight wrong by 3e-3, or one wrong output column, moves a tile / column median from 1e-8 to 1e-3 and fails;
test_gpu_bf16_mode.py::test_gather_refine_bf16, which lets the kernel under test choose the rows it excludes, passes both.
"""
import numpy as np
import pytest

import bf16_bounds as B
import synth
from oracle import ora
from oracle.ora_bf16 import refine_bf16_ref, refine_error_structure, saliency_bf16_ref

pytestmark = pytest.mark.gpu


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_structure(desc, ref, case, what):
    """Every figure of refine_error_structure within its reference-alone bound; all figures printed before the first assertion."""
    fig = refine_error_structure(desc, ref)
    bounds = {k: B.bound(case, k) for k in fig}
    print(f"{what} {case}: " + ", ".join(f"{k} {fig[k]:.3g} (cpu {B.TABLE[case][k]:.3g}, bound {bounds[k]})" for k in fig))
    for k in fig:
        if bounds[k] is None:       # the per-tile share at depth 8: the four-tile share holds instead (bf16_bounds.py)
            continue
        assert fig[k] <= bounds[k], f"{what} {case}: {k} = {fig[k]:.4g} above {bounds[k]:.4g} (= {B.MARGIN[k]} x the CPU figure {B.TABLE[case][k]:.4g})"
    if case[3] <= 2:            # the bounds this mode has always been held to stay, where the new ones are not tighter
        assert fig["rows_hit"] < 0.15 and fig["max"] < 5e-3
    return fig


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: "G%d_K%d_x%d_depth%d" % c)
def test_refine_bf16_structure(T, hip, case):
    grid, K, frames, n_blocks = case
    feat, kp, x, sd = B.inputs(*case)
    packed = dev(T, hip.pack_refiner_bf16(ora.refiner_weight_list(sd, n_blocks), n_blocks))
    desc = hip.gather_refine_bf16(dev(T, feat), dev(T, kp), packed, n_blocks).cpu().numpy().reshape(-1, 128)
    desc2 = hip.refine_bf16(dev(T, x), packed, n_blocks).cpu().numpy()
    np.testing.assert_array_equal(bits(desc), bits(desc2))                    # fused gather == x_in entry
    ref = refine_bf16_ref(x, sd, n_blocks)
    assert_structure(desc, ref, case, "gather_refine_bf16")
    # model-level drift of the mode against the exact oracle
    cos = (desc.astype(np.float64) * ora.refine(x, sd, n_blocks)).sum(-1)
    assert cos.min() > B.COS_MIN, cos.min()
    assert np.abs(np.sqrt((desc.astype(np.float64) ** 2).sum(-1)) - 1).max() < B.NORM_TOL


@pytest.mark.parametrize("n_blocks", [1, 3, 8])
def test_exact_refine_other_depths(T, hip, n_blocks):
    """The exact kernel at the depths the ABI accepts besides 2 (the sharded runner ships n_blocks = 1 to its ranks): bit for bit."""
    feat, kp, x, sd = B.inputs(28, 192, 3, n_blocks)
    packed = dev(T, hip.pack_refiner(ora.refiner_weight_list(sd, n_blocks), n_blocks))
    desc = hip.gather_refine(dev(T, feat), dev(T, kp), packed, n_blocks).cpu().numpy().reshape(-1, 128)
    np.testing.assert_array_equal(bits(desc), bits(ora.refine(x, sd, n_blocks)))


# ---- rows where the folded LayerNorm is ill-conditioned --------------------------------------------------------------------
@pytest.mark.parametrize("kind", B.ILL_KINDS)
def test_refine_bf16_ill_conditioned_rows(T, hip, kind):
    """Activations set directly by input_proj.bias: an ordinary row, a constant row, an all-zero row, mean / std from 1 to 1e6 -
    next to rows of (almost) zero activations in the same tiles.  Every row: finite, unit norm, and the bits of the same row run
    alone.  Agreement with the float64 checker within the depth-2 maximum bound over the whole measured range (the CPU emulation
    stays within it up to mean / std = 1e6: the one-pass variance loses its bits, but the residual carries the row)."""
    x, sd, zero_row = B.ill_conditioned(kind)
    packed = dev(T, hip.pack_refiner_bf16(ora.refiner_weight_list(sd, 2), 2))
    desc = hip.refine_bf16(dev(T, x), packed, 2).cpu().numpy()
    assert np.isfinite(desc).all()
    assert np.abs(np.sqrt((desc.astype(np.float64) ** 2).sum(-1)) - 1).max() < 1e-5
    for rows_of_kind in (zero_row, ~zero_row):
        i = int(np.flatnonzero(rows_of_kind)[0])
        alone = hip.refine_bf16(dev(T, x[i:i + 1]), packed, 2).cpu().numpy()
        assert np.isfinite(alone).all()
        same = (bits(desc[rows_of_kind]) == bits(alone)).all(-1)
        assert same.all(), f"{kind}: rows {np.flatnonzero(rows_of_kind)[~same][:8].tolist()} differ from the same row run alone"
    ref = refine_bf16_ref(x, sd, 2)
    d = np.abs(desc.astype(np.float64) - ref).max(-1)
    exact = ora.refine(x, sd, 2)
    cos = (desc.astype(np.float64) * exact).sum(-1)
    print(f"{kind}: mean/std {B.ill_ratio(sd):.4g}: device - float64 checker max {d[zero_row].max():.3g} (near-zero rows {d[~zero_row].max():.3g}), "
          f"cos against the exact oracle {cos[zero_row].min():.6f} (near-zero rows {cos[~zero_row].min():.4f})")
    assert d.max() <= B.bound((28, 500, 3, 2), "max"), d.max()
    assert cos[zero_row].min() > B.COS_MIN


# ---- the bf16 pipeline, stage by stage --------------------------------------------------------------------------------------
def test_pipeline_bf16_stage_by_stage(T, hip):
    """SequencePipeline(precision='bf16').run: every stage against the oracle applied to the input that stage had ON THE DEVICE, so
    that nothing between the two bf16 kernels is taken on trust."""
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    n, K, grid = 4, 500, 28
    toks, imgs = synth.token_sequence(n, grid), synth.image_sequence(n)
    ssd, rsd = synth.selector_state(0), synth.refiner_state(0)
    cfg = ExtractorConfig(precision="bf16")
    out = SequencePipeline(cfg, ssd, rsd).run(dev(T, imgs), dev(T, toks))
    get = lambda k: out[k].cpu().numpy()
    feat = ora.bn_tokens(toks)[0].reshape(n, grid, grid, 384)
    # saliency: float64 checker of the oracle's BatchNorm output; bound = margin x the CPU emulation's own maximum
    sal = get("saliency")
    ref_sal = saliency_bf16_ref(feat, ssd)
    print("saliency: max |device - float64 checker| =", np.abs(sal - ref_sal).max())
    assert np.abs(sal - ref_sal).max() <= B.MARGIN["max"] * B.SALIENCY_MAX_CPU
    # selection: the oracle on the DEVICE's saliency, bit for bit
    kp, sc, idx, st = ora.select_keypoints(sal, K, cfg.nms_radius, cfg.min_score_percentile)
    np.testing.assert_array_equal(get("idx"), idx)
    np.testing.assert_array_equal(bits(get("keypoints_patch")), bits(kp))
    np.testing.assert_array_equal(bits(get("scores")), bits(sc))
    # descriptors: float64 checker of the oracle's gather at the device's keypoints, structured bounds of the depth-2 case
    # of the same shape (28 x 28 grid, 500 keypoints)
    x = ora.gather(feat, get("keypoints_patch")).reshape(-1, 384)
    desc = get("descriptors")
    fig = refine_error_structure(desc.reshape(-1, 128), refine_bf16_ref(x, rsd, 2))
    case = (28, 500, 3, 2)
    print("descriptors:", fig)
    for k in fig:
        assert B.bound(case, k) is not None and fig[k] <= B.bound(case, k), (k, fig[k], B.bound(case, k))
    # matches and quality: the oracle on the device's own descriptors, scores and intensities, bit for bit
    inten = get("intensity")
    total_matches = 0
    for p in range(n - 1):
        omt, oq = ora.match_with_quality(desc[p], desc[p + 1], sc[p], sc[p + 1], cfg.saliency_weight, cfg.min_saliency,
                                         cfg.min_descriptor_sim, inten[p], inten[p + 1], cfg.min_intensity)
        c = int(get("match_count")[p])
        assert c == len(omt), (p, c, len(omt))
        total_matches = total_matches + c
        np.testing.assert_array_equal(get("matches")[p, :c], omt)
        np.testing.assert_array_equal(bits(get("quality")[p, :c]), bits(oq))
    assert total_matches > 0, "no pair matched: the last stage compared nothing"
