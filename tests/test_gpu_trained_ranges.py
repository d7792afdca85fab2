"""The fp32 "exact" path outside the band of the default synthetic weights, BIT FOR BIT against the CPU oracle (which
tests/test_stress_inputs.py holds to float64 and to the reference's own modules on the same inputs, tests/stress_cases.py):

* the sigmoid epilogue of every selector form over the whole logit range: the clamp at -87 / 88, the scale factor 2^n at both
  ends, the subnormal saliency floor, the exact 1.0f;
* saturated saliency maps of steep selectors, and select_keypoints on their plateaus of exactly 1.0f;
* the fp32 selector at G = 61 .. 64;
* the descriptor MLP at 0, 1, 3 and 8 residual blocks (2 as control) and in every arm of its two square roots;
* BatchNorm one past each launch-form boundary, in eval mode, with other prefixes and eps, on constant / ill-conditioned / tiny
  channels;
* one end-to-end pass with a saturated selector and a three-block refiner.

Run on the GPU box: python -m pytest tests/test_gpu_trained_ranges.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import stress_cases as sc
import synth
from oracle import ora

pytestmark = pytest.mark.gpu

FORMS = ["latency2", "latency", "throughput", "throughput_tail", "throughput_stage"]
F32_MIN_NORMAL = np.float32(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def hip(T):
    from sslam_amd import lib
    lib.lib()          # raises if libsslam_hip.so is not built: no fallback
    return lib


def dev(T, a):
    a = np.ascontiguousarray(a)
    return T.from_numpy(a if a.flags.writeable else a.copy()).cuda()      # the shared oracle results are read-only


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.nonzero(bits(got).ravel() != bits(want).ravel())[0]
        raise AssertionError(f"{what}: {bad.size}/{got.size} elements differ; first at {bad[0]}: "
                             f"{got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}; "
                             f"max abs diff {np.abs(got.astype(np.float64) - want.astype(np.float64)).max():.3e}")


def set_form(knob, form):
    """The selector-form knobs of test_selector_saliency; None: the library's own choice."""
    if form is None:
        return
    knob("SSLAM_CONV_LATENCY_ROWS", "0" if form.startswith("throughput") else str(1 << 30))
    knob("SSLAM_CONV_LAT2_ROWS", str(1 << 30) if form == "latency2" else "0")
    if form == "throughput_stage":
        knob("SSLAM_CONV_NO_HALO", "1")
    if form == "throughput_tail":
        knob("SSLAM_CONV_TAIL", "4")


def saliency(T, hip, feat, sd):
    w1p = dev(T, hip.pack_conv3x3(sd["conv.0.weight"]))
    return hip.selector_saliency(dev(T, feat), w1p, dev(T, sd["conv.0.bias"]), dev(T, sd["conv.2.weight"].reshape(-1)),
                                 dev(T, sd["conv.2.bias"]), sd["conv.0.weight"].shape[0]).cpu().numpy()


# ---------------------------------------------------------------------------------- oracle results, computed once and shared
@functools.lru_cache(maxsize=None)
def features(grid, frames):
    f = ora.bn_tokens(synth.tokens(48, grid, frames))[0].reshape(frames, grid, grid, 384)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def steep_map(seed, hidden, scale, grid, frames):
    m = ora.selector_saliency(features(grid, frames), sc.steep_selector(seed, hidden, scale))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def default_map(grid, frames):
    m = ora.selector_saliency(features(grid, frames), synth.selector_state(0))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def passthrough_case(grid, frames):
    l = sc.logit_list(frames * grid * grid, grid)
    want = np.array([ora.sigmoid(v) for v in l], np.float32).reshape(frames, grid, grid)
    want.setflags(write=False)
    return sc.passthrough_feat(l, grid, frames), want


@functools.lru_cache(maxsize=None)
def refined(depth, variant, rows):
    out = ora.refine(sc.refiner_rows(rows), sc.refiner_variants(depth)[variant], depth)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------ sigmoid range
@pytest.mark.parametrize("grid,frames", [(7, 2), (28, 1)])
@pytest.mark.parametrize("hidden,form", [(256, f) for f in FORMS] + [(128, None), (128, "throughput")])
def test_sigmoid_range_in_every_epilogue(T, hip, knob, hidden, form, grid, frames):
    """The logit of every cell is a chosen number (pass-through selector): device bits equal the oracle's sigmoid of it, the
    subnormal floor below -88 and the exact 1.0f included.  98 cells: a tile tail and a frame boundary inside a tile."""
    set_form(knob, form)
    feat, want = passthrough_case(grid, frames)
    # the fixed points alone: 88, its upper neighbour, 103.97 and both sides of the n = 127 tie give 1.0f; -88, both its
    # neighbours and -103.97 give subnormals, three of them the floor
    assert (want == 1.0).sum() >= 5 and ((want > 0) & (want < F32_MIN_NORMAL)).sum() >= 4
    assert (bits(want) == bits(ora.sigmoid(-88.0))).sum() >= 3
    got = saliency(T, hip, feat, sc.passthrough_selector(hidden))
    assert_bits(got, want, "sigmoid of the chosen logits")
    assert_bits(got, ora.selector_saliency(feat, sc.passthrough_selector(hidden)), "saliency")


# --------------------------------------------------------------------------------------------------------- steep maps
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("grid,frames", [(28, 3), (44, 3)])
@pytest.mark.parametrize("scale", [60, 200])
def test_steep_selector_maps(T, hip, knob, scale, grid, frames, form):
    set_form(knob, form)
    want = steep_map(0, 256, scale, grid, frames)
    assert (want == 1.0).any() and (want < 0.05).any()
    assert_bits(saliency(T, hip, features(grid, frames), sc.steep_selector(0, 256, scale)), want, "saliency")


@pytest.mark.parametrize("seed,hidden,scale,grid,frames", [(0, 256, 60, 64, 1), (0, 256, 200, 64, 1), (1, 128, 200, 28, 2)])
def test_steep_selector_maps_default_form(T, hip, seed, hidden, scale, grid, frames):
    want = steep_map(seed, hidden, scale, grid, frames)
    assert_bits(saliency(T, hip, features(grid, frames), sc.steep_selector(seed, hidden, scale)), want, "saliency")


def check_select(T, hip, sal, K, radius, pct, tag, every_frame=True):
    kp, sco, idx, px, st = (t.cpu().numpy() for t in hip.select_keypoints(dev(T, sal), K, radius, pct))
    okp, osc, oidx, ost = ora.select_keypoints(sal, K, radius, pct)
    assert np.array_equal(st, ost), tag
    ok = np.ones_like(ost, bool) if every_frame else ost == 0
    assert np.array_equal(idx[ok], oidx[ok]), tag
    assert np.array_equal(bits(kp[ok]), bits(okp[ok])), tag
    assert np.array_equal(bits(sco[ok]), bits(osc[ok])), tag
    assert np.array_equal(bits(px[ok]), bits(ora.patch_to_pixel(okp[ok]))), tag
    return oidx, ost


@pytest.mark.parametrize("grid,frames", [(28, 3), (44, 3), (64, 1)])
@pytest.mark.parametrize("scale", [60, 200])
def test_select_on_steep_maps(T, hip, scale, grid, frames):
    """Hundreds of cells at exactly 1.0f: plateaus for the NMS, ties for the order (value descending, index ascending) and for
    the percentile, and a pad that repeats cells.  The oracle's canonical order is the line to hold."""
    sal = np.array(steep_map(0, 256, scale, grid, frames))
    repeats = 0
    for K, radius, pct in [(500, 2, 0.5), (500, 0, 0.9), (500, 3, 0.1)] + ([(4096, 2, 0.5)] if grid == 64 else []):
        oidx, ost = check_select(T, hip, sal, K, radius, pct, (scale, grid, K, radius, pct))
        repeats += sum(np.unique(i).size < K for i in oidx)
    if grid != 44:                # K = 500 of 784 cells, K = 4096 of 4096: the pad repeats cells (at G = 44 the survivors suffice)
        assert repeats > 0


@pytest.mark.parametrize("seed", range(3))
def test_fuzz_select_on_saturated_maps(T, hip, seed):
    """Maps that are the oracle's sigmoid of logits 120 u^3, u uniform in [-1, 1]: exact 1.0f plateaus, the subnormal floor and
    everything between, at random grids / K / radius / percentile (a stream of its own, drawn as test_fuzz_select_keypoints
    draws)."""
    rng = np.random.Generator(np.random.PCG64(8642 + seed))
    for case in range(6):
        g = int(rng.integers(3, 65))
        frames = int(rng.integers(1, 5))
        K = int(rng.integers(1, min(g * g, 4096) + 1))
        radius = int(rng.integers(0, 5))
        pct = float(rng.choice([0.0, 0.1, 0.5, 0.73, 0.9, 1.0]))
        u = rng.random((frames, g, g)) * 2.0 - 1.0
        logits = (120.0 * u ** 3).astype(np.float32)
        sal = np.array([ora.sigmoid(v) for v in logits.ravel()], np.float32).reshape(frames, g, g)
        check_select(T, hip, sal, K, radius, pct, (seed, case, g, frames, K, radius, pct), every_frame=False)


# ------------------------------------------------------------------------------------------- the selector beyond G = 60
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("grid,frames", [(61, 2), (64, 1), (64, 2)])
def test_selector_saliency_up_to_grid_64(T, hip, knob, grid, frames, form):
    set_form(knob, form)
    assert_bits(saliency(T, hip, features(grid, frames), synth.selector_state(0)), default_map(grid, frames), "saliency")


# ------------------------------------------------------------------------------------------------------ refiner depth
def packed_refiner(T, hip, sd, depth):
    return dev(T, hip.pack_refiner(ora.refiner_weight_list(sd, depth), depth))


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 8])
def test_refine_at_every_depth(T, hip, depth):
    """Row counts around the 32-row tile and beyond one; the stress rows (zero, -0, subnormal, 2^40, 2^60, a repeated row)."""
    packed = packed_refiner(T, hip, sc.refiner_variants(depth)["plain"], depth)
    for rows in (1, 31, 32, 33, 70, 257):
        got = hip.refine(dev(T, sc.refiner_rows(rows)), packed, depth).cpu().numpy()
        assert_bits(got, refined(depth, "plain", rows), f"refine, depth {depth}, {rows} rows")


@pytest.mark.parametrize("variant", ["dead", "zero_out", "bias_1e-30", "bias_1e-20", "bias_3e19"])
@pytest.mark.parametrize("depth", [1, 8])
def test_refine_in_every_arm(T, hip, depth, variant):
    """Dead hidden rows (LayerNorm of a constant row: 1/sqrtf(0 + 1e-5f)), a zero-norm output, norms below the 1e-12 floor
    (squares that underflow to 0, subnormal squares) and a sum of squares that overflows to +inf."""
    sd = sc.refiner_variants(depth)[variant]
    got = hip.refine(dev(T, sc.refiner_rows(70)), packed_refiner(T, hip, sd, depth), depth).cpu().numpy()
    assert np.isfinite(got).all()
    assert_bits(got, refined(depth, variant, 70), f"refine, depth {depth}, {variant}")


def fuzz_keypoints(rng, frames, K, g):
    kp = (rng.random((frames, K, 2)) * (g + 3) - 2).astype(np.float32)        # [-2, g+1): some taps fall outside
    kp[:, ::7] = np.floor(kp[:, ::7])                                           # integer coordinates
    kp[:, 5] = kp[:, 3]                                                         # a repeated keypoint
    return kp


@pytest.mark.parametrize("distinct", [0, 1])
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 8])
def test_gather_refine_at_every_depth(T, hip, knob, depth, distinct):
    """The fused launch (direct and distinct-row work list) at every depth, and proof that the comparison sees every block:
    one changed element of the packed weights - in the last block's fc2, in block 1's norm1.bias, output_proj.bias[127] - and
    the device output no longer equals the oracle's."""
    knob("SSLAM_REFINE_DISTINCT", distinct)
    g, K, frames = 7, 37, 2
    rng = np.random.Generator(np.random.PCG64(531 + depth))
    feat = rng.standard_normal((frames, g, g, 384)).astype(np.float32)
    kp = fuzz_keypoints(rng, frames, K, g)
    sd = synth.refiner_state(3, n_blocks=depth)
    want = ora.refine(ora.gather(feat, kp), sd, depth)
    host = hip.pack_refiner(ora.refiner_weight_list(sd, depth), depth)
    got = hip.gather_refine(dev(T, feat), dev(T, kp), dev(T, host), depth).cpu().numpy()
    assert_bits(got, want, f"descriptors, depth {depth}")
    lay = hip.refiner_layout(depth)
    assert lay.n_blocks == depth and lay.total == host.size
    spots = {"output_proj.bias[127]": lay.out_b + 127}
    if depth >= 1:
        spots["last fc2 weight"] = lay.blk[depth - 1][6] + 384 * 200 + 77
    if depth >= 2:
        spots["norm1.bias of block 1"] = lay.blk[1][1] + 300
    for what, at in spots.items():
        mutated = host.copy()
        mutated[at] += np.float32(0.5)
        out = hip.gather_refine(dev(T, feat), dev(T, kp), dev(T, mutated), depth).cpu().numpy()
        assert np.isfinite(out).all() and not np.array_equal(bits(out), bits(want)), (depth, what)


# --------------------------------------------------------------------------------------------------------- batch norm
def check_bn(T, hip, tok, n_prefix, group, train, eps, seed, what):
    gamma, beta, rmean, rvar = sc.bn_affine(seed)
    y, mean, var = hip.bn_tokens(dev(T, tok), n_prefix, group, dev(T, gamma), dev(T, beta), dev(T, rmean), dev(T, rvar), train, eps)
    oy, omean, ovar = ora.bn_tokens(tok, n_prefix, group, gamma, beta, rmean, rvar, train, eps)
    assert np.isfinite(oy).all()
    assert_bits(y.cpu().numpy(), oy, f"bn output, {what}")
    if train:
        assert_bits(mean.cpu().numpy(), omean, f"batch mean, {what}")
        assert_bits(var.cpu().numpy(), ovar, f"batch var, {what}")
        assert not bits(ovar[:, 0]).any()                     # the constant channel: variance exactly 0


@pytest.mark.parametrize("cells", [29 * 29, 41 * 41, 61 * 61, 64 * 64, 785, 1601, 3601])
def test_bn_train_past_every_form_boundary(T, hip, cells):
    """Per-frame statistics: the register-resident kernel switches form at 784, 1 600 and 3 600 cells; beyond, the three-sweep
    kernel runs."""
    check_bn(T, hip, sc.bn_tokens_case(cells, 2, 5, cells), 5, 1, True, 1e-5, cells, f"{cells} cells")


@pytest.mark.parametrize("grid", [29, 64])
def test_bn_train_three_sweep_kernel_forced(T, hip, knob, grid):
    knob("SSLAM_BN_FORM", 1)
    check_bn(T, hip, sc.bn_tokens_case(grid * grid, 2, 5, grid * grid), 5, 1, True, 1e-5, grid, f"three sweeps, G = {grid}")


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("grid", [7, 29, 41, 64])
def test_bn_eval(T, hip, grid, group):
    check_bn(T, hip, sc.bn_tokens_case(grid * grid, 2, 5, grid), 5, group, False, 1e-5, grid, f"eval, G = {grid}, group {group}")


@pytest.mark.parametrize("n_prefix", [0, 1, 5])
@pytest.mark.parametrize("train,group", [(True, 1), (True, 2), (False, 1)])
def test_bn_prefix_lengths(T, hip, n_prefix, train, group):
    check_bn(T, hip, sc.bn_tokens_case(29 * 29, 2, n_prefix, 100 + n_prefix), n_prefix, group, train, 1e-5, n_prefix,
             f"n_prefix {n_prefix}, train {train}, group {group}")


@pytest.mark.parametrize("train,group", [(True, 1), (True, 2), (False, 2)])
def test_bn_other_eps(T, hip, train, group):
    check_bn(T, hip, sc.bn_tokens_case(29 * 29, 2, 5, 55), 5, group, train, 1e-3, 55, f"eps 1e-3, train {train}, group {group}")


# --------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_saturated_selector_three_block_refiner(T, hip):
    """SequencePipeline at the default config with a saturated selector and a refiner of three residual blocks (the depth is
    taken from the state dict on both sides): every frame and pair bit exact, and the keypoint lists do repeat cells."""
    from oracle_check import check_pass
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    cfg = ExtractorConfig()
    ssd, rsd = sc.steep_selector(0, 256, 200), synth.refiner_state(0, n_blocks=3)
    toks, imgs = dev(T, synth.token_sequence(4, 28)), dev(T, synth.image_sequence(4))
    pipe = SequencePipeline(cfg, ssd, rsd, device="cuda")
    assert pipe.refiner.n_blocks == 3
    out = pipe.run(imgs, toks)
    res = check_pass(out, imgs, toks, ssd, rsd, cfg.input_size, cfg.num_keypoints, cfg, [(0, 4)])
    assert res["bit_exact"], res["first_mismatch"]
    assert res["frames_checked_vs_oracle"] == 4 and res["pairs_checked"] == 3 and res["matches_checked"] > 0, res
    idx = out["idx"].cpu().numpy()
    assert not out["status"].cpu().numpy().any()
    assert any(np.unique(i).size < cfg.num_keypoints for i in idx)
    assert float((out["scores"] == 1.0).float().mean()) > 0.2
