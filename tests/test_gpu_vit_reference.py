"""Both HIP ViTs (A1) against the float64 reference of oracle/ora_vit.py: csrc/vit_f32.hip against its exact mode,
csrc/vit.hip against its bf16 mode (the kernel's own rounding points restated), for the whole forward, one layer at a time,
every launch form on both sides of its boundary, the bf16 forward's batch independence, and the softmax at score ranges
LayerNorm-ed activations never reach.

Layer isolation: with ls1 = ls2 = 0 on every block but one, x + 0 leaves the residual stream unchanged bit for bit in both
libraries (the bf16 one folds LayerScale into wo / bo and wdown / bdown, the fp32 one multiplies by ls1 / ls2), so the tokens
are the final LayerNorm of the stream after that one layer (pinned on the CPU by tests/test_oracle_vit.py).

Every comparison prints its numbers (pytest -s).  Bars, per comparison: rel = |got - want| / |want| over all tokens, every
token's cosine, and max |got - want| / max |want|."""
import copy

import pytest
import torch

import foreign_vit
from oracle import ora_vit

pytestmark = pytest.mark.gpu

# Bars (rel, 1 - min cosine, max-abs / scale), ~3x the largest error measured on the MI355X:
#   fp32 kernel vs exact: rel 0.6-1.2e-6, 1 - cos <= 1.1e-12, max/scale <= 1.5e-6 - whole forward, every form, every isolated layer;
#   bf16 kernel vs bf16 mode: whole forward rel 3.6-4.5e-3 (1 - cos <= 1.6e-5, max/scale <= 5.3e-3), one layer 0.8-1.0e-3, twelve
#   attention halves 2.3e-3, twelve MLP halves 2.1e-3 - a kernel rounds its fp32 values to bf16 at other points of the interval
#   than float64 does (flips of one bf16 ulp, 2^-8), ~1e-3 per layer and compounding, so the whole forward is only ~5x inside the
#   2.5e-2 of tests/test_vit.py and the per-layer bars carry the tight check;
#   softmax edge cases (every v equal: the output is v whatever the weights, as long as they are finite): ~1e-7;
#   GELU probe (hidden values pinned away from bf16 ties): bf16 1.7e-7, fp32 3.7e-7; small-variance LayerNorm rows: bf16 1.9e-3.
BARS = {"f32": (4e-6, 4e-12, 5e-6), "bf16": (1.3e-2, 5e-5, 1.6e-2), "bf16_layer": (3e-3, 7e-6, 6e-3),
        "bf16_stack": (7e-3, 3.3e-5, 1.05e-2), "bf16_softmax": (6e-7, 1e-13, 1.2e-6), "f32_softmax": (1.5e-6, 6e-13, 3e-6),
        "bf16_probe": (6e-7, 5e-14, 1e-6), "f32_probe": (1.2e-6, 2.5e-13, 2e-6), "bf16_ln": (6e-3, 3e-5, 1.1e-2)}


@pytest.fixture(scope="module")
def vit():
    return foreign_vit.random_vit(1).cuda()


def _images(frames, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(frames, 3, size, size, generator=g).cuda()


def _check(tag, got, want, bars):
    rel_bar, cos_bar, max_bar = BARS[bars]
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{tag}: non-finite tokens"
    err = got - want
    rel = float(err.norm() / want.norm())
    cos = 1.0 - float(torch.nn.functional.cosine_similarity(got, want, dim=-1).min())
    mx = float(err.abs().max() / want.abs().max())
    print(f"\n  {tag}: rel {rel:.2e}  1-cos {cos:.2e}  max/scale {mx:.2e}")
    assert rel <= rel_bar and cos <= cos_bar and mx <= max_bar, (tag, rel, cos, mx)
    return rel


def _bf16(vit):
    from sslam_amd.vit_hip import HipViT
    return HipViT(vit)


def _f32(vit):
    from sslam_amd.vit_hip import HipViTF32
    return HipViTF32(vit)


def _isolate(vit, keep):
    """A copy with ls1 / ls2 zeroed except for the (layer, half) pairs in `keep` (half 1: attention, 2: MLP)."""
    one = copy.deepcopy(vit)
    with torch.no_grad():
        for i, b in enumerate(one.blocks):
            if (i, 1) not in keep:
                b.ls1.zero_()
            if (i, 2) not in keep:
                b.ls2.zero_()
    return one


ISOLATED = {"layer0": {(0, 1), (0, 2)}, "layer5": {(5, 1), (5, 2)}, "layer11": {(11, 1), (11, 2)},
            "attention_only": {(i, 1) for i in range(12)}, "mlp_only": {(i, 2) for i in range(12)}}


# ------------------------------------------------------------------------------------------------ whole forward
@pytest.mark.parametrize("size,frames", [(64, 2), (224, 3), (448, 1)])
def test_whole_forward_fp32_against_float64(vit, size, frames):
    x = _images(frames, size, size)
    want = ora_vit.forward(vit, x, "exact")
    with torch.no_grad():
        got = _f32(vit).forward_features(x)
    _check(f"fp32 {size}x{frames}", got, want, "f32")


@pytest.mark.parametrize("size,frames", [(64, 2), (224, 3), (448, 1)])
def test_whole_forward_bf16_against_float64(vit, size, frames):
    x = _images(frames, size, size)
    want = ora_vit.forward(vit, x, "bf16")
    with torch.no_grad():
        got = _bf16(vit).forward_features(x)
    _check(f"bf16 {size}x{frames}", got, want, "bf16")
    # the same tokens against the exact forward: the bf16 mode's own drift, for the record
    exact = ora_vit.forward(vit, x, "exact")
    print(f"  (bf16 kernel vs exact: rel {float((got.double().cpu() - exact).norm() / exact.norm()):.2e})")


# ------------------------------------------------------------------------------------------------ one layer at a time
@pytest.mark.parametrize("case", list(ISOLATED))
def test_isolated_layer_fp32_against_float64(vit, case):
    one = _isolate(vit, ISOLATED[case])
    x = _images(2, 224, 7)
    want = ora_vit.forward(one, x, "exact")
    with torch.no_grad():
        got = _f32(one).forward_features(x)
    _check(f"fp32 {case}", got, want, "f32")


@pytest.mark.parametrize("case", list(ISOLATED))
def test_isolated_layer_bf16_against_float64(vit, case):
    one = _isolate(vit, ISOLATED[case])
    x = _images(2, 224, 7)
    want = ora_vit.forward(one, x, "bf16")
    with torch.no_grad():
        got = _bf16(one).forward_features(x)
    _check(f"bf16 {case}", got, want, "bf16_layer" if case.startswith("layer") else "bf16_stack")


# ------------------------------------------------------------------------------------------------ launch forms
# csrc/vit.hip vit_forward_impl: small <=> ceil(rows / 128) * 4 <= 256 <=> rows = frames * T <= 8192 (QKV / up GEMMs one
# 192-column tile per workgroup, two-launch MLP); otherwise the throughput form (3 / 4 tiles per workgroup, fused MLP unless
# SSLAM_VIT_NO_FUSED_MLP).  T = 5 + (S/16)^2: 16 -> 6, 32 -> 9, 48 -> 14, 224 -> 201, 448 -> 789 (10 frames 7 890 small,
# 11 frames 8 679 throughput), 640 -> 1 605, 960 -> 3 605.
BF16_FORMS = [(16, 2), (16, 1400), (32, 3), (32, 1000), (48, 1), (48, 600), (224, 3), (224, 48), (448, 10), (448, 11)]


@pytest.mark.parametrize("size,frames", BF16_FORMS)
def test_bf16_launch_forms_against_float64(vit, knob, size, frames):
    T = 5 + (size // 16) ** 2
    small = frames * T <= 8192
    x = _images(frames, size, 100 + size)
    pick = sorted({0, frames - 1})                     # frames are independent: the reference of the first and the last
    want = ora_vit.forward(vit, x[pick], "bf16")
    with torch.no_grad():
        got = _bf16(vit).forward_features(x, chunk=frames)[pick]
    _check(f"bf16 {size}x{frames} {'small' if small else 'throughput fused'}", got, want, "bf16")
    if not small:
        knob("SSLAM_VIT_NO_FUSED_MLP", 1)
        with torch.no_grad():
            got2 = _bf16(vit).forward_features(x, chunk=frames)[pick]
        _check(f"bf16 {size}x{frames} throughput two-launch MLP", got2, want, "bf16")


@pytest.mark.parametrize("size,layer", [(640, 11), (960, 0)])
def test_bf16_large_frames_one_layer_against_float64(vit, size, layer):
    """640 x 640 (T = 1 605) and one 960 x 960 frame (T = 3 605, 57 key tiles) with one layer live (the reference's cost)."""
    one = _isolate(vit, {(layer, 1), (layer, 2)})
    x = _images(1, size, size)
    want = ora_vit.forward(one, x, "bf16")
    with torch.no_grad():
        got = _bf16(one).forward_features(x)
    _check(f"bf16 {size}x1 layer {layer}", got, want, "bf16_layer")


# csrc/vit_f32.hip: launch_gemm (patch embedding): 128-row tiles x 3 column tiles, blocks < 192 <=> patches <= 8 064 -> the 32-row
# gemm_f32_small_kernel (448: 10 frames = 7 840 small, 11 = 8 624 the 128-row GEMM).  launch_gemm_rows: the 64-row form while
# the padded 128-row blocks < 768 (N = 384: rows <= 31 744), the 32-row one-tile-wave form below 192 padded 64-row blocks for the
# non-transposed epilogues (N = 384: rows <= 3 584, N = 1 152 / 1 536 never at these sizes); 224 x 160 = 32 160 rows runs the
# 128-row form.  Attention: <= 8 frames key split (5 ranges of ceil(tiles / 5) 32-key tiles, merged) + the K-quartered down
# GEMM, above the one-pass form.  Empty key ranges: T <= 32 (one tile: ranges 1-4 empty; 48 -> T = 14) and 208 -> T = 174
# (6 tiles: ranges of 2, ranges 3 and 4 empty).
F32_FORMS = [(448, 8), (448, 9), (448, 10), (448, 11), (208, 2), (48, 3), (16, 1), (224, 160)]


@pytest.mark.parametrize("size,frames", F32_FORMS)
def test_fp32_launch_forms_against_float64(vit, size, frames):
    x = _images(frames, size, 200 + size + frames)
    pick = sorted({0, frames - 1})
    want = ora_vit.forward(vit, x[pick], "exact")
    with torch.no_grad():
        got = _f32(vit).forward_features(x)[pick]
    _check(f"fp32 {size}x{frames}", got, want, "f32")


# ------------------------------------------------------------------------------------------------ batch independence (bf16)
def test_bf16_tokens_do_not_depend_on_the_batch(vit, knob):
    """Within a launch form a frame's tokens are the same bits alone, at position i of 8, and in chunked launches (448: up to
    10 frames small, 11+ throughput).  Across forms (measured, then asserted): the small form and the throughput form with the
    two-launch MLP are bit-identical - every GEMM sums each output over the same fragments in the same k order, whatever the
    number of 192-column tiles per workgroup; the fused MLP sums the down projection in its own k order (64-wide hidden chunks,
    permuted within a chunk) and is not - it is bounded against the float64 reference like the other forms."""
    hv = _bf16(vit)
    x = _images(24, 448, 11)
    with torch.no_grad():
        t8 = hv.forward_features(x[:8], chunk=8).clone()
        alone = [hv.forward_features(x[i:i + 1]).clone() for i in (0, 3, 7)]
        chunked = hv.forward_features(x[:8], chunk=3).clone()            # groups of 3, 3, 2: small form
        t24 = hv.forward_features(x, chunk=24).clone()                   # throughput, fused MLP
        t24c = hv.forward_features(x, chunk=12).clone()                  # two groups of 12: throughput
    for j, i in enumerate((0, 3, 7)):
        assert torch.equal(alone[j][0], t8[i]), i
    assert torch.equal(chunked, t8)
    assert torch.equal(t24c, t24)
    knob("SSLAM_VIT_NO_FUSED_MLP", 1)
    with torch.no_grad():
        n24 = hv.forward_features(x, chunk=24).clone()
    same_small = torch.equal(n24[:8], t8)
    same_fused = torch.equal(t24[:8], t8)
    print(f"\n  small == throughput two-launch MLP: {same_small}; small == throughput fused MLP: {same_fused}")
    assert same_small
    print(f"  fused vs two-launch MLP: rel {float((t24 - n24).norm() / n24.norm()):.2e}")
    want = ora_vit.forward(vit, x[:1], "bf16")
    _check("bf16 448 fused-MLP frame 0", t24[:1], want, "bf16")
    _check("bf16 448 small frame 0", t8[:1], want, "bf16")


# ------------------------------------------------------------------------------------------------ softmax dynamic range
def _layer0_attention(vit):
    """Only layer 0's attention reaches the output: ls2 = 0 on layer 0, ls1 = ls2 = 0 everywhere else."""
    return _isolate(vit, {(0, 1)})


def _uniform_scores_model(vit, sign, lowest_freq):
    """Every token's LN1 row is exactly beta (norm1.weight = 0), so q and k are the same for all tokens: q . k / 8 = sign * 1000
    per head.  lowest_freq: q, k in dims (15, 47) of every head - the y pair of the lowest RoPE frequency, angle
    <= 2 pi 100^(-15/16) = 0.084, so after rotation q . k keeps >= cos(0.168) = 0.986 of its value; else q, k in every dim
    (G = 1: the RoPE angle is 0)."""
    one = _layer0_attention(vit)
    b = one.blocks[0]
    with torch.no_grad():
        b.norm1.weight.zero_()
        b.norm1.bias.zero_()
        b.norm1.bias[0] = 1.0
        b.q_proj.weight.zero_()
        b.k_proj.weight.zero_()
        b.q_proj.bias.zero_()
        if lowest_freq:
            for hh in range(6):
                b.q_proj.bias[64 * hh + 15] = 64.0
                b.k_proj.weight[64 * hh + 15, 0] = 125.0 * sign          # 64 * 125 / 8 = 1000
        else:
            b.q_proj.bias.fill_(4.0)
            b.k_proj.weight[:, 0] = 31.25 * sign                        # 64 * 4 * 31.25 / 8 = 1000
    return one


@pytest.mark.parametrize("case,size", [("negative", 16), ("negative_multitile", 144), ("negative_multitile", 448),
                                       ("positive_multitile", 144)])
def test_softmax_uniform_extreme_scores(vit, case, size):
    """All scores ~ -1000 (natural log units; -1 443 in the exp2 domain): the first key tile's maximum lies below -128, where
    a re-centre by 2^-shift overflows.  And all ~ +1000.  Every token's v is the same, so the attention output is v - in
    closed form - whatever the weights, as long as they are finite."""
    one = _uniform_scores_model(vit, -1.0 if case.startswith("negative") else 1.0, case.endswith("multitile"))
    x = _images(2, size, 5)
    tr = {}
    want_b = ora_vit.forward(one, x, "bf16", trace=tr, scores_of_layer=0)
    s = tr["scores"]
    lo, hi = float(s.min()), float(s.max())
    print(f"\n  {case} {size}: exp2-domain scores in [{lo:.0f}, {hi:.0f}], shifts [{tr['shift_min']:.0f}, {tr['shift_max']:.0f}]")
    if case.startswith("negative"):
        assert hi < -1400 and tr["shift_max"] < -128
    else:
        assert lo > 1400
    want_e = ora_vit.forward(one, x, "exact")
    with torch.no_grad():
        got_b = _bf16(one).forward_features(x)
        got_f = _f32(one).forward_features(x)
    _check(f"bf16 softmax {case} {size}", got_b, want_b, "bf16_softmax")
    _check(f"fp32 softmax {case} {size}", got_f, want_e, "f32_softmax")


def _guard_model(vit):
    """Per-token scores driven by image content through ONE LayerNorm channel (c = 0): norm1.weight = e_0, norm1.bias = 0, the
    patch embedding passes the patch mean into channel 0 only (the bias row b, with b[0] = 0, mean 0, variance 1, on every other
    channel), [CLS] and registers = b.  Plain patches (value 0) normalise to n = 0, bright ones (+10) to n1 ~ +11.9, the dark
    one (-10) to -n1.  In each head's lowest-frequency dim 15: q = 8 + 2 n, k = 8 n, so (exp2 domain) s ~ 0.18 * 8 (8 + 2 n_q) n_k."""
    one = _layer0_attention(vit)
    b = one.blocks[0]
    with torch.no_grad():
        bias = torch.randn(384, generator=torch.Generator().manual_seed(3))
        bias[0] = 0.0
        bias[1:] -= bias[1:].mean()
        bias[1:] /= bias[1:].pow(2).mean().sqrt() * (383 / 384) ** 0.5        # mean 0, E[b^2] = 1 over the 384 channels
        one.patch_embed.weight.zero_()
        one.patch_embed.weight[0] = 1.0 / 512                                  # channel 0 = 1.5 x the patch mean
        one.patch_embed.bias.copy_(bias)
        one.cls_token.copy_(bias.expand_as(one.cls_token))
        one.register_tokens.copy_(bias.expand_as(one.register_tokens))
        b.norm1.weight.zero_()
        b.norm1.weight[0] = 1.0
        b.norm1.bias.zero_()
        b.q_proj.weight.zero_()
        b.k_proj.weight.zero_()
        b.q_proj.bias.zero_()
        for hh in range(6):
            b.q_proj.bias[64 * hh + 15] = 8.0
            b.q_proj.weight[64 * hh + 15, 0] = 2.0
            b.k_proj.weight[64 * hh + 15, 0] = 8.0
    return one


def test_softmax_recentre_guard(vit):
    """144 x 144 (G = 9, T = 86: key tiles [0, 64) and [64, 86)).  Bright patches 59..80 = tokens 64..85 (all of key tile 1), a
    dark patch 10 = token 15 in wave 0 (queries 0..31).  A plain query of wave 0 sees tile 1 exceed its shift (first tile's
    maximum) by > 64 - the guard fires for the wave - while the dark query's tile-1 maximum sits > 128 below its own shift:
    re-centring it by that difference (scale 2^+d) overflowed O and the row sum to inf, NaN tokens (fixed: the shift only rises).
    The reference's scores, with the kernel's wave rule, show the case is reached."""
    one = _guard_model(vit)
    G = 9
    img = torch.zeros(1, 3, 16 * G, 16 * G)
    for p in range(59, 81):
        img[..., (p // G) * 16:(p // G + 1) * 16, (p % G) * 16:(p % G + 1) * 16] = 10.0
    img[..., (10 // G) * 16:(10 // G + 1) * 16, (10 % G) * 16:(10 % G + 1) * 16] = -10.0
    x = img.cuda()
    tr = {}
    want_b = ora_vit.forward(one, x, "bf16", trace=tr, scores_of_layer=0)
    s = tr["scores"][0, 0]                                               # head 0, exp2 domain
    shift = s[:, :64].max(-1).values
    rel1 = s[:, 64:].max(-1).values - shift
    print(f"\n  guard: wave 0 tile-1 max - shift in [{float(rel1[:32].min()):.0f}, {float(rel1[:32].max()):.0f}]; "
          f"re-centred queries {tr['guard_trips']}, lowest tile max of a re-centred wave {tr['guard_min_rel']:.0f}")
    assert float(rel1[:32].max()) > 64 and float(rel1[15]) < -128          # the case, from the scores
    assert tr["guard_trips"] > 0 and tr["guard_min_rel"] < -128 and tr["guard_max_rel"] > 64
    want_e = ora_vit.forward(one, x, "exact")
    with torch.no_grad():
        got_b = _bf16(one).forward_features(x)
        got_f = _f32(one).forward_features(x)
    _check("bf16 softmax guard", got_b, want_b, "bf16_softmax")
    _check("fp32 softmax guard", got_f, want_e, "f32_softmax")


# ------------------------------------------------------------------------------------------------ GELU and LayerNorm probes
def _gelu_probe_model(vit):
    """Layer 0's MLP alone with LN2 -> 1 for every token (norm2.weight = 0, bias = 1) and up_proj.weight = 0: the hidden
    pre-activations are the up bias exactly (the GEMM's initial accumulator plus zero products), 1 536 fp32 values over [-6, 6]
    whose gelu_poly lies at least 2^-7 of a bf16 ulp from a rounding tie - so an fp32 evaluation of the same GELU rounds to the
    same bf16 as the float64 one and the probe's tokens sit at fp32 accumulation noise.  Any other GELU (the tanh form: off by
    up to 4.7e-4, many bf16 ulps of GELU's small negative values) moves them by orders of magnitude more."""
    u = torch.linspace(-6.0, 6.0, 24001, dtype=torch.float32)
    g = ora_vit.gelu_poly(u.double()).float()
    low = g.view(torch.int32) & 0xFFFF
    u = u[((low - 0x8000).abs() > 0x200) & (g != 0)]
    u = u[torch.linspace(0, len(u) - 1, 1536).round().long()]
    one = _isolate(vit, {(0, 2)})
    b = one.blocks[0]
    with torch.no_grad():
        b.norm2.weight.zero_()
        b.norm2.bias.fill_(1.0)
        b.up_proj.weight.zero_()
        b.up_proj.bias.copy_(u)
    return one


@pytest.mark.parametrize("size,frames", [(64, 2), (16, 1400)])        # small form (EpiGelu) and throughput (fused MLP)
def test_gelu_probe_against_float64(vit, size, frames):
    one = _gelu_probe_model(vit)
    x = _images(frames, size, 9)
    pick = sorted({0, frames - 1})
    want_b = ora_vit.forward(one, x[pick], "bf16")
    want_e = ora_vit.forward(one, x[pick], "exact")
    with torch.no_grad():
        got_b = _bf16(one).forward_features(x, chunk=frames)[pick]
        got_f = _f32(one).forward_features(x)[pick]
    _check(f"bf16 GELU probe {size}x{frames}", got_b, want_b, "bf16_probe")
    _check(f"fp32 GELU probe {size}x{frames}", got_f, want_e, "f32_probe")


def test_layernorm_eps_with_small_variance_rows(vit):
    """Residual rows of variance ~1e-5 (patch embedding, [CLS] and registers scaled by 2e-3): LayerNorm's eps (1e-5) then
    moves rstd by ~30 %, so LN1 of layer 0 (both halves live) pins the eps the kernels use - the bf16 one in its folded
    one-pass prologue, the fp32 one in its two-pass kernel."""
    one = _isolate(vit, {(0, 1), (0, 2)})
    with torch.no_grad():
        for p in (one.patch_embed.weight, one.patch_embed.bias, one.cls_token, one.register_tokens):
            p.mul_(2e-3)
    x = _images(2, 64, 13)
    want_b = ora_vit.forward(one, x, "bf16")
    want_e = ora_vit.forward(one, x, "exact")
    with torch.no_grad():
        got_b = _bf16(one).forward_features(x)
        got_f = _f32(one).forward_features(x)
    _check("fp32 small-variance LN", got_f, want_e, "f32")
    _check("bf16 small-variance LN", got_b, want_b, "bf16_ln")


# ------------------------------------------------------------------------------------------------ fp32 workspace and launch groups
@pytest.fixture(scope="module")
def x64():
    return _images(20, 64, 64)


@pytest.fixture(scope="module")
def ref64(vit, x64):
    return ora_vit.forward(vit, x64, "exact")


def test_fp32_workspace_for_a_batch_serves_every_smaller_launch(vit, x64):
    """One buffer of sslam_vit_f32_workspace_bytes(12) at 64 x 64 runs every n <= 12 in each legal form (one-pass always, key
    split up to 8 frames), each the tokens of the form's larger launch bit for bit; where that size is the form's own need (key
    split <= 8, one-pass >= 13 frames), one byte less is SSLAM_E_INVALID - checked before anything is launched."""
    from sslam_amd import lib
    hv = _f32(vit)
    N, S = 12, 64
    with torch.no_grad():
        one_pass = hv.forward_features(x64[:N]).clone()          # also points hv.w at the RoPE tables of G = 4
        split = hv.forward_features(x64[:8]).clone()
    ws = torch.empty(lib.vit_f32_workspace_bytes(N, S), dtype=torch.uint8, device="cuda")
    for n in range(1, N + 1):
        for form, want in ((lib.ATTN_ONE_PASS, one_pass), (lib.ATTN_KEY_SPLIT, split)):
            if form == lib.ATTN_KEY_SPLIT and n > lib.ATTN_KEY_SPLIT_MAX_FRAMES:
                continue
            got = lib.vit_forward_f32(x64[:n].contiguous(), hv.w, ws, attention_form=form)
            assert torch.equal(got, want[:n]), (n, form)
    for n, form in ((1, lib.ATTN_KEY_SPLIT), (5, lib.ATTN_KEY_SPLIT), (8, lib.ATTN_KEY_SPLIT), (13, lib.ATTN_ONE_PASS),
                    (20, lib.ATTN_ONE_PASS)):
        need = lib.vit_f32_workspace_bytes(n, S)
        buf = torch.empty(need, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="invalid"):
            lib.vit_forward_f32(x64[:n].contiguous(), hv.w, buf[:need - 1], attention_form=form)
        lib.vit_forward_f32(x64[:n].contiguous(), hv.w, buf, attention_form=form)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,chunk", [(17, 9), (15, 9), (18, 10), (19, 11), (20, 12), (9, 8), (12, 5), (20, 1)])
def test_fp32_tokens_do_not_depend_on_the_launch_groups(vit, x64, ref64, n, chunk):
    """HipViTF32.forward_features in launch groups of `chunk` frames, a short last group included, gives the tokens of one
    group bit for bit (the form follows the batch: one-pass above 8 frames in every group), within the float64 bars.  A fresh
    instance each time: its workspace is sized from the first group, which must serve the last."""
    hv = _f32(vit)
    with torch.no_grad():
        cut = hv.forward_features(x64[:n], chunk=chunk).clone()
        whole = hv.forward_features(x64[:n], chunk=n).clone()
    assert torch.equal(cut, whole)
    _check(f"fp32 64x{n} in groups of {chunk}", cut, ref64[:n], "f32")
