"""The float64 ViT reference (oracle/ora_vit.py) on the CPU: its exact mode against the eager fp32 definition and against
`transformers.DINOv3ViTModel`, its bf16 mode against its exact mode (rounding off: equal; on: within the drift bar of
tests/test_vit.py), the restated gelu_poly against erf-GELU, the layer-isolation trick, and the softmax shift rule at the
score ranges the GPU tests drive (tests/test_gpu_vit_reference.py)."""
import math

import pytest
import torch

import foreign_vit
from oracle import ora_vit


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def vit():
    return foreign_vit.random_vit(1)


@pytest.fixture(scope="module")
def images():
    torch.manual_seed(0)
    return torch.randn(2, 3, 64, 64)                  # 4 x 4 patches, T = 21 (one partial key tile)


def test_exact_mode_matches_the_fp32_definition(vit, images):
    want = ora_vit.forward(vit, images, "exact")
    with torch.no_grad():
        got = vit.forward_features(images).double()
    rel = _rel(got, want)
    print(f"\neager fp32 definition vs float64: rel {rel:.2e}")
    assert rel < 5e-6, rel                            # observed ~1e-6: fp32 rounding of the eager evaluation
    cos = torch.nn.functional.cosine_similarity(got, want, dim=-1)
    assert float(cos.min()) > 1 - 1e-9


def test_exact_mode_matches_transformers_dinov3():
    from transformers import DINOv3ViTConfig, DINOv3ViTModel
    from sslam_amd.vit import DinoV3ViT
    torch.manual_seed(3)
    hf = DINOv3ViTModel(DINOv3ViTConfig(num_register_tokens=4)).eval()
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if "lambda1" in n:
                p.copy_(0.5 + torch.rand_like(p))
            elif n.endswith("bias") or "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
            elif "cls_token" in n or "register_tokens" in n:
                p.copy_(0.5 * torch.randn_like(p))
            else:
                p.mul_(3.0)
    mine = DinoV3ViT().eval().load_hf_state_dict(hf.state_dict())
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        want = hf(pixel_values=x).last_hidden_state.double()
    got = ora_vit.forward(mine, x, "exact")
    assert float((got - want).abs().max()) < 2e-4


def test_bf16_mode_without_rounding_is_the_exact_forward(vit, images):
    """Shift rule, folded q scale and LayerScale, one-pass LayerNorm: the same forward when nothing is rounded."""
    e = ora_vit.forward(vit, images, "exact")
    b = ora_vit.forward(vit, images, "bf16", round=False, gelu="erf")
    assert float((b - e).abs().max()) < 1e-12


def test_gelu_poly_restated_within_its_claimed_error():
    v = torch.linspace(-8.0, 8.0, 160001, dtype=torch.float64)
    err = float((ora_vit.gelu_poly(v) - ora_vit.gelu_erf(v)).abs().max())
    assert err <= 1.9e-4, err
    # and it is not the tanh form (which is off by up to ~4.7e-4 from the erf form)
    tanh = 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))
    assert float((tanh - ora_vit.gelu_erf(v)).abs().max()) > 2 * err


def test_bf16_mode_within_the_drift_bar_of_the_exact_mode(vit, images):
    e = ora_vit.forward(vit, images, "exact")
    b = ora_vit.forward(vit, images, "bf16")
    rel = _rel(b, e)
    print(f"\nbf16 mode vs exact: rel {rel:.2e}")
    assert rel < 2.5e-2
    assert float(torch.nn.functional.cosine_similarity(b, e, dim=-1).min()) > 0.995


@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_blocks_with_zero_layerscale_are_identities(vit, images, mode):
    """The layer-isolation trick of the GPU tests: with ls1 = ls2 = 0 on every block but one, evaluating the zeroed blocks changes
    nothing, bit for bit (x + 0 = x), and the tokens differ from the final LayerNorm of the embedding only through that block."""
    import copy
    one = copy.deepcopy(vit)
    with torch.no_grad():
        for i, b in enumerate(one.blocks):
            if i != 5:
                b.ls1.zero_()
                b.ls2.zero_()
        one.blocks[5].ls2.zero_()                        # attention half of layer 5 only
    full = ora_vit.forward(one, images, mode, skip_zero_layerscale=False)
    skipped = ora_vit.forward(one, images, mode)
    assert torch.equal(full, skipped)
    with torch.no_grad():
        one.blocks[5].ls1.zero_()
    none = ora_vit.forward(one, images, mode, skip_zero_layerscale=False)
    assert not torch.equal(none, full)
    p = ora_vit.params(one, mode)
    x0 = ora_vit.forward(one, images, mode)
    assert all(not (ly["attn_on"] or ly["mlp_on"]) for ly in p["layers"]) and torch.equal(x0, none)


def test_shift_rule_keeps_the_softmax_at_any_score_range():
    """attn_kernel's shift rule (first-tile maximum, re-centre by max(tile max - shift, 0) when a query of the wave exceeds its
    shift by > 64): with rounding off it is the softmax exactly, for scores all far below zero, far above it, and for a wave
    where one query's later tile jumps by 200 while another's sits 300 below its shift - where re-centring by the unclamped
    difference would scale by 2^300 (inf) and give NaN."""
    torch.manual_seed(1)
    T = 150
    v = torch.randn(1, 1, T, 64, dtype=torch.float64)
    base = torch.randn(1, 1, T, T, dtype=torch.float64)
    guard = base.clone()
    guard[0, 0, 0, 64:128] += 200.0                        # query 0: tile 1 far above its first tile
    guard[0, 0, 1, 64:] -= 300.0                           # query 1 (same wave): later tiles far below its shift
    for s in (base - 1500.0, base + 1500.0, guard):
        tr = {}
        got = ora_vit._attn_kernel_softmax(s, v, lambda t: t, tr)
        want = torch.softmax(s * math.log(2.0), -1) @ v
        assert torch.isfinite(got).all()
        assert float((got - want).abs().max()) < 1e-12
    assert tr["guard_trips"] >= 32 and tr["guard_min_rel"] < -128 and tr["guard_max_rel"] > 64
