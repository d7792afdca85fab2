"""A1: the in-repo DINOv3 ViT-S/16 definition against the same architecture family in `transformers`
(DINOv3ViTModel built FROM CONFIG with random weights - no download), and the HIP forward against that definition.
Parity with the reference's *pretrained* timm weights cannot be pinned offline (remote fetch): "parity unpinned" there."""
import numpy as np
import pytest
import torch


def _hf_pair(seed=0):
    from transformers import DINOv3ViTConfig, DINOv3ViTModel
    from sslam_amd.vit import DinoV3ViT
    torch.manual_seed(seed)
    hf = DINOv3ViTModel(DINOv3ViTConfig(num_register_tokens=4)).eval()
    with torch.no_grad():      # make LayerScale / biases / norms non-trivial so that every term is exercised
        for n, p in hf.named_parameters():
            if "lambda1" in n:
                p.copy_(0.5 + torch.rand_like(p))
            elif n.endswith("bias") or "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
            elif "cls_token" in n or "register_tokens" in n:
                p.copy_(0.5 * torch.randn_like(p))
            else:
                p.mul_(3.0)
    mine = DinoV3ViT().eval()
    mine.load_hf_state_dict(hf.state_dict())
    return hf, mine


def test_vit_definition_matches_transformers_dinov3():
    hf, mine = _hf_pair()
    x = torch.randn(2, 3, 64, 96)             # non-square grid (4 x 6 patches): RoPE axes must not be swapped
    with torch.no_grad():
        want = hf(pixel_values=x).last_hidden_state
        got = mine.forward_features(x)
    assert got.shape == want.shape == (2, 1 + 4 + 24, 384)
    assert float((got - want).abs().max()) < 2e-4
    assert mine.embed_dim == 384
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for n, p in hf.named_parameters() if "mask_token" not in n)


@pytest.mark.parametrize("layout", ["transformers", "transformers_flat", "dinov3_upstream", "timm_dinov3"])
def test_foreign_key_layouts_round_trip(layout):
    """A random DinoV3ViT written out in each known third-party key layout (fused qkv, separate / fused-and-masked biases,
    other token names and shapes) and read back through load_mapped_state_dict / from_state_dict: identical parameters,
    identical tokens.  The layouts other than transformers' are unverified against their packages (not installed)."""
    import foreign_vit
    from sslam_amd.vit import KEY_MAPS, DinoV3ViT, detect_key_map
    src = foreign_vit.random_vit(5, depth=3)
    sd = foreign_vit.foreign_state_dict(src, layout)
    assert detect_key_map(sd) == layout
    back = DinoV3ViT.from_state_dict(sd)
    assert len(back.blocks) == 3 and back.embed_dim == 384 and back.n_register == 4 and back.patch == 16
    for (n1, p1), (n2, p2) in zip(src.state_dict().items(), back.state_dict().items()):
        assert n1 == n2 and torch.equal(p1, p2), n1
    x = torch.randn(1, 3, 48, 64)
    with torch.no_grad():
        assert torch.equal(back.forward_features(x), src.forward_features(x))
    again = DinoV3ViT(depth=3).load_mapped_state_dict(sd, KEY_MAPS[layout], fused_qkv=layout in ("dinov3_upstream", "timm_dinov3"))
    assert torch.equal(again.blocks[2].v_proj.bias, src.blocks[2].v_proj.bias)


def test_foreign_conversion_refuses_what_it_cannot_represent():
    import foreign_vit
    from sslam_amd.vit import DinoV3ViT, convert_module
    src = foreign_vit.random_vit(6, depth=2)
    sd = foreign_vit.foreign_state_dict(src, "timm_dinov3")
    sd["blocks.1.attn.k_bias"] = torch.full((384,), 0.1)                   # a k bias that is really applied
    with pytest.raises(ValueError, match="k bias"):
        DinoV3ViT.from_state_dict(sd)
    sd = foreign_vit.foreign_state_dict(src, "dinov3_upstream")
    del sd["blocks.0.attn.qkv.bias_mask"], sd["blocks.1.attn.qkv.bias_mask"]   # fused bias with a live k part, no mask
    with pytest.raises(ValueError, match="k bias"):
        DinoV3ViT.from_state_dict(sd)
    with pytest.raises(KeyError):
        DinoV3ViT.from_state_dict({"weight": torch.zeros(3)})
    # a module in a known layout converts and is verified against its own forward ...
    good = foreign_vit.ForeignViT.from_vit(src)
    vit, why = convert_module(good)
    assert vit is not None and "verified" in why
    # ... one with the same parameter shapes but another RoPE base does not pass the numeric check
    vit, why = convert_module(foreign_vit.ForeignViT.from_vit(src, rope_theta=10000.0))
    assert vit is None and "differ" in why
    vit, why = convert_module(torch.nn.Linear(3, 3))
    assert vit is None


@pytest.mark.gpu
def test_foreign_keyed_module_runs_on_the_hip_vit():
    """The reference's setup (dino_backbone.py:44-48, :85): `self.dino` is a third-party module, not the in-repo class.
    A module with timm-style parameters (fused qkv, q_bias / v_bias, gamma_1 / gamma_2, reg_token) handed to DinoBackbone
    ends up on sslam_vit_forward - same tokens, bit for bit, as the in-repo definition with the same weights - and a
    module that cannot be converted keeps its own eager forward after a warning that says so."""
    import warnings

    import foreign_vit
    from models.dino_backbone import DinoBackbone
    from sslam_amd import lib
    src = foreign_vit.random_vit(7)
    x = torch.randn(3, 3, 448, 448, device="cuda")
    own = DinoBackbone(input_size=448, dino=src).cuda()
    with torch.no_grad():
        want = own.forward_tokens(x).clone()
    bb = DinoBackbone(input_size=448, dino=foreign_vit.ForeignViT.from_vit(src)).cuda()
    assert type(bb.dino).__name__ == "ForeignViT"
    n0 = lib.launch_count()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")                       # the conversion succeeds: no fallback warning
        got = bb.forward_tokens(x)
        feats = bb(x)
    assert lib.launch_count() - n0 >= 2 * 50, "A1 must have run as HIP launches (sslam_vit_forward)"
    assert "verified" in bb.hip_vit_status
    assert torch.equal(got, want) and feats.shape == (3, 28, 28, 384)
    with torch.no_grad():
        eager = bb.dino.forward_features(x)
    assert float((got - eager).norm() / eager.norm()) < 2.5e-2
    # the module's own forward on request: no HIP ViT launch
    ref = DinoBackbone(input_size=448, dino=bb.dino, vit_precision="eager").cuda()
    n0 = lib.launch_count()
    with torch.no_grad():
        assert torch.equal(ref.forward_tokens(x), eager)
    assert lib.launch_count() == n0
    # reference numerics on the HIP kernels: the converted weights on the fp32-operand ViT, within 1e-4 of the module's own tokens
    f32 = DinoBackbone(input_size=448, dino=bb.dino, vit_precision="fp32").cuda()
    with torch.no_grad():
        t32 = f32.forward_tokens(x)
    assert lib.launch_count() > n0 and float((t32 - eager).norm() / eager.norm()) < 1e-4
    # not convertible: warned, eager
    odd = DinoBackbone(input_size=448, dino=foreign_vit.ForeignViT.from_vit(src, rope_theta=10000.0)).cuda()
    with torch.no_grad(), pytest.warns(UserWarning, match="NOT running on the HIP kernels"):
        t = odd.forward_tokens(x)
    with torch.no_grad():
        assert torch.equal(t, odd.dino.forward_features(x))


@pytest.mark.gpu
@pytest.mark.parametrize("size,frames", [(448, 2), (224, 3), (640, 1), (448, 12), (224, 48)])   # the last two: the throughput launch shapes (3 / 4 column tiles per workgroup)
def test_hip_vit_matches_fp32_definition(size, frames):
    from sslam_amd import lib
    from sslam_amd.vit_hip import HipViT
    _, mine = _hf_pair(1)
    mine = mine.cuda()
    torch.manual_seed(size)
    x = torch.randn(frames, 3, size, size, device="cuda")
    before = lib.launch_count()
    with torch.no_grad():
        want = mine.forward_features(x)                 # fp32 torch ops on the same weights
        got = HipViT(mine).forward_features(x)
    assert lib.launch_count() > before
    assert got.shape == want.shape
    err = (got - want).float()
    rel = float(err.norm() / want.norm())
    assert rel < 2.5e-2, rel                            # bf16 operands, fp32 accumulation: ~1e-2 after 12 layers
    assert float(err.abs().max()) < 0.35
    # token-wise cosine similarity: every token, not just the average
    cos = torch.nn.functional.cosine_similarity(got, want, dim=-1)
    assert float(cos.min()) > 0.995


@pytest.mark.gpu
@pytest.mark.parametrize("size,frames", [(448, 2), (224, 3), (640, 1), (448, 9), (32, 5), (48, 1), (960, 1), (448, 8)])
def test_hip_vit_f32_matches_fp32_definition(size, frames):
    """The fp32-operand HIP ViT (sslam_vit_forward_f32: the reference's numerics for A1) against the eager fp32 torch
    definition on the same weights.  Bar (stated here): relative error of the tokens <= 1e-4, every token's cosine > 1 - 1e-6,
    max abs error <= 2e-3 of the token scale - observed ~1e-5: fma-chain contractions against rocBLAS's blocked sums."""
    from sslam_amd import lib
    from sslam_amd.vit_hip import HipViTF32
    _, mine = _hf_pair(1)
    mine = mine.cuda()
    torch.manual_seed(size + frames)
    x = torch.randn(frames, 3, size, size, device="cuda")
    before = lib.launch_count()
    with torch.no_grad():
        want = mine.forward_features(x)
        got = HipViTF32(mine).forward_features(x)
    assert lib.launch_count() >= before + 3 + 12 * 7
    assert got.shape == want.shape
    err = (got - want).float()
    rel = float(err.norm() / want.norm())
    assert rel <= 1e-4, rel
    assert float(err.abs().max()) <= 2e-3 * float(want.abs().max())
    cos = torch.nn.functional.cosine_similarity(got.double(), want.double(), dim=-1)
    assert float(cos.min()) > 1 - 1e-6
    # launch groups: a batch cut in chunks gives the same tokens bit for bit (deterministic kernels, frame-independent)
    if frames >= 3:
        with torch.no_grad():
            assert torch.equal(HipViTF32(mine).forward_features(x, chunk=2), got)


@pytest.mark.gpu
def test_hip_vit_f32_small_and_big_launch_forms_agree():
    """The per-layer GEMM has a 64-row form for launches that would leave most CUs empty (a few frames: what the reference's
    per-frame callers send) and the 128-row throughput form; both sum every output over k in the same order, so a frame's
    tokens do not depend on how many frames share its launch - bit for bit wherever the attention runs the same form:
    inside 20 frames (QKV and up + GELU big, the two residual GEMMs small) and inside 48 frames (all big).
    Launches of <= 8 frames run the KEY-SPLIT attention (five key ranges per query tile, partials merged in a fixed order:
    another summation order of the same softmax): among themselves they are bit-identical and independent of the batch
    (1, 2 and 8 frames), against the one-pass form they agree to ~1e-6 relative (bar 3e-6; A1's bar is 1e-4 against the eager evaluation) -
    and with the test-only knob that switches the split off, bit for bit again."""
    from sslam_amd import lib
    from sslam_amd.vit_hip import HipViTF32
    _, mine = _hf_pair(2)
    mine = mine.cuda()
    torch.manual_seed(5)
    x = torch.randn(48, 3, 448, 448, device="cuda")
    hv = HipViTF32(mine)
    with torch.no_grad():
        t48 = hv.forward_features(x)
        t20 = hv.forward_features(x[:20])
        t8 = hv.forward_features(x[:8])
        t2 = hv.forward_features(x[:2])
        t1 = hv.forward_features(x[1:2])
        again = hv.forward_features(x[:2])
    assert torch.equal(t20, t48[:20])
    assert torch.equal(t2, t8[:2]) and torch.equal(t1[0], t8[1]) and torch.equal(again, t2)          # split form: batch-independent, deterministic
    rel = float((t8 - t48[:8]).norm() / t48[:8].norm())
    worst = float((t8 - t48[:8]).abs().max() / t48[:8].abs().max())
    print(f"\nkey-split vs one-pass attention: rel {rel:.2e}, max-abs / max {worst:.2e}")
    assert rel < 3e-6 and worst < 1e-5          # observed 0.6e-6 .. 1.0e-6 / 1.2e-6: the size of the HIP-vs-eager difference itself
    with lib.knobs(SSLAM_VIT_F32_NO_KEY_SPLIT=1), torch.no_grad():
        u2 = hv.forward_features(x[:2])
        u1 = hv.forward_features(x[1:2])
    assert torch.equal(u2, t48[:2]) and torch.equal(u1[0], t48[1])


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [2, 12])       # the few-frame launch shapes and the throughput ones (fused MLP)
def test_hip_vit_layernorm_with_dc_offset_and_outlier_channels(frames):
    """The LayerNorm folded into the GEMM prologues takes ONE-pass statistics (sum, sum of squares from the producing
    epilogue; var = E[x^2] - mean^2 in fp32), the fp32 definition two-pass ones.  Pretrained ViT residual streams carry a
    per-row offset and a few outlier channels of large magnitude: with a DC offset of 30 and three channels at +-150 (token
    std ~ 1) the HIP forward still meets the bars of the random-weight test (parity with real weights is unpinned;
    this pins the numerics of the statistic itself)."""
    from sslam_amd.vit_hip import HipViT
    _, mine = _hf_pair(4)
    with torch.no_grad():
        off = torch.full((384,), 30.0)
        off[[7, 130, 301]] = torch.tensor([150.0, -150.0, 150.0])
        mine.patch_embed.bias.add_(off)
        mine.cls_token.add_(off)
        mine.register_tokens.add_(off)
    mine = mine.cuda()
    torch.manual_seed(17)
    x = torch.randn(frames, 3, 448, 448, device="cuda")
    with torch.no_grad():
        want = mine.forward_features(x)
        got = HipViT(mine).forward_features(x)
    err = (got - want).float()
    rel = float(err.norm() / want.norm())
    cos = torch.nn.functional.cosine_similarity(got, want, dim=-1)
    assert rel < 2.5e-2 and float(cos.min()) > 0.995, (rel, float(cos.min()))


@pytest.mark.gpu
def test_hip_vit_from_patch_rows_equals_from_image():
    """uint8 frames -> A0 as bf16 patch rows -> sslam_vit_forward_patches gives the tokens of A0 as fp32 image ->
    sslam_vit_forward bit for bit (the patch embedding rounds the image to bf16 either way); no im2patch launch."""
    import synth
    from sslam_amd import lib
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    _, mine = _hf_pair(1)
    pv = SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0), device="cuda", vit=mine.cuda())
    imgs = torch.from_numpy(synth.image_sequence(5)).cuda()
    with torch.no_grad():
        n_img = lib.launch_count()
        want = pv.vit_hip.forward_features(pv.preprocess(imgs)).clone()
        n0 = lib.launch_count()
        got = pv.tokens_from_images(imgs)
        n_pat = lib.launch_count() - n0
    n_img = n0 - n_img
    assert torch.equal(got, want)
    # one launch group: A0 + im2patch + the forward against A0 (patch rows) + the same forward - a silent fallback to the
    # fp32 image (preprocess_u8 + im2patch) would give the same tokens but not one launch fewer
    assert n_pat == n_img - 1, (n_pat, n_img)
    pt = pv.preprocess_patches(imgs)
    assert pt is not None and pt.shape == (5, 784, 768)


@pytest.mark.gpu
def test_hip_vit_launch_groups_on_two_streams_equal_one_group():
    """forward_features cuts the batch into launch groups and alternates them between two side streams; the result is the
    same bits as one group (the kernels are deterministic and a frame's tokens do not depend on its group), and it is visible
    on the caller's stream without any extra synchronisation."""
    from sslam_amd.vit_hip import HipViT
    _, mine = _hf_pair(1)
    hv = HipViT(mine.cuda())
    torch.manual_seed(3)
    x = torch.randn(5, 3, 224, 224, device="cuda")
    with torch.no_grad():
        one = hv.forward_features(x, chunk=5).clone()
        many = hv.forward_features(x, chunk=2)          # 3 groups on 2 streams
        checksum = many.sum()                           # consumed on the current stream right away
    assert torch.equal(one, many)
    assert torch.isfinite(checksum)


def test_vit_weight_packs_are_permutations():
    """Host packers (no GPU): every weight lands in the stream exactly once, rounded to bf16 (and scaled per output row where a
    LayerScale is folded in) - a dropped or duplicated element would show as a changed multiset."""
    import numpy as np

    from sslam_amd import lib

    def bf16_bits(a):
        u = np.ascontiguousarray(a, np.float32).view(np.uint32)
        return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)

    rng = np.random.default_rng(0)
    w = rng.standard_normal((1152, 384)).astype(np.float32)
    assert np.array_equal(np.sort(lib.pack_vit_linear(w).ravel()), np.sort(bf16_bits(w).ravel()))
    w_up = rng.standard_normal((1536, 384)).astype(np.float32)
    w_down = rng.standard_normal((384, 1536)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, 384).astype(np.float32)
    got = np.sort(lib.pack_vit_mlp(w_up, w_down, scale))
    want = np.sort(np.concatenate([bf16_bits(w_up).ravel(), bf16_bits(w_down * scale[:, None]).ravel()]))
    assert np.array_equal(got, want)


# the geometries A0 brings into the ViTs (tests/test_gpu_harness.py, "images in"): (H, W, S, K, the bf16 ViT's route, taps)
IMAGES_IN_ROWS = {
    "vga448": (480, 640, 448, 500, "patch", 5),           # the shipped geometry
    "vga224": (480, 640, 224, 100, "patch", 7),           # exactly 7 taps: the last ratio on the patch route
    "w704_224": (480, 704, 224, 100, "image", 9),         # the first ratio on the fp32-image fallback
    "hd448": (1080, 1920, 448, 500, "image", 11),
    "tiny64": (160, 360, 64, 10, "image", 13),            # G = 4: cheap to reference
    "odd224": (231, 517, 224, 100, "patch", 7),           # 358 281-byte frames, a batch from frame 0: aligned base
    "odd224_view": (231, 517, 224, 100, "image", 7),      # the same frames as a view from frame 1: unaligned base
}
IMAGES_IN_MAXR_ROW = (480, 640, 64, 10)                   # 480 / 64: 17 vertical taps, 137 input rows per 16-row tile


def test_images_in_rows_take_the_route_they_name():
    """Host tables (no GPU): the horizontal tap counts the pipeline uploads (lib.resample_table) follow Pillow's bilinear rule,
    2 ceil(W / S) + 1, and put each row on the route it names (the tiled patch-row kernel takes <= 7 taps), so a row cannot drift
    onto the other route unnoticed; the odd row's frames are not a whole number of dwords."""
    import math

    from sslam_amd import lib
    for name, (h, w, s, k, route, taps) in IMAGES_IN_ROWS.items():
        kh = lib.resample_table(w, s, False)[2]
        assert kh == taps == 2 * math.ceil(w / s) + 1, name
        assert (route == "patch") == (kh <= 7 and not name.endswith("_view")), name
        assert k <= (s // 16) ** 2, name
    assert (231 * 517 * 3) % 4 != 0
    h, w, s, _ = IMAGES_IN_MAXR_ROW
    assert lib.resample_table(h, s, False)[2] == 17


def test_vit_f32_workspace_is_monotone_in_the_frame_count():
    """Host entry (no GPU): sslam_vit_f32_workspace_bytes never decreases with the frame count, so a buffer sized for a batch
    serves every smaller launch in either attention form (the key-split partials put 8 frames above 9 - 12 one-pass ones)."""
    from sslam_amd import lib
    for s in (64, 448, 1280):
        b = [lib.vit_f32_workspace_bytes(n, s) for n in range(1, 41)]
        down = [n + 2 for n in range(len(b) - 1) if b[n + 1] < b[n]]
        assert not down, (s, down)
