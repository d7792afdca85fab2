"""The bf16 ViT's few-frame launch form (SSLAM_VIT_FORM_FEW_FRAME: key-split attention, K-split down projection, csrc/vit.hip)
against the float64 bf16-mode reference of oracle/ora_vit.py under the bars of tests/test_gpu_vit_reference.py, its batch
independence bit for bit, the legality checks of the named-form entries, and the form selected by name through
HipViT.forward_features, SequencePipeline / FrameStepper and DinoBackbone.  The unnamed entries must not move by a bit.

Key ranges (csrc/vit.hip af_per / af_ranges): the 64-key tiles of a frame are cut into ranges of ceil(tiles / 4) tiles, so
T = 6, 14, 54 -> 1 tile, 1 range; 144 (T = 86) -> 2 tiles, 2 ranges (fewer tiles than ranges); 208 (T = 174) -> 3 ranges;
224 (T = 201) -> 4 tiles, 4 ranges of 1; 448 (T = 789) -> 13 tiles, ranges of 4, 4, 4, 1 (a count the ranges do not divide);
640 (T = 1 605) -> 26 tiles, 7, 7, 7, 5; 960 (T = 3 605) -> 57 tiles, 15, 15, 15, 12.

Every comparison prints its numbers (pytest -s)."""
import numpy as np
import pytest
import torch

import foreign_vit
import synth
import test_gpu_vit_reference as ref
from oracle import ora_vit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vit():
    return foreign_vit.random_vit(1).cuda()


def _hv(v):
    from sslam_amd.vit_hip import HipViT
    return HipViT(v)


def _few(v, x, **kw):
    with torch.no_grad():
        return _hv(v).forward_features(x, form="few_frame", **kw)


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("size,frames", [(64, 2), (224, 3), (448, 1), (448, 8)])
def test_whole_forward_few_frame_against_float64(vit, size, frames):
    x = ref._images(frames, size, size)
    want = ora_vit.forward(vit, x, "bf16")
    got = _few(vit, x)
    with torch.no_grad():
        small = _hv(vit).forward_features(x)
    ref._check(f"small form {size}x{frames} (for comparison)", small, want, "bf16")
    ref._check(f"few-frame {size}x{frames}", got, want, "bf16")
    print(f"  few-frame vs small: rel {float((got - small).norm() / small.norm()):.2e}")


@pytest.mark.parametrize("case", list(ref.ISOLATED))
def test_isolated_layer_few_frame_against_float64(vit, case):
    """One layer (or twelve attention halves / MLP halves) live: the tight check of the two split sums."""
    one = ref._isolate(vit, ref.ISOLATED[case])
    x = ref._images(2, 224, 7)
    want = ora_vit.forward(one, x, "bf16")
    bars = "bf16_layer" if case.startswith("layer") else "bf16_stack"
    with torch.no_grad():
        small = _hv(one).forward_features(x)
    ref._check(f"small form {case} (for comparison)", small, want, bars)
    ref._check(f"few-frame {case}", _few(one, x), want, bars)


# size -> the key-range case it is (module docstring)
@pytest.mark.parametrize("size,layer", [(16, 0), (48, 0), (112, 5),          # one key tile: one range
                                        (144, 0),                           # 2 tiles: fewer tiles than ranges
                                        (208, 11),                          # 3 tiles: 3 ranges of 1
                                        (224, 5),                           # 4 tiles: 4 ranges of 1
                                        (448, 0),                           # 13 tiles: 4, 4, 4, 1
                                        (640, 11), (960, 0)])               # 26 tiles: 7, 7, 7, 5; 57 tiles: 15, 15, 15, 12
def test_key_range_edges_one_layer_against_float64(vit, size, layer):
    one = ref._isolate(vit, {(layer, 1), (layer, 2)})
    x = ref._images(1, size, size)
    want = ora_vit.forward(one, x, "bf16")
    ref._check(f"few-frame {size}x1 layer {layer}", _few(one, x), want, "bf16_layer")


@pytest.mark.parametrize("case,size", [("negative", 16), ("negative_multitile", 144), ("negative_multitile", 448),
                                       ("positive_multitile", 144)])
def test_softmax_uniform_extreme_scores_few_frame(vit, case, size):
    """Scores ~ -1000 / +1000 in every range: each range's shift lies far from 0, the merge's weights 2^(m_s - M) stay <= 1.
    Only layer 0's attention is live, so the per-layer bar is the matching one (a range's P is rounded relative to the range's
    own shift, not the one-pass shift the reference restates); with every score equal P = 1 exactly in any range: that case is
    held to the softmax bar."""
    one = ref._uniform_scores_model(vit, -1.0 if case.startswith("negative") else 1.0, case.endswith("multitile"))
    x = ref._images(2, size, 5)
    want = ora_vit.forward(one, x, "bf16")
    ref._check(f"few-frame softmax {case} {size}", _few(one, x), want, "bf16_softmax" if (case, size) == ("negative", 16) else "bf16_layer")


def test_softmax_recentre_guard_few_frame(vit):
    """The image of test_softmax_recentre_guard: 144 x 144 is two key tiles = two ranges of one tile, whose maxima differ by more
    than 128 for the dark query - the merge's weight for the lower range underflows to 0 (right) instead of the higher one's
    overflowing."""
    one = ref._guard_model(vit)
    G = 9
    img = torch.zeros(1, 3, 16 * G, 16 * G)
    for p in range(59, 81):
        img[..., (p // G) * 16:(p // G + 1) * 16, (p % G) * 16:(p % G + 1) * 16] = 10.0
    img[..., (10 // G) * 16:(10 // G + 1) * 16, (10 % G) * 16:(10 % G + 1) * 16] = -10.0
    x = img.cuda()
    tr = {}
    want = ora_vit.forward(one, x, "bf16", trace=tr, scores_of_layer=0)
    s = tr["scores"][0, 0]
    d = s[:, 64:].max(-1).values - s[:, :64].max(-1).values
    print(f"\n  range maxima, tile 1 - tile 0: [{float(d.min()):.0f}, {float(d.max()):.0f}]")
    assert float(d.min()) < -128 and float(d.max()) > 64
    ref._check("few-frame softmax guard", _few(one, x), want, "bf16_layer")


# ------------------------------------------------------------------------------------------------ batch independence
def test_few_frame_tokens_do_not_depend_on_the_batch(vit):
    from sslam_amd import lib
    hv = _hv(vit)
    x = ref._images(8, 448, 11)
    with torch.no_grad():
        t8 = hv.forward_features(x, form="few_frame").clone()
        again = hv.forward_features(x, form="few_frame").clone()
        alone = [hv.forward_features(x[i:i + 1], form="few_frame").clone() for i in (0, 3, 7)]
        chunked = hv.forward_features(x, form="few_frame", chunk=3).clone()          # groups of 3, 3, 2
        small = hv.forward_features(x).clone()
    assert torch.equal(again, t8)
    for j, i in enumerate((0, 3, 7)):
        assert torch.equal(alone[j][0], t8[i]), i
    assert torch.equal(chunked, t8)
    print(f"\n  few-frame vs small, 8 x 448: rel {float((t8 - small).norm() / small.norm()):.2e}, equal {torch.equal(t8, small)}")
    assert not torch.equal(t8, small), "the few-frame form sums in another order: equal bits mean it did not run"


def test_few_frame_patch_route_equals_the_image_route(vit):
    from sslam_amd import lib
    from sslam_amd.pipeline import ResampleTables
    imgs = torch.from_numpy(synth.image_sequence(3)).cuda()                            # 640 x 480 -> 448: the patch route exists
    th, tv = ResampleTables(torch.device("cuda")).get(480, 640, 448, False)
    patches = lib.preprocess_u8_patches(imgs, 448, th, tv)
    assert patches is not None
    chw = lib.preprocess_u8(imgs, 448, th, tv)
    hv = _hv(vit)
    with torch.no_grad():
        a = hv.forward_features(chw, form="few_frame").clone()
        b = hv.forward_features(None, patches=patches, size=448, form="few_frame").clone()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ legality
def test_named_form_legality_on_the_device(vit):
    from sslam_amd import lib
    hv = _hv(vit)
    S = 64
    x = ref._images(9, S, 64)
    with torch.no_grad():
        t8 = hv.forward_features(x[:8], form="few_frame").clone()                  # also points hv.w at the RoPE tables of G = 4
    FEW = lib.VIT_FORM_FEW_FRAME
    need8 = lib.vit_workspace_bytes(8, S, FEW)
    ws = torch.empty(need8, dtype=torch.uint8, device="cuda")
    big = torch.empty(4 * need8, dtype=torch.uint8, device="cuda")
    out = torch.full((9, 5 + (S // 16) ** 2, 384), float("nan"), device="cuda")
    n0 = lib.launch_count()
    with pytest.raises(ValueError, match="invalid"):
        lib.vit_forward(x, hv.w, big, out=out, form=FEW)                            # 9 frames
    with pytest.raises(ValueError, match="invalid"):
        lib.vit_forward(x[:2].contiguous(), hv.w, big, out=out[:2], form=7)         # unknown form
    with pytest.raises(ValueError, match="invalid"):
        lib.vit_forward(x[:8].contiguous(), hv.w, ws[:need8 - 1], out=out[:8], form=FEW)
    assert lib.launch_count() == n0, "a refused call launched something"
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for n in range(1, 9):                                                           # one buffer sized for 8 serves every shorter launch
        got = lib.vit_forward(x[:n].contiguous(), hv.w, ws, form=FEW)
        assert torch.equal(got, t8[:n]), n


# ------------------------------------------------------------------------------------------------ the old entries
def test_unnamed_entries_are_untouched_and_forms_by_name(vit):
    from sslam_amd import lib
    hv = _hv(vit)
    x = ref._images(12, 448, 21)
    with torch.no_grad():
        for n in (3, 12):
            a = hv.forward_features(x[:n]).clone()
            b = hv.forward_features(x[:n], form=None, batch_frames=5).clone()
            assert torch.equal(a, b), n
        d3 = hv.forward_features(x[:3]).clone()
        d12 = hv.forward_features(x).clone()
        ws = torch.empty(lib.vit_workspace_bytes(12, 448), dtype=torch.uint8, device="cuda")
        s3 = lib.vit_forward(x[:3].contiguous(), hv.w, ws, form=lib.VIT_FORM_SMALL)
        t12 = lib.vit_forward(x, hv.w, ws, form=lib.VIT_FORM_THROUGHPUT)
        assert torch.equal(s3, d3) and torch.equal(t12, d12)
        assert torch.equal(hv.forward_features(x[:3], form="small"), d3)
        assert torch.equal(hv.forward_features(x, form="throughput"), d12)
        # above 8 frames "few_frame" changes nothing
        assert torch.equal(hv.forward_features(x, form="few_frame"), d12)
        assert torch.equal(hv.forward_features(x[:3], form="few_frame", batch_frames=12), d3)
    with pytest.raises(ValueError, match="form"):
        hv.forward_features(x[:1], form="bogus")


# ------------------------------------------------------------------------------------------------ pipeline, stepper, backbone
def _pipe(vit_form, vit):
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    return SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0), device="cuda", vit=vit,
                            vit_precision="bf16", vit_form=vit_form)


def test_pipeline_and_stepper_in_the_few_frame_form():
    import test_gpu_harness as har
    from sslam_amd import lib
    from sslam_amd.online import FrameStepper
    from sslam_amd.vit import DinoV3ViT
    torch.manual_seed(3)
    dv = DinoV3ViT().cuda().eval()
    imgs_np = synth.image_sequence(12)
    imgs = torch.from_numpy(imgs_np).cuda()
    pf, pn = _pipe("few_frame", dv), _pipe(None, dv)
    tok = pf.tokens_from_images(imgs[:4]).clone()
    assert torch.equal(tok, pf.vit_hip.forward_features(pf.preprocess(imgs[:4]), form="few_frame"))
    assert not torch.equal(tok, pn.tokens_from_images(imgs[:4])), "vit_form did not reach the ViT"
    want = {k: v.clone() for k, v in pf.run(imgs[:4]).items()}
    har._assert_run_is_the_oracle_chain(want, tok.cpu().numpy(), imgs_np[:4], 448, pf.cfg.num_keypoints)
    for use_graph in (False, True):
        st = FrameStepper(pf, 480, 640, use_graph=use_graph)
        for i in range(4):
            n0 = lib.launch_count()
            o = st.step(imgs[i])
            if use_graph and i:
                assert lib.launch_count() == n0, "a replayed step issues no library call"
            for k in ("idx", "descriptors", "intensity", "scores"):
                assert torch.equal(o[k], want[k][i]), (use_graph, k, i)
            if i:
                c = int(o["match_count"])
                assert c == int(want["match_count"][i - 1]) and torch.equal(o["matches"][:c], want["matches"][i - 1][:c])
    a, b = pf.run(imgs), pn.run(imgs)                        # 12 frames: above the form's limit, the setting changes nothing
    for k in ("idx", "descriptors", "intensity", "scores", "match_count", "matches"):
        assert torch.equal(a[k], b[k]), k


def test_dino_backbone_in_the_few_frame_form():
    from models.dino_backbone import DinoBackbone
    from sslam_amd import lib
    from sslam_amd.vit import DinoV3ViT
    torch.manual_seed(4)
    dv = DinoV3ViT().cuda().eval()
    bb = DinoBackbone(input_size=448, dino=dv, vit_precision="bf16", vit_form="few_frame").cuda().eval()
    plain = DinoBackbone(input_size=448, dino=dv, vit_precision="bf16").cuda().eval()
    hv = _hv(dv)
    x = ref._images(12, 448, 31)
    with torch.no_grad():
        for n in (1, 4):
            n0 = lib.launch_count()
            tok = bb.forward_tokens(x[:n])
            assert lib.launch_count() - n0 >= 50, "the HIP path did not run"
            assert torch.equal(tok, hv.forward_features(x[:n], form="few_frame")), n
            assert not torch.equal(tok, plain.forward_tokens(x[:n])), n
            assert tuple(bb(x[:n]).shape) == (n, 28, 28, 384)
        assert torch.equal(bb.forward_tokens(x), plain.forward_tokens(x))
