"""GPU tests of the validation stage (csrc/validate.hip, SequencePipeline.validation_stats, sslam_amd.validation) against the
float64 statement tests/val_ref.py and the reference-held values of tests/golden/val_losses.npz.

One tolerance rule for every scalar (val_ref.tolerance): |x - ref64| <= max(4 |ref32 - ref64|, 2^-20 max(1, |ref64|)), with
ref32 the reference's own fp32 value where a golden holds one.  An intermediate that comes out of a cancellation takes the
same 2^-20 at its natural scale, named at the assertion:
  * a row's log-sum-exp: max(|lse|, 1 / T).  A similarity of unit vectors is a 128-term fp32 dot product, roundoff in units
    of 2^-24 at scale 1, and the logit is that similarity over T;
  * Sobel block means and the frame maximum: 8 max |gray|, the sum of the Sobel weights' magnitudes times the largest pixel;
  * the centred sums A, E, Ss: the uncentred sums they are what is left of - sqrt(sum P^2 sum s^2), sum P^2, sum s^2;
  * per-dimension descriptor means: 1 (the rows are unit vectors); their centred sums of squares: the value.
Exact assertions carry no tolerance."""
import os

import numpy as np
import pytest

import synth
import val_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 37, 64, 65, 128, 129, 500)       # the tile edges of the 64-candidate stage and of the 128-query block


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "val_losses.npz"))


def _same(T, a, b):
    """Same shape and the same bits (floats compared as integers: a NaN or a signed zero cannot hide a difference)."""
    if a.shape != b.shape:
        return False
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return T.equal(a.view(T.int32), b.view(T.int32)) if a.dtype.is_floating_point else T.equal(a, b)


def _bank(k, related):
    """3 frames of k unit descriptors with duplicated rows (the exact ties of the real selector); related: frames 1 and 2 are
    noisy copies of frame 0, so that similarities reach 0.9 and the clamp at 50 is active for T = 0.01."""
    dup = min(k // 4, 8)
    if related and k > 1:
        d0, d1 = synth.descriptor_pair(11 + k, k, k, dup, noise=0.25)[:2]
        d2 = synth.descriptor_pair(11 + k, k, k, dup, noise=0.4)[1]
        return np.stack([d0, d1, d2])
    return np.stack([synth.unit_descriptors(100 * k + f, k, 128, dup) for f in range(3)])


_LSE_REF = {}


def _lse_ref(k, related, temperature, a, b):
    key = (k, related, temperature, a, b)
    if key not in _LSE_REF:
        bank = _bank(k, related)
        x = val_ref.logits(bank[a], bank[b], temperature)
        _LSE_REF[key] = (val_ref.row_lse(bank[a], bank[b], temperature), x)
    return _LSE_REF[key]


def _check_lse(T, lib, k, related, temperature, first, second, lse, ce, s00, nn12, nn21, pstats, cnt, where):
    lse, ce, s00, nn12, nn21, pstats, cnt = (t.cpu().numpy() for t in (lse, ce, s00, nn12, nn21, pstats, cnt))
    for p, (a, b) in enumerate(zip(first, second)):
        if a < 0 or b < 0:      # an absent pair: zero rows, count 0
            assert not lse[p].view(np.uint32).any() and not ce[p].view(np.uint32).any() and s00[p] == 0, (where, p)
            assert cnt[p] == 0 and not pstats[p].view(np.uint32).any(), (where, p)
            continue
        ref, x = _lse_ref(k, related, temperature, a, b)
        scale = np.maximum(np.abs(ref), 1.0 / temperature)      # the logits' scale (module docstring)
        tol = val_ref.tolerance(ref, scale=scale)
        err = np.abs(lse[p] - ref)
        print(f"{where} K {k} T {temperature} pair ({a}, {b}): max |lse - ref| {err.max():.3e}, tolerance there {tol[err.argmax()]:.3e}")
        assert (err <= tol).all(), (where, k, p, float(err.max()))
        cref = ref - x.max(axis=1)
        assert (np.abs(ce[p] - cref) <= val_ref.tolerance(cref, scale=scale)).all(), (where, k, p)
        # the pair's sums over the DEVICE's mutual rows (its arg-max arrays are pinned bit for bit elsewhere)
        i = np.arange(k)
        mask = nn21[p][nn12[p]] == i
        assert cnt[p] == mask.sum() and pstats[p, lib.VAL_PAIR_SLOTS["matches"]] == mask.sum()
        want = float(np.sum(ref[mask] - x[i[mask], nn12[p][mask]]))
        tol_sum = val_ref.tolerance(want, scale=max(abs(want), mask.sum() / temperature))      # a sum of that many rows
        assert abs(pstats[p, lib.VAL_PAIR_SLOTS["ce_sum"]] - want) <= tol_sum, (where, k, p)
        pad = float(ref[0] - x[0, 0])
        assert abs(pstats[p, lib.VAL_PAIR_SLOTS["pad_ce"]] - pad) <= val_ref.tolerance(pad, scale=max(abs(pad), 1.0 / temperature))


@pytest.mark.parametrize("related,temperature", [(False, 0.1), (True, 0.01)])
@pytest.mark.parametrize("k", KS)
def test_row_lse_strided_and_listed(T, k, related, temperature):
    """Row log-sum-exp, its cross-entropy form and the pair sums against float64 - at spacing 1 and over a listed pair set with
    a repeated frame, a self pair and an absent pair - and the exact assertions: the listed form gives the strided form's
    bits for the same pairs, a second run gives the first run's bits, n_matches is the batched matcher's count."""
    from sslam_amd import lib
    import matching
    bank = T.from_numpy(_bank(k, related)).cuda()
    sal = T.from_numpy(np.random.default_rng(k).uniform(0, 1, (3, 4, 4)).astype(np.float32)).cuda()
    if temperature == 0.01 and k > 1:
        raw = val_ref.sims(bank[0].cpu().numpy(), bank[1].cpu().numpy()) / temperature
        assert (raw > 50).any(), "the clamp is meant to be active"
    stride = k * lib.D_OUT

    def strided():
        nn12, s12, nn21, _, _ = lib.sim_argmax(bank[:2], stride, k, bank[1:], stride, k, 2)
        lse, ce, s00 = lib.row_lse(bank[:2], stride, k, bank[1:], stride, k, 2, s12, temperature)
        ps, cnt = lib.val_pair_stats(sal[:2], sal[1:], nn12, nn21, s12, ce, s00, temperature)
        return lse, ce, s00, nn12, nn21, ps, cnt

    first, second = [0, 2, -1, 1, 2, 0], [1, 0, 1, 2, 2, 1]
    f, s = (T.tensor(v, dtype=T.int32, device="cuda") for v in (first, second))

    def listed():
        nn12, s12, nn21, _, _ = lib.sim_argmax_pairs(bank, f, s)
        lse, ce, s00 = lib.row_lse_pairs(bank, f, s, s12, temperature)
        ps, cnt = lib.val_pair_stats_pairs(sal, f, s, nn12, nn21, s12, ce, s00, temperature)
        return lse, ce, s00, nn12, nn21, ps, cnt

    a, b = strided(), listed()
    _check_lse(T, lib, k, related, temperature, [0, 1], [1, 2], *a, "strided")
    _check_lse(T, lib, k, related, temperature, first, second, *b, "listed")
    for name, x, y in zip(("lse", "ce", "s00", "nn12", "nn21", "pair stats", "n_matches"), a, b):
        assert _same(T, x[0], y[0]) and _same(T, x[1], y[3]) and _same(T, y[0], y[5]), f"{name}: strided and listed bits differ"
    for name, x, y in zip(("lse", "ce", "s00", "nn12", "nn21", "pair stats", "n_matches"), a, strided()):
        assert _same(T, x, y), f"{name}: a second run gave other bits"
    for name, x, y in zip(("lse", "ce", "s00", "nn12", "nn21", "pair stats", "n_matches"), b, listed()):
        assert _same(T, x, y), f"{name}: a second listed run gave other bits"
    for p in range(2):
        m = matching.find_matches_batched(bank[p:p + 1], bank[p + 1:p + 2])
        assert int(a[6][p]) == m.shape[1], "n_matches is the count of the batched M3 matcher"
    # the repeat term of the same pairs
    sn = sal.cpu().numpy()
    for p in range(2):
        want = float(np.mean((sn[p].astype(np.float64) - sn[p + 1]) ** 2))
        assert abs(float(a[5][p, lib.VAL_PAIR_SLOTS["repeat"]]) - want) <= val_ref.tolerance(want)


def _images(kind, n, size, seed=0):
    rng = np.random.default_rng(1000 * size + seed)
    if kind == "random":      # smooth blocks plus texture, in the range of a normalised image
        coarse = rng.normal(0, 1, (n, 3, size // 8, size // 8))
        return (np.kron(coarse, np.ones((8, 8))) + rng.normal(0, 0.3, (n, 3, size, size))).astype(np.float32)
    if kind == "constant":
        return np.full((n, 3, size, size), 0.75, np.float32)
    img = np.zeros((n, 3, size, size), np.float32)      # "border": structure on the outermost rows and columns only
    img[:, :, 0, :] = rng.normal(0, 1, (n, 3, size))
    img[:, :, -1, :] = rng.normal(0, 1, (n, 3, size))
    img[:, :, :, 0] = rng.normal(0, 1, (n, 3, size))
    img[:, :, :, -1] = rng.normal(0, 1, (n, 3, size))
    return img


@pytest.mark.parametrize("kind", ["random", "constant", "border"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", [64, 80, 448])
def test_sobel_pool_and_frame_stats(T, size, n, kind):
    """The Sobel / pool pass and the per-frame statistics against float64, with zero padding at the image border; frame 0 has a
    constant saliency map (A = Ss = 0 exactly: correlation 0).  One launch over n frames equals per-frame launches, and a
    second run the first, bit for bit."""
    from sslam_amd import lib
    g, k = size // 16, 37
    img = _images(kind, n, size)
    rng = np.random.default_rng(size + n)
    sal = rng.uniform(0.02, 0.98, (n, g, g)).astype(np.float32)
    sal[0] = np.float32(0.4)
    desc = np.stack([synth.unit_descriptors(7 * size + f, k, 128, 4) for f in range(n)])
    d_img, d_sal, d_desc = (T.from_numpy(x).cuda() for x in (img, sal, desc))
    pooled, emax = lib.edge_pool(d_img)
    stats, dmean, dm2 = lib.val_frame_stats(d_sal, pooled, emax, d_desc)
    P, M, S, DM, D2 = (t.cpu().numpy() for t in (pooled, emax, stats, dmean, dm2))
    slot = lib.VAL_FRAME_SLOTS
    for f in range(n):
        ref = val_ref.frame_stats(sal[f], img[f], desc[f])
        c = img[f].astype(np.float64)
        gray_scale = 8.0 * np.abs(0.299 * c[0] + 0.587 * c[1] + 0.114 * c[2]).max()      # Sobel weights times the largest pixel
        err = np.abs(P[f] - ref["pooled"])
        print(f"S {size} {kind} frame {f}: max |P - ref| {err.max():.3e} (tolerance {val_ref.tolerance(0.0, scale=gray_scale):.3e}), "
              f"m {M[f]:.6e} ref {ref['edge_max']:.6e}")
        assert (err <= val_ref.tolerance(ref["pooled"], scale=gray_scale)).all(), (size, kind, f, float(err.max()))
        assert abs(M[f] - ref["edge_max"]) <= val_ref.tolerance(ref["edge_max"], scale=gray_scale)
        assert S[f, slot["edge_max"]] == M[f]
        for key in ("sal_mean", "sal_var", "sal_max", "sal_dx", "sal_dy", "sal_high", "edge_mean"):
            assert abs(S[f, slot[key]] - ref[key]) <= val_ref.tolerance(ref[key]), (key, f, S[f, slot[key]], ref[key])
        s64, p64 = sal[f].astype(np.float64), ref["pooled"]
        uncentred = dict(edge_a=np.sqrt((p64 ** 2).sum() * (s64 ** 2).sum()), edge_e=(p64 ** 2).sum(), sal_ss=(s64 ** 2).sum())
        for key, scale in uncentred.items():      # centred sums: what a cancellation leaves of the uncentred ones
            assert abs(S[f, slot[key]] - ref[key]) <= val_ref.tolerance(ref[key], scale=scale), (key, f, S[f, slot[key]], ref[key])
        assert (np.abs(DM[f] - ref["desc_mean"]) <= val_ref.tolerance(ref["desc_mean"], scale=1.0)).all()      # unit rows
        assert (np.abs(D2[f] - ref["desc_m2"]) <= val_ref.tolerance(ref["desc_m2"])).all()
    assert S[0, slot["edge_a"]] == 0.0 and S[0, slot["sal_ss"]] == 0.0 and S[0, slot["sal_var"]] == 0.0, "a constant map centres to zero"
    assert S[0, slot["sal_mean"]] == np.float32(0.4)
    # exact: per-frame launches, and a second run
    for f in range(n):
        p1, m1 = lib.edge_pool(d_img[f:f + 1])
        s1, a1, b1 = lib.val_frame_stats(d_sal[f:f + 1], p1, m1, d_desc[f:f + 1])
        for name, x, y in (("pooled", p1, pooled), ("edge_max", m1, emax), ("stats", s1, stats), ("desc_mean", a1, dmean), ("desc_m2", b1, dm2)):
            assert _same(T, x[0], y[f]), f"{name} of frame {f}: a launch of its own gave other bits"
    p2, m2 = lib.edge_pool(d_img)
    s2, a2, b2 = lib.val_frame_stats(d_sal, p2, m2, d_desc)
    for name, x, y in (("pooled", p2, pooled), ("edge_max", m2, emax), ("stats", s2, stats), ("desc_mean", a2, dmean), ("desc_m2", b2, dm2)):
        assert _same(T, x, y), f"{name}: a second run gave other bits"


def _assert_rule(got, order, ref32, ref64, what):
    for key, r32, r64 in zip(order, ref32, ref64):
        tol = val_ref.tolerance(r64, r32)
        print(f"{what} {key:20s} got {got[key]:+.9e} ref64 {r64:+.9e} |d| {abs(got[key] - r64):.2e} tol {tol:.2e}")
    for key, r32, r64 in zip(order, ref32, ref64):
        assert abs(got[key] - r64) <= val_ref.tolerance(r64, r32), (what, key, got[key], r64)


@pytest.mark.parametrize("name", ["g4", "g5"])
def test_golden_cases_end_to_end(T, golden, name):
    """The reference-held cases through validation_stats and compose at B = 4 and B = 1 (the listed form: pair b = frames
    (b, 4 + b) of a bank of eight), and the same pairs in the strided form (spacing 4): identical bits."""
    from sslam_amd import validation
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    c = val_ref.golden_case(golden, name)
    g, k = c["saliency"].shape[1], c["desc"].shape[1]
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    out = dict(saliency=T.from_numpy(c["saliency"]).cuda(), descriptors=T.from_numpy(c["desc"]).cuda())
    img = T.from_numpy(c["images"]).cuda()
    stats = pipe.validation_stats(out, img, first=c["first"], second=c["second"], temperature=c["temperature"])
    assert np.array_equal(stats["n_matches"].cpu().numpy(), golden[f"{name}_counts"])
    b4 = validation.compose(stats, batch=4)
    _assert_rule({key: float(v[0]) for key, v in b4.items()}, c["order"], golden[f"{name}_ref32_b4"], golden[f"{name}_ref64_b4"], f"{name} B=4")
    b1 = validation.compose(stats, batch=1)
    for b in range(4):
        _assert_rule({key: float(v[b]) for key, v in b1.items()}, c["order"], golden[f"{name}_ref32_b1"][b], golden[f"{name}_ref64_b1"][b],
                     f"{name} B=1 pair {b}")
    strided = pipe.validation_stats(out, img, spacing=4, temperature=c["temperature"])
    for key, v in stats.items():
        if hasattr(v, "shape"):
            assert _same(T, v, strided[key]), f"{key}: the strided form gave other bits than the listed form"


def test_validate_on_a_synthetic_sequence(T):
    """validation.validate on 6 synthetic frames at input_size 80 (tokens in, tests/synth.py weights), uint8 images through A0,
    batches of 4 with a last batch of 1: equal to val_ref.validate on the pipeline's OWN saliency, descriptors and A0 image
    within the rule; the uint8 and the fp32 image give the same bits; the stage is capturable."""
    from sslam_amd import validation
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    n, g, k = 6, 5, 12
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    toks = T.from_numpy(synth.token_sequence(n, g)).cuda()
    imgs = T.from_numpy(synth.image_sequence(n, 96, 128)).cuda()
    got = validation.validate(pipe, imgs, spacing=1, batch=4, tokens=toks)
    out = pipe.extract(toks, None)
    a0 = pipe.preprocess(imgs)
    sal, desc = out["saliency"].cpu().numpy(), out["descriptors"].cpu().numpy()
    first = np.arange(n - 1)
    want = val_ref.validate(sal, a0.cpu().numpy(), desc, first, first + 1, batch=4, temperature=0.1)
    assert set(got) == set(want) == set(("total",) + validation.TERMS + validation.METRICS)
    for key in want:
        print(f"validate {key:20s} got {got[key]:+.9e} ref64 {want[key]:+.9e} |d| {abs(got[key] - want[key]):.2e}")
    for key in want:
        assert abs(got[key] - want[key]) <= val_ref.tolerance(want[key]), (key, got[key], want[key])
    s_u8 = pipe.validation_stats(out, imgs, spacing=1)
    s_f32 = pipe.validation_stats(out, a0, spacing=1)
    for key, v in s_u8.items():
        if hasattr(v, "shape"):
            assert _same(T, v, s_f32[key]), key
    # only launches on the current stream: the stage can be captured and replayed
    side = T.cuda.Stream()
    side.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(side):
        pipe.validation_stats(out, a0, spacing=1)      # warm-up: every buffer of the pipeline exists before the capture
    T.cuda.current_stream().wait_stream(side)
    T.cuda.synchronize()
    graph = T.cuda.CUDAGraph()
    with T.cuda.graph(graph):
        cap = pipe.validation_stats(out, a0, spacing=1)
    graph.replay()
    T.cuda.synchronize()
    for key, v in s_f32.items():
        if hasattr(v, "shape"):
            assert _same(T, v, cap[key]), f"{key}: the replayed capture gave other bits"
