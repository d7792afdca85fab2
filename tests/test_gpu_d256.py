"""GPU tests of descriptor width 256: the refiner's two-tile output projection, the D = 256 instantiations of the similarity /
arg-max and log-sum-exp kernels, the descriptor moments, and every layer above them (sslam_amd.lib, matching.py,
SequencePipeline, the streaming harness, the online stepper, validation, the drop-in DescriptorRefiner).

Bit for bit against oracle/ora.py (whose similarity is one fma chain over k = 0 .. 255 and whose refiner evaluates the output
projection in the kernel's column layout) wherever no tolerance is named.  Tolerances that are named:
  * against tests/golden/d256.npz (the reference's own outputs): descriptors within 5e-6, the bar of tests/test_oracle_golden.py;
    match INDICES identical (the fixture's smallest top-1 / top-2 gaps exceed 4e-6);
  * validation against tests/val_ref.py in float64: the rule of tests/test_gpu_validation.py (val_ref.tolerance; a row's
    log-sum-exp at scale max(|lse|, 1 / T); descriptor means at scale 1, their centred sums of squares at their own value)."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import d256_cases as cases
import synth
import val_ref
from oracle import ora

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = cases.D


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "d256.npz"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _packed(T, n_blocks):
    from sslam_amd import lib
    sd = cases.refiner_state(n_blocks)
    return sd, T.from_numpy(lib.pack_refiner(ora.refiner_weight_list(sd, n_blocks), n_blocks)).cuda()


# ------------------------------------------------------------------------------------------------ the refiner
@pytest.mark.parametrize("n_blocks", [0, 2])
def test_refine_256_bit_exact(T, gold, n_blocks):
    from sslam_amd import lib
    sd, packed = _packed(T, n_blocks)
    x = cases.mlp_rows()
    want = ora.refine(x, sd, n_blocks)
    for rows in (1, 31, 32, 33, 70):
        before = lib.launch_count()
        got = lib.refine(T.from_numpy(x[:rows]).cuda(), packed, n_blocks)
        assert lib.launch_count() == before + 1
        assert got.shape == (rows, D) and _same(got.cpu().numpy(), want[:rows]), (n_blocks, rows)
    if n_blocks == 2:
        assert np.abs(got.cpu().numpy() - gold["mlp_out"]).max() < 5e-6


def _repeated_keypoints(n_frames, K, G, seed):
    """(n_frames, K, 2) patch coordinates, fractional and out of range; rows K // 2 + 1 .. repeat earlier rows bit for bit."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kp = (rng.random((n_frames, K, 2)) * (G + 1.0) - 1.0).astype(np.float32)
    h = K // 2 + 1
    kp[:, h:] = kp[:, :K - h]
    return kp


def test_gather_refine_256_every_launch_form(T, gold, knob):
    """G = 5, K = 33, 2 frames with repeated keypoints: the direct launch, the distinct-row work list with its duplicate copy, and
    the entry without a workspace - all the oracle's bits; then the reference-held frame."""
    from sslam_amd import lib
    sd, packed = _packed(T, 2)
    G, K, n = 5, 33, 2
    feat = ora.bn_tokens(synth.token_sequence(n, G), group=1, train=True)[0].reshape(n, G, G, 384)
    kp = _repeated_keypoints(n, K, G, 71)
    want = ora.refine(ora.gather(feat, kp), sd)
    assert np.array_equal(want[:, K // 2 + 1:], want[:, :K - K // 2 - 1])
    d_feat, d_kp = T.from_numpy(feat).cuda(), T.from_numpy(kp).cuda()
    knob("SSLAM_REFINE_DISTINCT", 0)
    assert lib.lib().sslam_gather_refine_workspace_bytes(n, K) == 0
    got = lib.gather_refine(d_feat, d_kp, packed, 2)
    assert got.shape == (n, K, D) and _same(got.cpu().numpy(), want), "direct launch"
    knob("SSLAM_REFINE_DISTINCT", 1)
    need = int(lib.lib().sslam_gather_refine_workspace_bytes(n, K))
    assert need > 0
    ws = T.zeros(need, dtype=T.uint8, device="cuda")
    before = lib.launch_count()
    got = lib.gather_refine(d_feat, d_kp, packed, 2, out=T.full((n, K, D), float("nan"), device="cuda"), workspace=ws)
    assert lib.launch_count() == before + 4, "rep, list, MLP over the list, duplicate copy"
    assert _same(got.cpu().numpy(), want), "work-list launch"
    counts, total = lib.gather_refine_counts(ws, n)
    assert counts.tolist() == [K // 2 + 1] * n and int(total) == n * (K // 2 + 1), "the repeated rows did not run the MLP"
    out = T.full((n, K, D), float("nan"), device="cuda")
    lib._run("gather_refine_d", lib.lib().sslam_gather_refine_d, (d_feat, d_kp, packed, out), lib._dp(d_feat), n, G, lib._dp(d_kp), K,
             lib._dp(packed), 2, lib._dp(out), D)
    assert _same(out.cpu().numpy(), want), "entry without a workspace"
    # the reference's own DescriptorRefiner(384, 384, 256, 4) on one gathered frame
    g = cases.GATHER_GRID
    f8 = ora.bn_tokens(cases.gather_tokens(), group=1, train=True)[0].reshape(1, g, g, 384)
    got = lib.gather_refine(T.from_numpy(f8).cuda(), T.from_numpy(cases.gather_keypoints()).cuda(), packed, 2).cpu().numpy()
    assert _same(got, ora.refine(ora.gather(f8, cases.gather_keypoints()), sd))
    assert np.abs(got[0] - gold["gather_desc"]).max() < 5e-6


# ------------------------------------------------------------------------------------------------ similarity / arg-max
SHAPES = [(1, 1), (2, 1), (63, 65), (64, 64), (128, 129), (129, 127), (200, 190)]
_SIM = {}


def _three_pairs(n1, n2):
    """Three pairs of (n1, 256) x (n2, 256) with duplicated rows on both sides (exact ties), and the oracle's answer per pair."""
    key = (n1, n2)
    if key not in _SIM:
        d1s, d2s, want = [], [], []
        for p in range(3):
            dup = min(n1, n2) // 8 * 2
            a, b, *_ = cases.pair(100 * n1 + n2 + p, n1, n2, dup) if n1 > 1 else (synth.unit_descriptors(p, 1, D), synth.unit_descriptors(9 + p, n2, D))
            d1s.append(a)
            d2s.append(b)
            nn12, s12, nn21, s21 = ora.sim_argmax(a, b)
            S = ora.sim_matrix(a, b)
            assert _same(S.max(axis=1), s12) and np.array_equal(S.argmax(axis=1), nn12)      # first maximum
            rest = S.copy()
            rest[np.arange(n1), nn12] = -np.inf
            want.append(dict(nn12=nn12, s12=s12, nn21=nn21, s21=s21, second=rest.max(axis=1)))
        _SIM[key] = (np.stack(d1s), np.stack(d2s), want)
    return _SIM[key]


def _check_sim(got, want, where, second=True, cols=True):
    nn12, s12, nn21, s21, sec = (None if t is None else t.cpu().numpy() for t in got)
    for p, w in enumerate(want):
        assert np.array_equal(nn12[p], w["nn12"]) and _same(s12[p], w["s12"]), (where, p, "rows")
        if cols:
            assert np.array_equal(nn21[p], w["nn21"]) and _same(s21[p], w["s21"]), (where, p, "columns")
        if second:
            assert _same(sec[p], w["second"]), (where, p, "runner-up")


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_sim_argmax_256_every_form(T, knob, n1, n2):
    from sslam_amd import lib
    d1, d2, want = _three_pairs(n1, n2)
    if min(n1, n2) >= 8:
        assert any((w["s12"][:, None] == ora.sim_matrix(d1[p], d2[p])).sum(axis=1).max() > 1 for p, w in enumerate(want)), "no exact tie in the case"
    a, b = T.from_numpy(d1).cuda(), T.from_numpy(d2).cuda()
    ws = T.zeros(3 * n2 * 8, dtype=T.uint8, device="cuda")
    for variant, name in ((1, "two-direction"), (2, "single-evaluation")):
        knob("SSLAM_M1_VARIANT", variant)
        for second in (True, False):
            got = lib.sim_argmax(a, n1 * D, n1, b, n2 * D, n2, 3, want_s21=True, want_second=second, workspace=ws)
            assert (got[4] is not None) == second
            _check_sim(got, want, (name, n1, n2, second), second=second)
    for second in (True, False):
        r = lib.sim_argmax_rows(a, n1 * D, n1, b, n2 * D, n2, 3, want_second=second)
        _check_sim((r[0], r[1], None, None, r[2]), want, ("rows-only", n1, n2, second), second=second, cols=False)
    # stride 0 broadcasts the first operand: pair p = frame 0 of d1 against frame p of d2
    got = lib.sim_argmax(a, 0, n1, b, n2 * D, n2, 3, want_s21=True)
    _check_sim(got[:4] + (None,), [want[0]], "stride 0", second=False)


@pytest.mark.parametrize("variant", [1, 2])
def test_sim_argmax_pairs_256_with_an_absent_pair(T, knob, variant):
    from sslam_amd import lib
    k = 129
    d1, d2, _ = _three_pairs(k, k)
    bank = np.concatenate([d1, d2])                      # frames 0..2 and 3..5
    first, second = [0, 4, -1, 2, 5], [3, 1, 2, 2, 0]
    want = []
    for f, s in zip(first, second):
        if f < 0:
            z = np.zeros(k, np.float32)
            want.append(dict(nn12=np.zeros(k, np.int32), s12=z, nn21=np.zeros(k, np.int32), s21=z, second=z))
            continue
        nn12, s12, nn21, s21 = ora.sim_argmax(bank[f], bank[s])
        rest = ora.sim_matrix(bank[f], bank[s])
        rest[np.arange(k), nn12] = -np.inf
        want.append(dict(nn12=nn12, s12=s12, nn21=nn21, s21=s21, second=rest.max(axis=1)))
    knob("SSLAM_M1_VARIANT", variant)
    d_bank = T.from_numpy(bank).cuda()
    f, s = (T.tensor(v, dtype=T.int32, device="cuda") for v in (first, second))
    got = lib.sim_argmax_pairs(d_bank, f, s, want_s21=True, want_second=True)
    _check_sim(got, want, ("pairs", variant))
    r = lib.sim_argmax_rows_pairs(d_bank, f, s, want_second=True)
    _check_sim((r[0], r[1], None, None, r[2]), want, "rows pairs", cols=False)


@pytest.mark.parametrize("variant", [1, 2])
def test_upper_half_of_the_dimensions_decides(T, knob, variant):
    """Every candidate agrees exactly in dimensions 0..127 and differs only in 128..255 (and likewise the queries): a kernel that
    dropped, repeated or reordered the upper half would fail on the INDICES here."""
    from sslam_amd import lib
    n1, n2 = 70, 130
    rng = np.random.Generator(np.random.PCG64(7))
    lo = rng.standard_normal(128).astype(np.float32)
    hi = synth.unit_descriptors(5, n2, 128)
    d2 = np.concatenate([np.broadcast_to(lo, (n2, 128)), 8.0 * hi], axis=1)
    d2 = np.ascontiguousarray(d2 / np.float32(np.sqrt(128.0 + 64.0)), np.float32)
    perm = rng.permutation(n2)[:n1]
    d1 = d2[perm] + np.concatenate([np.zeros((n1, 128), np.float32), 0.05 * rng.standard_normal((n1, 128)).astype(np.float32)], axis=1)
    d1 = np.ascontiguousarray(d1, np.float32)
    assert np.array_equal(d2[:, :128], np.broadcast_to(d2[0, :128], (n2, 128))) and np.array_equal(d1[:, :128], d2[perm][:, :128])
    nn12, s12, nn21, s21 = ora.sim_argmax(d1, d2)
    assert np.array_equal(nn12, perm), "the case is meant to be decided by the upper half"
    low_only = ora.sim_argmax(np.ascontiguousarray(d1[:, :128]), np.ascontiguousarray(d2[:, :128]))[0]
    assert not low_only.any(), "on the lower half alone every candidate ties: the first wins"
    knob("SSLAM_M1_VARIANT", variant)
    a, b = T.from_numpy(d1).cuda(), T.from_numpy(d2).cuda()
    # 16 pairs: the batch size at which the library itself takes the single-evaluation form
    got = lib.sim_argmax(a, 0, n1, b, 0, n2, 16, want_s21=True)
    for p in (0, 7, 15):
        assert np.array_equal(got[0][p].cpu().numpy(), nn12) and _same(got[1][p].cpu().numpy(), s12)
        assert np.array_equal(got[2][p].cpu().numpy(), nn21) and _same(got[3][p].cpu().numpy(), s21)


# ------------------------------------------------------------------------------------------------ M1 - M5
@pytest.mark.parametrize("tag", list(cases.PAIRS))
def test_matchers_256_through_matching_py(T, gold, tag):
    import matching
    seed, n, m, dup = cases.PAIRS[tag]
    d1, d2, s1, s2, i1, i2 = cases.pair(seed, n, m, dup)
    for rtag, kw in cases.RUNS.items():
        mt, q = matching.match_with_quality(d1, d2, s1, s2, **kw(i1, i2))
        assert mt.dtype == np.int64 and np.array_equal(mt, gold[f"{tag}_{rtag}_matches"]), (tag, rtag)
        assert _same(q, ora.match_with_quality(d1, d2, s1, s2, **kw(i1, i2))[1]), (tag, rtag)
    m2 = matching.find_matches(d1, d2, cases.M2_RATIO)
    assert np.array_equal(np.array([(a, b) for a, b, _ in m2], np.int64).reshape(-1, 2), gold[f"{tag}_m2_ij"])
    assert _same(np.array([c for *_, c in m2], np.float32), np.array([c for *_, c in ora.find_matches_m2(d1, d2, cases.M2_RATIO)], np.float32))
    m4, dist = matching.find_mutual_nearest_neighbors(d1, d2, cases.M4_RATIO)
    assert np.array_equal(m4, gold[f"{tag}_m4_matches"]) and _same(np.asarray(dist, np.float32), ora.find_mnn_m4(d1, d2, cases.M4_RATIO)[1])
    assert matching.count_tracked(d1, d2, cases.M5_THRESHOLD) == int(gold[f"{tag}_m5_count"])


def test_matchers_refuse_other_widths(T):
    import matching
    from sslam_amd import lib
    d64, d128, d256 = (synth.unit_descriptors(1, 8, w) for w in (64, 128, 256))
    before = lib.launch_count()
    for a, b in ((d64, d64), (d128, d256), (d256, d128)):
        with pytest.raises(lib.SslamHipError, match=r"128, 256"):
            matching.find_matches(a, b)
        with pytest.raises(lib.SslamHipError, match=r"128, 256"):
            matching.find_matches_batched(T.from_numpy(a)[None], T.from_numpy(b)[None])
    assert lib.launch_count() == before


@pytest.fixture(scope="module")
def pipe256(T):
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    return SequencePipeline(ExtractorConfig(input_size=128, num_keypoints=40), synth.selector_state(0), cases.refiner_state(), device="cuda")


def test_m3_and_the_rules_256_through_the_pipeline(T, gold, pipe256):
    """The B = 4 batch of the reference's _find_matches; the same eight frames as a bank through SequencePipeline.match_pairs and
    .match under M1 and the three rules, against the oracle."""
    import match_rules_cases as mc
    import matching
    from sslam_amd.pipeline import MatchRule
    b1, b2 = (np.stack(x) for x in zip(*[cases.pair(seed, 200, 200, 10, noise)[:2] for seed, noise in cases.M3_CASES]))
    got = matching.find_matches_batched(T.from_numpy(b1).cuda(), T.from_numpy(b2).cuda()).cpu().numpy()
    want = gold["m3_matches"]
    assert got.shape[0] == 4 and np.array_equal(got, want[:, :got.shape[1]]) and not want[:, got.shape[1]:].any()
    bank = np.empty((8, 200, D), np.float32)
    bank[0::2], bank[1::2] = b1, b2
    rng = np.random.Generator(np.random.PCG64(3))
    sc, inten = rng.random((8, 200)).astype(np.float32), rng.random((8, 200)).astype(np.float32)
    d_bank, d_sc, d_in = (T.from_numpy(x).cuda() for x in (bank, sc, inten))
    cfg = pipe256.cfg
    first, second = [0, 2, -1, 4, 6, 1], [1, 3, 0, 5, 7, 0]

    def m1(i, j):
        return ora.match_with_quality(bank[i], bank[j], sc[i], sc[j], cfg.saliency_weight, cfg.min_saliency, cfg.min_descriptor_sim,
                                      inten[i], inten[j], cfg.min_intensity)

    def check(res, pairs, want_fn, value="quality"):
        r = {k: res[k].cpu().numpy() for k in ("matches", value, "match_count")}
        total = 0
        for row, (i, j) in enumerate(pairs):
            wm, wv = (np.zeros((0, 2), np.int64), np.zeros(0, np.float32)) if i < 0 else want_fn(i, j)
            c = int(r["match_count"][row])
            assert c == len(wm) and np.array_equal(r["matches"][row, :c], wm) and _same(r[value][row, :c], np.asarray(wv, np.float32)), (row, i, j)
            assert not r["matches"][row, c:].any() and not _bits(r[value][row, c:]).any()
            total += c
        return total

    assert check(pipe256.match_pairs(d_bank, d_sc, d_in, first=first, second=second), list(zip(first, second)), m1) > 0
    assert check(pipe256.match(d_bank, d_sc, d_in, spacing=1), [(i, i + 1) for i in range(7)], m1) > 0
    for name, param in ((mc.RATIO, cases.M2_RATIO), (mc.MNN_RATIO, cases.M4_RATIO), (mc.TRACKED, cases.M5_THRESHOLD)):
        rule = getattr(MatchRule, name)(param)
        fn = lambda i, j: mc.oracle_rule(name, bank[i], bank[j], param)
        assert check(pipe256.match_pairs(d_bank, d_sc, d_in, first=first, second=second, rule=rule), list(zip(first, second)), fn, "value") > 0
        check(pipe256.match(d_bank, d_sc, spacing=2, rule=rule), [(i, i + 2) for i in range(6)], fn, "value")      # unrelated frames
    with pytest.raises(ValueError, match="256"):
        pipe256.match(d_bank[:, :, :128].contiguous(), d_sc)


# ------------------------------------------------------------------------------------------------ pipeline, tokens in
N_SEQ, G_SEQ, K_SEQ = 5, 8, 40
FRAME_KEYS = ("idx", "scores", "descriptors", "intensity")


@pytest.fixture(scope="module")
def seq256(T, pipe256):
    import oracle_check
    toks, imgs = synth.token_sequence(N_SEQ, G_SEQ), synth.image_sequence(N_SEQ, 96, 128)
    o = {sp: oracle_check.oracle_block(imgs, toks, synth.selector_state(0), cases.refiner_state(), 16 * G_SEQ, K_SEQ,
                                       type(pipe256.cfg)(input_size=16 * G_SEQ, num_keypoints=K_SEQ, spacing=sp)) for sp in (1, 2)}
    return dict(toks=T.from_numpy(toks).cuda(), imgs=T.from_numpy(imgs).cuda(), oracle=o)


def test_pipeline_256_equals_the_oracle(T, pipe256, seq256):
    import oracle_check
    assert pipe256.descriptor_dim == D
    for n in (3, N_SEQ):                                  # 3 frames at spacing 1, then the sequence the harness tests use
        out = pipe256.run(seq256["imgs"][:n], seq256["toks"][:n])
        assert out["descriptors"].shape == (n, K_SEQ, D)
        o = seq256["oracle"][1]
        part = dict(o, **{k: o[k][:n] for k in FRAME_KEYS}, matches=o["matches"][:n - 1], quality=o["quality"][:n - 1])
        ok, frames, pairs, nm, why = oracle_check.compare_block(part, {k: out[k].cpu().numpy() for k in FRAME_KEYS},
                                                                {k: out[k].cpu().numpy() for k in ("matches", "quality", "match_count")}, 0, K_SEQ)
        assert ok and pairs == n - 1 and nm > 0, why
    idx = seq256["oracle"][1]["idx"]
    assert any(len(set(r.tolist())) < K_SEQ for r in idx), "repeated keypoints are part of the case"


def test_streaming_and_stepper_256_equal_the_batched_run(T, pipe256, seq256):
    from sslam_amd import lib
    from sslam_amd.harness import StreamingSequence
    from sslam_amd.online import FrameStepper
    sp = (1, 2)
    toks, imgs = seq256["toks"], seq256["imgs"]
    want = StreamingSequence(pipe256, sp).run(toks, imgs)
    for s in sp:
        o = seq256["oracle"][s]
        r = {k: want[s][k].cpu().numpy() for k in ("matches", "quality", "match_count")}
        for p, (m, q) in enumerate(zip(o["matches"], o["quality"])):
            c = int(r["match_count"][p])
            assert c == len(m) and np.array_equal(r["matches"][p, :c], m) and _same(r["quality"][p, :c], q), (s, p)
    assert _same(want["frames"]["descriptors"].cpu().numpy(), seq256["oracle"][1]["descriptors"])
    for chunk in (3, 1):
        got = StreamingSequence(pipe256, sp).run(toks, imgs, chunk=chunk)
        for s in sp:
            for key in ("matches", "quality", "match_count", "first"):
                assert T.equal(got[s][key], want[s][key]), (chunk, s, key)
        assert T.equal(got["frames"]["descriptors"], want["frames"]["descriptors"])
    ring = StreamingSequence(pipe256, sp)
    outs = [ring.push(toks[a:a + 3], imgs[a:a + 3]) for a in range(0, N_SEQ, 3)]
    assert ring._ring["descriptors"].shape == (2, K_SEQ, D)
    for s in sp:
        for key in ("matches", "quality", "match_count"):
            assert T.equal(T.cat([o[s][key] for o in outs if s in o]), want[s][key]), (s, key)
    for use_graph in (False, True):
        st = FrameStepper(pipe256, 96, 128, use_graph=use_graph, tokens_in=True, spacings=sp)
        assert st.bank["descriptors"].shape == (3, K_SEQ, D)
        for rnd in range(2):
            for t in range(N_SEQ):
                n0 = lib.launch_count()
                o = st.step(imgs[t], toks[t])
                if use_graph and (rnd or t):
                    assert lib.launch_count() == n0, "a replayed step issues no library call"
                for k in ("idx", "descriptors", "intensity", "scores"):
                    assert T.equal(o[k], want["frames"][k][t]), (use_graph, k, t)
                for row, s in enumerate(sp):
                    if t < s:
                        assert int(o["match_count"][row]) == 0 and not o["matches"][row].any()
                    else:
                        for key in ("matches", "quality", "match_count"):
                            assert T.equal(o[key][row], want[s][key][t - s]), (use_graph, key, t, s)
            st.reset()


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("n1,n2", [(1, 1), (255, 300), (257, 64)])
def test_row_lse_256(T, n1, n2):
    from sslam_amd import lib
    temperature = 0.1
    d1 = np.stack([synth.unit_descriptors(40 + p, n1, D) for p in range(2)])
    d2 = np.stack([synth.unit_descriptors(50 + p, n2, D, dup=n2 // 8) for p in range(2)])
    if n1 > 1:
        d1[:, :8] = d2[:, :8]                      # rows whose best logit is 1 / T
    a, b = T.from_numpy(d1).cuda(), T.from_numpy(d2).cuda()
    nn12, s12, nn21, _, _ = lib.sim_argmax(a, n1 * D, n1, b, n2 * D, n2, 2)
    lse, ce, s00 = lib.row_lse(a, n1 * D, n1, b, n2 * D, n2, 2, s12, temperature)
    for p in range(2):
        ref = val_ref.row_lse(d1[p], d2[p], temperature)
        x = val_ref.logits(d1[p], d2[p], temperature)
        scale = np.maximum(np.abs(ref), 1.0 / temperature)
        err = np.abs(lse[p].cpu().numpy() - ref)
        print(f"row_lse 256 ({n1}, {n2}) pair {p}: max |lse - ref| {err.max():.3e}, tolerance there {val_ref.tolerance(ref, scale=scale)[err.argmax()]:.3e}")
        assert (err <= val_ref.tolerance(ref, scale=scale)).all()
        cref = ref - x.max(axis=1)
        assert (np.abs(ce[p].cpu().numpy() - cref) <= val_ref.tolerance(cref, scale=scale)).all()
        assert _same(s00[p].cpu().numpy(), ora.sim_matrix(d1[p][:1], d2[p][:1])[0, 0])
    if n1 > 1:
        return
    # (1, 1) also as a listed pair of one bank
    f, s = (T.tensor(v, dtype=T.int32, device="cuda") for v in ([0, -1], [1, 0]))
    bank = T.cat([a[0:1], b[0:1]])
    r = lib.sim_argmax_pairs(bank, f, s)
    l2, c2, z2 = lib.row_lse_pairs(bank, f, s, r[1], temperature)
    assert T.equal(l2[0], lse[0]) and T.equal(c2[0], ce[0]) and not l2[1].any() and float(z2[1]) == 0.0


def test_row_lse_pairs_256_equals_the_strided_form(T):
    from sslam_amd import lib
    k = 130
    bank = T.from_numpy(np.stack([synth.unit_descriptors(60 + p, k, D, dup=8) for p in range(3)])).cuda()
    s12 = lib.sim_argmax(bank[:2], k * D, k, bank[1:], k * D, k, 2)[1]
    want = lib.row_lse(bank[:2], k * D, k, bank[1:], k * D, k, 2, s12, 0.05)
    f, s = (T.tensor(v, dtype=T.int32, device="cuda") for v in ([0, -1, 1], [1, 2, 2]))
    r = lib.sim_argmax_pairs(bank, f, s)
    got = lib.row_lse_pairs(bank, f, s, r[1], 0.05)
    for x, y in zip(got, want):
        assert T.equal(x[0].view(T.int32), y[0].view(T.int32)) and T.equal(x[2].view(T.int32), y[1].view(T.int32))
        assert not x[1].view(T.int32).any()


@pytest.mark.parametrize("k", [1, 37])
def test_frame_stats_descriptor_moments_256(T, k):
    from sslam_amd import lib
    n = 2
    sal = np.random.default_rng(k).uniform(0.02, 0.98, (n, 4, 4)).astype(np.float32)
    desc = np.stack([synth.unit_descriptors(70 + f, k, D, 4 if k > 8 else 0) for f in range(n)])
    stats, dmean, dm2 = lib.val_frame_stats(T.from_numpy(sal).cuda(), descriptors=T.from_numpy(desc).cuda())
    assert dmean.shape == dm2.shape == (n, D)
    for f in range(n):
        ref = val_ref.frame_stats(sal[f], None, desc[f])
        assert (np.abs(dmean[f].cpu().numpy() - ref["desc_mean"]) <= val_ref.tolerance(ref["desc_mean"], scale=1.0)).all()      # unit rows
        assert (np.abs(dm2[f].cpu().numpy() - ref["desc_m2"]) <= val_ref.tolerance(ref["desc_m2"])).all()
        assert abs(float(stats[f, lib.VAL_FRAME_SLOTS["sal_mean"]]) - ref["sal_mean"]) <= val_ref.tolerance(ref["sal_mean"])
    if k == 1:
        assert not dm2.cpu().numpy().any(), "one row: the centred sum of squares is exactly 0"


def test_validate_256_on_a_synthetic_sequence(T):
    """validation.validate on its smallest existing configuration (6 frames, input_size 80, 12 keypoints; batches of 4 and 1)
    with a 256-wide refiner, against val_ref.validate on the pipeline's own saliency, descriptors and A0 image."""
    from sslam_amd import validation
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    n, g, k = 6, 5, 12
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k), synth.selector_state(0), cases.refiner_state(), device="cuda")
    toks = T.from_numpy(synth.token_sequence(n, g)).cuda()
    imgs = T.from_numpy(synth.image_sequence(n, 96, 128)).cuda()
    got = validation.validate(pipe, imgs, spacing=1, batch=4, tokens=toks)
    out = pipe.extract(toks, None)
    assert out["descriptors"].shape == (n, k, D)
    first = np.arange(n - 1)
    want = val_ref.validate(out["saliency"].cpu().numpy(), pipe.preprocess(imgs).cpu().numpy(), out["descriptors"].cpu().numpy(), first,
                            first + 1, batch=4, temperature=0.1)
    assert set(got) == set(want)
    for key in want:
        print(f"validate 256 {key:20s} got {got[key]:+.9e} ref64 {want[key]:+.9e} |d| {abs(got[key] - want[key]):.2e}")
    for key in want:
        assert abs(got[key] - want[key]) <= val_ref.tolerance(want[key]), (key, got[key], want[key])
    stats = pipe.validation_stats(out, imgs, spacing=1)
    assert stats["desc_mean"].shape == stats["desc_m2"].shape == (n, D)


# ------------------------------------------------------------------------------------------------ the drop-in module, bf16
def test_dropin_refiner_256_runs_the_kernel(T):
    from models.descriptor_refiner import DescriptorRefiner
    from sslam_amd import lib
    T.manual_seed(0)
    ref = DescriptorRefiner(384, 384, 256).cuda().eval()
    x = T.randn(2, 50, 384, device="cuda")
    before = lib.launch_count()
    with T.no_grad(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        d = ref(x)
    assert not [w for w in caught if "eager" in str(w.message)], "a 256-wide refiner must not fall back"
    assert lib.launch_count() > before, "the 256-wide refiner must run the HIP kernel"
    sd = {k: v.detach().cpu().numpy() for k, v in ref.state_dict().items()}
    assert d.shape == (2, 50, 256) and _same(d.cpu().numpy(), ora.refine(x.cpu().numpy(), sd, len(ref.residual_blocks)))
    with T.no_grad(), pytest.warns(UserWarning, match="eager torch path"):
        DescriptorRefiner(384, 384, 64).cuda().eval()(x)


def test_bf16_mode_refuses_a_256_wide_refiner(T):
    from sslam_amd import lib
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    with pytest.raises(lib.SslamHipError, match=r"bf16.*256|256.*bf16"):
        SequencePipeline(ExtractorConfig(precision="bf16"), synth.selector_state(0), cases.refiner_state(), device="cuda")
    SequencePipeline(ExtractorConfig(precision="bf16"), synth.selector_state(0), synth.refiner_state(0), device="cuda")


# ------------------------------------------------------------------------------------------------ D = 128 through both entries
def test_width_128_through_the_old_and_the_new_entry(T):
    """One refine call and one sim_argmax call through the entry without a width and through its _d form with d = 128:
    identical bytes (they launch the same kernel)."""
    from sslam_amd import lib
    L = lib.lib()
    st = ctypes.c_void_p(T.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    sd = synth.refiner_state(0)
    packed = T.from_numpy(lib.pack_refiner(ora.refiner_weight_list(sd, 2), 2)).cuda()
    x = T.from_numpy(cases.mlp_rows()).cuda()
    old, new = (T.full((70, 128), float("nan"), device="cuda") for _ in range(2))
    assert L.sslam_refine(p(x), 70, p(packed), 2, p(old), st) == 0
    assert L.sslam_refine_d(p(x), 70, p(packed), 2, p(new), 128, st) == 0
    assert T.equal(old.view(T.int32), new.view(T.int32)) and _same(old.cpu().numpy(), ora.refine(cases.mlp_rows(), sd))
    n1, n2 = 129, 127
    d1 = T.from_numpy(np.stack([synth.unit_descriptors(80 + i, n1, 128, 8) for i in range(3)])).cuda()
    d2 = T.from_numpy(np.stack([synth.unit_descriptors(90 + i, n2, 128, 8) for i in range(3)])).cuda()
    outs = []
    for entry, width in ((L.sslam_sim_argmax, ()), (L.sslam_sim_argmax_d, (128,))):
        nn12, nn21 = T.full((3, n1), -7, dtype=T.int32, device="cuda"), T.full((3, n2), -7, dtype=T.int32, device="cuda")
        s12, sec, s21 = T.zeros((3, n1), device="cuda"), T.zeros((3, n1), device="cuda"), T.zeros((3, n2), device="cuda")
        assert entry(p(d1), n1 * 128, n1, p(d2), n2 * 128, n2, 3, p(nn12), p(s12), p(nn21), p(s21), p(sec), *width, st) == 0
        outs.append((nn12, s12, nn21, s21, sec))
    for a, b in zip(*outs):
        assert T.equal(a.view(T.int32), b.view(T.int32))
    want = ora.sim_argmax(d1[1].cpu().numpy(), d2[1].cpu().numpy())
    assert np.array_equal(outs[1][0][1].cpu().numpy(), want[0]) and _same(outs[1][1][1].cpu().numpy(), want[1])
