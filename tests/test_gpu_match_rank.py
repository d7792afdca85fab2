"""GPU tests of the ranking stage: sslam_match_rank through sslam_amd.lib, matching.best_matches, SequencePipeline.rank_matches,
harness.rank_result and online.RankedFrameStepper.  Everything is BIT FOR BIT against tests/match_rank_cases.rank_ref - rows,
value bits, counts, slots, zeroed tails - and there are no tolerances in this file.  The shapes are the smallest at which the
kernel can go wrong: one element, one wave, one workgroup's stride, the powers of two on both sides of every merge size, and the
LDS limit of 4096 rows."""
import numpy as np
import pytest

import match_rank_cases as rc
import synth

pytestmark = pytest.mark.gpu

N = 27
GUARD_I, GUARD_F = -7, np.float32(-123.5)


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _rank(T, m, v, c, best, ascending=False, want_slot=True):
    """One launch over numpy inputs, every output lying between two guard rows that must come back untouched.
    -> (matches, value, count, slot or None) as numpy."""
    from sslam_amd import lib
    p = v.shape[0]
    dm, dv, dc = (T.from_numpy(np.ascontiguousarray(x)).cuda() for x in (m, v, np.asarray(c, np.int32)))
    om = T.full((p + 2, best, 2), GUARD_I, dtype=T.int64, device="cuda")
    ov = T.full((p + 2, best), float(GUARD_F), dtype=T.float32, device="cuda")
    oc = T.full((p + 2,), GUARD_I, dtype=T.int32, device="cuda")
    osl = T.full((p + 2, best), GUARD_I, dtype=T.int32, device="cuda") if want_slot else None
    n0 = lib.launch_count()
    got = lib.match_rank(dm, dv, dc, best, ascending=ascending, want_slot=want_slot,
                         out=(om[1:p + 1], ov[1:p + 1], oc[1:p + 1], None if osl is None else osl[1:p + 1]))
    assert lib.launch_count() - n0 == 1, "one launch"
    assert got[3] is None or want_slot
    for buf, guard in ((om, GUARD_I), (ov, GUARD_F), (oc, GUARD_I)) + (((osl, GUARD_I),) if want_slot else ()):
        h = buf.cpu().numpy()
        assert (h[0] == guard).all() and (h[-1] == guard).all(), "a guard row was written"
    assert T.equal(dm, T.from_numpy(np.ascontiguousarray(m)).cuda()) and T.equal(dc, T.from_numpy(np.asarray(c, np.int32)).cuda())
    return (om[1:p + 1].cpu().numpy(), ov[1:p + 1].cpu().numpy(), oc[1:p + 1].cpu().numpy(), None if osl is None else osl[1:p + 1].cpu().numpy())


def _check(got, want, where, slot=True):
    gm, gv, gc, gs = got
    wm, wv, wc, ws = want
    assert gc.dtype == np.int32 and np.array_equal(gc, wc), (where, gc.tolist()[:8], wc.tolist()[:8])
    assert gm.dtype == np.int64 and np.array_equal(gm, wm), where
    assert rc.same_bits(gv, wv), where
    if slot:
        assert gs.dtype == np.int32 and np.array_equal(gs, ws), where


# ------------------------------------------------------------------------------------------------ 1. raw entry: sizes
@pytest.mark.parametrize("n1", rc.N_SWEEP)
def test_n1_sweep(T, n1):
    counts = [0, 1, n1 // 2, n1] + [int(x) for x in np.random.default_rng(n1).integers(0, n1 + 1, 2)]
    v = rc.random_values(n1, len(counts), n1)
    m = rc.slot_matches(len(counts), n1)
    for best in sorted({n1, max(1, n1 // 3)}):
        for asc in (False, True):
            _check(_rank(T, m, v, counts, best, asc), rc.rank_ref(m, v, counts, best, asc), (n1, best, asc))
    distinct = np.random.default_rng(n1 + 1).permutation(n1).astype(np.float32)[None]      # no ties: every exchange moves a key
    _check(_rank(T, m[:1], distinct, [n1], n1), rc.rank_ref(m[:1], distinct, [n1], n1), (n1, "distinct"))


def test_count_words_outside_the_range_are_clamped(T):
    n1 = 70
    counts = [-5, n1 + 7, -2 ** 31, 2 ** 31 - 1, 0, n1]
    v = rc.random_values(5, len(counts), n1)
    m = rc.slot_matches(len(counts), n1)
    for best in (n1, 9):
        got = _rank(T, m, v, counts, best)                     # the guard rows around every output are checked in there
        _check(got, rc.rank_ref(m, v, counts, best), best)
        assert got[2].tolist() == [0, best, 0, best, 0, best]


# ----------------------------------------------------------------------------------------------- 2. value patterns
@pytest.mark.parametrize("ascending", [False, True], ids=["descending", "ascending"])
@pytest.mark.parametrize("n1", [64, 300, 1000])
def test_value_patterns(T, n1, ascending):
    """Every pattern is one pair of the launch.  300 and 1000 put equal values on both sides of lane 63 | 64 and of slot
    255 | 256: the slot order must hold across a wave and across a workgroup's stride."""
    pats = rc.value_patterns(n1)
    names = sorted(pats)
    v = np.stack([pats[k] for k in names])
    m = rc.slot_matches(len(names), n1)
    for counts in ([n1] * len(names), [n1 - 3 if n1 > 3 else 1] * len(names)):
        got = _rank(T, m, v, counts, n1, ascending)
        want = rc.rank_ref(m, v, counts, n1, ascending)
        for row, name in enumerate(names):
            _check(tuple(x[row:row + 1] for x in got), tuple(x[row:row + 1] for x in want), (name, n1, ascending, counts[0]))
    c = counts[0]
    row = names.index("all_equal")
    assert np.array_equal(got[3][row, :c], np.arange(c)), "all equal: the output is the input order"
    row = names.index("ascending" if ascending else "descending")
    assert np.array_equal(got[3][row, :c], np.arange(c)), "already in order"
    row = names.index("nans")
    k = int((~np.isnan(v[row, :c])).sum())
    assert 0 < k < c and not np.isnan(got[1][row, :k]).any() and np.isnan(got[1][row, k:c]).all(), "NaN rows come last"
    assert np.all(np.diff(got[3][row, k:c]) > 0), "in slot order"


# ---------------------------------------------------------------------------------------------------------- 3. best
@pytest.mark.parametrize("n1,count", [(300, 200), (64, 64), (5, 2)])
def test_best_around_the_count(T, n1, count):
    v = rc.random_values(11, 3, n1)
    m = rc.slot_matches(3, n1)
    counts = [count, max(count - 1, 0), min(count + 1, n1)]
    for best in sorted({1, max(count - 1, 1), count, min(count + 1, n1), n1}):
        want = rc.rank_ref(m, v, counts, best)
        got = _rank(T, m, v, counts, best)
        _check(got, want, (n1, count, best))
        lean = _rank(T, m, v, counts, best, want_slot=False)   # out_slot NULL: the same rows
        assert lean[3] is None
        _check(lean, want, (n1, count, best, "no slot"), slot=False)
        for p in range(3):
            kept = int(got[2][p])
            assert kept == min(counts[p], best)
            assert np.array_equal(m[p][got[3][p, :kept]], got[0][p, :kept]), "matches[out_slot] == out_matches"
            assert rc.same_bits(v[p][got[3][p, :kept]], got[1][p, :kept])
            assert not got[0][p, kept:].any() and not got[1][p, kept:].view(np.uint32).any() and not got[3][p, kept:].any()


# ---------------------------------------------------------------------------------------------------- 4. pair counts
@pytest.mark.parametrize("n_pairs", [1, 3, 70000])
def test_pair_counts(T, n_pairs):
    """70 000 pairs of 8 rows: past any 16-bit grid dimension.  Every seventh pair is absent (count 0: zero rows); the same launch
    twice gives the same bytes."""
    from sslam_amd import lib
    n1, best = 8, 5
    v = rc.random_values(n_pairs, n_pairs, n1)
    m = rc.slot_matches(n_pairs, n1)
    counts = (np.arange(n_pairs) * 5 + 3) % (n1 + 1)
    counts[::7] = 0
    counts = counts.astype(np.int32)
    dm, dv, dc = (T.from_numpy(x).cuda() for x in (m, v, counts))
    a = lib.match_rank(dm, dv, dc, best)
    b = lib.match_rank(dm, dv, dc, best)
    for x, y in zip(a, b):
        assert T.equal(x.view(T.int32), y.view(T.int32))
    want = rc.rank_ref(m, v, counts, best)
    _check(tuple(x.cpu().numpy() for x in a), want, n_pairs)
    absent = T.from_numpy(counts == 0).cuda()
    assert not a[0][absent].any() and not a[1][absent].view(T.int32).any() and not a[2][absent].any()
    assert n_pairs < 3 or (int(a[2][-1]) == min(int(counts[-1]), best) and int(a[2].sum()) == int(want[2].sum()) > 0)


# ------------------------------------------------------------------------------------------- 5. reference-held lists
def test_reference_m1_lists(T):
    """The 60 lists of the reference's own match_with_quality: through matching.best_matches at the reference's two defaults and
    at the whole list, and through lib.match_rank in one launch, against what tests/test_match_rank_api.py derives from the same
    arrays on the CPU (the largest qualities bit for bit; np.argsort(-q)'s rows where the qualities are distinct)."""
    import matching
    from sslam_amd import lib
    pairs = rc.m1_pairs()
    assert len(pairs) == 60
    n1 = max(len(q) for _, _, q in pairs)
    m = np.zeros((60, n1, 2), np.int64)
    v = np.zeros((60, n1), np.float32)
    c = np.array([len(q) for _, _, q in pairs], np.int32)
    for p, (_, mt, q) in enumerate(pairs):
        m[p, :len(q)], v[p, :len(q)] = mt, q
    for best in (50, 100, n1):
        _check(_rank(T, m, v, c, best), rc.rank_ref(m, v, c, best), best)
    for tag, mt, q in pairs:
        for max_matches in (50, 100, len(q)):
            gm, gq = matching.best_matches(mt, q, max_matches)
            kept = min(len(q), max_matches)
            assert gm.dtype == np.int64 and gm.shape == (kept, 2) and gq.shape == (kept,)
            assert rc.same_bits(gq, np.sort(q)[::-1][:kept]), (tag, max_matches)
            wm, wv, _, _ = rc.rank_ref(*rc.padded(mt, q), kept)
            assert np.array_equal(gm, wm[0]) and rc.same_bits(gq, wv[0]), (tag, max_matches)
            if len(np.unique(q)) == len(q):
                assert np.array_equal(gm, mt[np.argsort(-q)[:kept]]), (tag, max_matches)
    dm, dq = matching.best_matches(T.from_numpy(pairs[0][1]).cuda(), T.from_numpy(pairs[0][2]).cuda())      # tensors in, tensors out
    assert dm.is_cuda and dq.is_cuda and np.array_equal(dm.cpu().numpy(), matching.best_matches(pairs[0][1], pairs[0][2])[0])
    em, ev = matching.best_matches(np.zeros((0, 2), np.int64), np.zeros((0,), np.float32))
    assert em.shape == (0, 2) and ev.shape == (0,)
    n0 = lib.launch_count()
    with pytest.raises(ValueError):
        matching.best_matches(pairs[0][1], pairs[0][2], 0)
    assert lib.launch_count() == n0


def test_reference_m2_and_m4_lists(T):
    import matching
    for tag, ij, sim in rc.rule_lists("m2"):
        want = sorted([(int(a), int(b), s) for (a, b), s in zip(ij, sim)], key=lambda x: x[2], reverse=True)[:100]
        gm, gs = matching.best_matches(ij, sim)                 # visualize_matches.py:150-151 at its default
        assert [tuple(r) for r in gm.tolist()] == [(a, b) for a, b, _ in want], tag
        assert rc.same_bits(gs, np.array([s for *_, s in want], np.float32)), tag
        _check(_rank(T, *rc.padded(ij, sim), len(sim)), rc.rank_ref(*rc.padded(ij, sim), len(sim)), tag)
    for tag, mt, dist in rc.rule_lists("m4"):
        gm, gd = matching.best_matches(mt, dist, max(len(dist), 1), ascending=True)      # one of the lists is empty
        order = np.argsort(dist, kind="stable")
        assert np.array_equal(gm, mt[order].reshape(-1, 2)) and rc.same_bits(gd, dist[order]), tag
        wide = rc.padded(mt, dist, max(len(dist) + 9, 100))
        _check(_rank(T, *wide, 100, True), rc.rank_ref(*wide, 100, True), tag)


# ------------------------------------------------------------------------------------------------------ 6. pipeline
@pytest.fixture(scope="module")
def pipe(T):
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    return SequencePipeline(ExtractorConfig(saliency_weight=0.3, min_saliency=0.5, min_descriptor_sim=0.7, min_intensity=0.15),
                            synth.selector_state(0), synth.refiner_state(0), device="cuda")


@pytest.fixture(scope="module")
def seq(T, pipe):
    toks = T.from_numpy(synth.token_sequence(N, 28)).cuda()
    imgs = T.from_numpy(synth.image_sequence(N)).cuda()
    return dict(toks=toks, imgs=imgs, ex=pipe.extract(toks, imgs))


def _rules():
    from sslam_amd.pipeline import MatchRule
    import match_rules_cases as mc
    return [None] + [getattr(MatchRule, name)(mc.MIDDLE[name]) for name in (mc.RATIO, mc.MNN_RATIO, mc.TRACKED)]


def _ref_of(res, rule, best):
    from sslam_amd import lib
    val = "quality" if rule is None else "value"
    asc = rule is not None and rule.kind == lib.RULE_RATIO_SECOND
    return rc.rank_ref(res["matches"].cpu().numpy(), res[val].cpu().numpy(), res["match_count"].cpu().numpy(), best, asc)


def _check_ranked(ranked, want, rule, where):
    val = "quality" if rule is None else "value"
    assert set(ranked) == {"matches", val, "match_count", "slot"}, where
    _check(tuple(ranked[k].cpu().numpy() for k in ("matches", val, "match_count", "slot")), want, where)


@pytest.mark.parametrize("rule_index", range(4), ids=["m1", "ratio", "mnn_ratio", "tracked"])
def test_rank_matches_of_match_and_match_pairs(T, pipe, seq, rule_index):
    from sslam_amd import lib
    rule = _rules()[rule_index]
    kw = {} if rule is None else {"rule": rule}
    val = "quality" if rule is None else "value"
    ex = seq["ex"]
    res = pipe.match(ex["descriptors"], ex["scores"], ex["intensity"], spacing=1, **kw)
    before = {k: v.clone() for k, v in res.items()}
    total = int(res["match_count"].sum())
    assert 0 < total < (N - 1) * 500
    for best in (50, 500, None):
        n0 = lib.launch_count()
        ranked = pipe.rank_matches(res, best, **kw)
        assert lib.launch_count() - n0 == 1
        b = 500 if best is None else best
        assert ranked["matches"].shape == (N - 1, b, 2) and ranked[val].shape == (N - 1, b) and ranked["slot"].dtype == T.int32
        _check_ranked(ranked, _ref_of(res, rule, b), rule, ("match", best))
    for k, v in before.items():
        assert T.equal(res[k].view(T.int32), v.view(T.int32)), (k, "match()'s own outputs are unchanged by a rank call")
    if rule is not None and rule.kind == lib.RULE_RATIO_SECOND:
        d = ranked["value"][0, :int(ranked["match_count"][0])]
        assert bool((d[1:] >= d[:-1]).all()) and float(d[0]) < float(d[-1]), "a distance: the smaller is the better"
    # pair lists: reversed, repeated and absent pairs; out= row slices of alloc_ranked buffers
    first, second = [9, 2, -1, 5, 2, 13, 4, -1, 0], [4, 9, 3, 6, 9, 13, -1, -1, 26]
    resp = pipe.match_pairs(ex["descriptors"], ex["scores"], ex["intensity"], first=first, second=second, **kw)
    bufs = pipe.alloc_ranked(len(first) + 4, 50, **kw)
    for v in bufs.values():
        v.fill_(GUARD_I)
    ranked = pipe.rank_matches(resp, 50, out={k: v[2:2 + len(first)] for k, v in bufs.items()}, **kw)
    _check_ranked(ranked, _ref_of(resp, rule, 50), rule, "match_pairs")
    for k, v in bufs.items():
        assert bool((v[:2] == GUARD_I).all()) and bool((v[2 + len(first):] == GUARD_I).all()), (k, "rows outside the slice")
        assert ranked[k].data_ptr() == v[2:].data_ptr()
    for row, (i, j) in enumerate(zip(first, second)):
        if -1 in (i, j):
            assert int(ranked["match_count"][row]) == 0 and not ranked["matches"][row].any() and not ranked[val][row].view(T.int32).any()
    assert T.equal(ranked["matches"][1], ranked["matches"][4]) and T.equal(ranked["slot"][1], ranked["slot"][4]), "a pair listed twice"


def test_rank_matches_at_descriptor_width_256(T):
    import d256_cases
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    p256 = SequencePipeline(ExtractorConfig(input_size=128, num_keypoints=40), synth.selector_state(0), d256_cases.refiner_state(), device="cuda")
    out = p256.run(T.from_numpy(synth.image_sequence(5, 96, 128)).cuda(), T.from_numpy(synth.token_sequence(5, 8)).cuda())
    assert out["descriptors"].shape == (5, 40, 256) and int(out["match_count"].sum()) > 0
    for best in (7, 40):
        _check_ranked(p256.rank_matches(out, best), _ref_of(out, None, best), None, ("d256", best))
    rule = MatchRule.mnn_ratio()
    res = p256.match(out["descriptors"], out["scores"], spacing=2, rule=rule)
    _check_ranked(p256.rank_matches(res, 10, rule=rule), _ref_of(res, rule, 10), rule, "d256 mnn_ratio")
    with pytest.raises(ValueError, match="best"):
        p256.rank_matches(out, 41)


def test_rank_result_over_spacings(T, pipe, seq):
    from sslam_amd import lib
    from sslam_amd.harness import StreamingSequence, rank_result
    result = StreamingSequence(pipe, (1, 5)).run(seq["toks"], seq["imgs"], chunk=10)
    n0 = lib.launch_count()
    ranked = rank_result(pipe, result, 50)
    assert lib.launch_count() - n0 == 2, "one rank launch per spacing"
    assert set(ranked) == {1, 5}
    for s in (1, 5):
        assert ranked[s]["match_count"].shape == (N - s,)
        _check_ranked(ranked[s], _ref_of(result[s], None, 50), None, s)
        for row in (0, N - s - 1):                             # per-pair ranking: a pair alone gives its rows of the batch
            one = pipe.rank_matches({k: result[s][k][row:row + 1] for k in ("matches", "quality", "match_count")}, 50)
            for k in one:
                assert T.equal(one[k][0].view(T.int32), ranked[s][k][row].view(T.int32)), (s, row, k)


# ------------------------------------------------------------------------------------------------------- 7. online
N_STEP = 6


@pytest.mark.parametrize("spacings", [None, (1, 3)], ids=["one_spacing", "two_spacings"])
@pytest.mark.parametrize("name", [None, "tracked"], ids=["m1", "tracked"])
def test_ranked_stepper(T, pipe, seq, name, spacings):
    """6 steps, as ordinary launches and from the captured graph: "best" is rank_ref of the step's own match arrays, the two forms
    agree bit for bit, and every key the parent stepper returns is what a FrameStepper / RuleFrameStepper returns on the frames."""
    import match_rules_cases as mc
    from sslam_amd import lib
    from sslam_amd.online import FrameStepper, RankedFrameStepper, RuleFrameStepper
    from sslam_amd.pipeline import MatchRule
    rule = None if name is None else MatchRule.tracked(mc.MIDDLE[name])
    val = "quality" if rule is None else "value"
    best = 50
    toks, imgs = seq["toks"][:N_STEP], seq["imgs"][:N_STEP]
    if rule is None:
        parent = FrameStepper(pipe, 480, 640, use_graph=False, tokens_in=True, spacings=spacings)
    else:
        parent = RuleFrameStepper(pipe, 480, 640, use_graph=False, tokens_in=True, spacings=spacings, rule=rule)
    forms = {g: RankedFrameStepper(pipe, 480, 640, use_graph=g, tokens_in=True, spacings=spacings, rule=rule, best=best) for g in (False, True)}
    total = 0
    for t in range(N_STEP):
        po = parent.step(imgs[t], toks[t])
        outs = {}
        for g, st in forms.items():
            n0 = lib.launch_count()
            o = st.step(imgs[t], toks[t])
            assert (lib.launch_count() - n0 == 0) == (g and t > 0), "a replayed step issues no library call"
            assert set(o) == set(po) | {"best"}
            for k, v in po.items():                            # the parent's keys: bit-identical
                if isinstance(v, T.Tensor):
                    assert T.equal(o[k].view(T.int32), v.view(T.int32)), (k, t, g)
                else:
                    assert o[k] == v, (k, t, g)
            outs[g] = o
            if spacings is None and t == 0:
                assert o["best"] is None
                continue
            b = o["best"]
            assert set(b) == {"matches", val, "match_count", "slot"}
            lead = () if spacings is None else (len(spacings),)
            assert tuple(b["matches"].shape) == lead + (best, 2) and tuple(b["match_count"].shape) == lead
            as2d = (lambda x: x[None]) if spacings is None else (lambda x: x)
            want = rc.rank_ref(as2d(o["matches"]).cpu().numpy(), as2d(o[val]).cpu().numpy(), as2d(o["match_count"]).cpu().numpy(), best)
            _check(tuple(as2d(b[k]).cpu().numpy() for k in ("matches", val, "match_count", "slot")), want, (name, spacings, t, g))
            if g:
                total += int(b["match_count"].sum())
                if spacings is not None:
                    for row, s in enumerate(spacings):
                        if t < s:
                            assert int(b["match_count"][row]) == 0 and not b["matches"][row].any() and not b[val][row].view(T.int32).any()
        if outs[False]["best"] is not None:
            for k in outs[False]["best"]:
                assert T.equal(outs[False]["best"][k].view(T.int32), outs[True]["best"][k].view(T.int32)), (k, t, "the two forms agree")
    assert total > 0
