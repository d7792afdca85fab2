"""GPU tests of the rule matchers: M2 (ratio test against the runner-up), M4 (mutual nearest neighbours + Lowe ratio) and M5 (the
tracking count) as the device-side finalize stage of the matcher, batched, over pair lists, streaming and in the online step.
Everything is BIT FOR BIT - indices, values, counts - against the reference-held goldens, oracle/ora.py and matching.py (which
stays on its own torch-op path and is the independent yardstick here); there are no tolerances in this file.

Inputs: the synthetic 27-frame sequence, tokens in (no ViT), K = 500; its first 6 frames are the frames on which
tests/test_match_rules_api.py asserts, on the oracle alone, that every rule's middle threshold keeps some rows and rejects some.
"""
import numpy as np
import pytest

import match_rules_cases as mc
import synth
from match_rules_cases import MNN_RATIO, RATIO, THRESHOLDS, TRACKED

pytestmark = pytest.mark.gpu

N = 27
RULES = (RATIO, MNN_RATIO, TRACKED)
RULE_KEYS = ("matches", "value", "match_count", "nn12", "sim")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def pipe(T):
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    return SequencePipeline(ExtractorConfig(saliency_weight=0.3, min_saliency=0.5, min_descriptor_sim=0.7, min_intensity=0.15),
                            synth.selector_state(0), synth.refiner_state(0), device="cuda")


@pytest.fixture(scope="module")
def seq(T, pipe):
    """27 extracted frames (device dict) and the host copy of their descriptors for the oracle."""
    toks = T.from_numpy(synth.token_sequence(N, 28)).cuda()
    imgs = T.from_numpy(synth.image_sequence(N)).cuda()
    ex = pipe.extract(toks, imgs)
    return dict(toks=toks, imgs=imgs, ex=ex, desc=ex["descriptors"].cpu().numpy())


def _rule(name, param=None):
    from sslam_amd.pipeline import MatchRule
    return getattr(MatchRule, name)(*(() if param is None else (param,)))


_ORACLE = {}


def _oracle(seq, name, param, i, j):
    key = (name, param, i, j)
    if key not in _ORACLE:
        _ORACLE[key] = mc.oracle_rule(name, seq["desc"][i], seq["desc"][j], param)
    return _ORACLE[key]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_row(matches, value, count, want, where):
    """One pair's fixed-capacity arrays against (matches, value) of the oracle: count, index pairs, value bits, zeroed tail."""
    want_m, want_v = want
    c = int(count)
    assert c == len(want_m), (where, c, len(want_m))
    assert matches.dtype == np.int64 and np.array_equal(matches[:c], want_m), where
    assert _same_bits(value[:c], want_v), where
    assert not matches[c:].any() and not value[c:].view(np.uint32).any(), where
    return c


def _host(res, keys=("matches", "value", "match_count")):
    return {k: res[k].cpu().numpy() for k in keys}


def _lib_rule(T, name, param, d1, d2):
    """One pair through sslam_amd.lib directly: d1 (n1, 128), d2 (n2, 128) numpy -> (matches (n1, 2), value (n1,), count, nn12)."""
    from sslam_amd import lib
    a, b = T.from_numpy(np.ascontiguousarray(d1)).cuda(), T.from_numpy(np.ascontiguousarray(d2)).cuda()
    n1, n2 = a.shape[0], b.shape[0]
    r = _rule(name, param)
    if name == TRACKED:
        nn12, s12, sec = lib.sim_argmax_rows(a, 0, n1, b, 0, n2, 1)
        nn21 = None
    else:
        nn12, s12, nn21, _, sec = lib.sim_argmax(a, 0, n1, b, 0, n2, 1, want_second=True)
    m, v, c = lib.match_finalize_rule(nn12, s12, sec, nn21, n1, n2, 1, r.kind, r.param)
    return m[0].cpu().numpy(), v[0].cpu().numpy(), int(c[0]), nn12[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. reference goldens
@pytest.mark.parametrize("tag", ["p500", "p500x480", "p1024", "p33x70"])
def test_reference_goldens(T, tag):
    from test_oracle_golden import _pair, gold
    g = gold("matchers")
    seed, n, m, dup = (int(v) for v in g[f"{tag}_spec"])
    d1, d2, *_ = _pair(seed, n, m, dup)
    mt, v, c, _ = _lib_rule(T, RATIO, 0.8, d1, d2)                                      # M2
    assert np.array_equal(mt[:c], g[f"{tag}_m2_ij"])
    _check_row(mt, v, c, mc.oracle_rule(RATIO, d1, d2, 0.8), (tag, "m2"))
    mt, v, c, _ = _lib_rule(T, MNN_RATIO, 0.9, d1, d2)                                  # M4
    assert np.array_equal(mt[:c], g[f"{tag}_m4_matches"])
    _check_row(mt, v, c, mc.oracle_rule(MNN_RATIO, d1, d2, 0.9), (tag, "m4"))
    mt, v, c, _ = _lib_rule(T, TRACKED, 0.8, d1, d2)                                    # M5
    assert c == int(g[f"{tag}_m5_count"])
    _check_row(mt, v, c, mc.oracle_rule(TRACKED, d1, d2, 0.8), (tag, "m5"))


# -------------------------------------------------------------------------------------------- 2. selective thresholds
SIX_PAIRS = [(i, j) for i in range(mc.N_COND) for j in range(i + 1, mc.N_COND)]


@pytest.mark.parametrize("name", RULES)
def test_selective_thresholds_on_every_pair_of_six_frames(T, pipe, seq, name):
    import matching
    ex = seq["ex"]
    kept = {}
    for param in THRESHOLDS[name]:
        res = pipe.match_pairs(ex["descriptors"], ex["scores"], first=[p[0] for p in SIX_PAIRS], second=[p[1] for p in SIX_PAIRS],
                               rule=_rule(name, param))
        assert "quality" not in res and set(RULE_KEYS) <= set(res)
        assert ("second" in res and "nn21" in res) == (name != TRACKED)
        h = _host(res)
        for row, (i, j) in enumerate(SIX_PAIRS):
            want = _oracle(seq, name, param, i, j)
            c = _check_row(h["matches"][row], h["value"][row], h["match_count"][row], want, (name, param, i, j))
            kept[(param, i, j)] = c
            d1, d2 = ex["descriptors"][i], ex["descriptors"][j]
            if name == RATIO:                                  # the torch-op matchers of matching.py, pair by pair
                got = matching.find_matches(d1, d2, param)
                assert [(a, b) for a, b, _ in got] == [tuple(r) for r in want[0].tolist()]
                assert _same_bits(np.array([s for *_, s in got], np.float32), want[1])
            elif name == MNN_RATIO:
                gm, gd = matching.find_mutual_nearest_neighbors(d1, d2, param)
                assert np.array_equal(gm.reshape(-1, 2), want[0]) and _same_bits(gd, want[1])
            else:
                assert matching.count_tracked(d1, d2, param) == c
    for i, j in mc.CONDITION_PAIRS:                            # the rules select here (asserted on the oracle in the CPU test)
        assert 0 < kept[(mc.MIDDLE[name], i, j)] < kept[(mc.LOOSEST[name], i, j)]


# ------------------------------------------------------------------------------ 3. batching and both similarity forms
def _single_pair(T, pipe, seq, cache, name, i, j):
    """match() on the two frames alone (one pair: the two-pass form, no knob)."""
    if (name, i, j) not in cache:
        ex = seq["ex"]
        d = T.stack([ex["descriptors"][i], ex["descriptors"][j]])
        s = T.stack([ex["scores"][i], ex["scores"][j]])
        r = pipe.match(d, s, spacing=1, rule=_rule(name, mc.MIDDLE[name]))
        cache[(name, i, j)] = {k: v[0].clone() for k, v in r.items()}
    return cache[(name, i, j)]


@pytest.fixture(scope="module")
def single(T):
    return {}


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", RULES)
def test_batches_in_both_similarity_forms_equal_single_pairs(T, pipe, seq, single, name, variant):
    """20 frames: spacing 1 gives 19 pairs (S evaluated once, 64-bit key reduction), spacing 15 gives 5 (S once per direction);
    variant 1 / 2 force either form on either batch (SSLAM_M1_VARIANT).  tracked takes the rows-only launch whatever the knob."""
    from sslam_amd import lib
    ex = seq["ex"]
    d, s = ex["descriptors"][:20], ex["scores"][:20]
    for sp, n_pairs in ((1, 19), (15, 5)):
        n0 = lib.launch_count()
        if variant:
            with lib.knobs(SSLAM_M1_VARIANT=variant):          # restored on the way out, also when the call raises
                res = pipe.match(d, s, spacing=sp, rule=_rule(name, mc.MIDDLE[name]))
        else:
            res = pipe.match(d, s, spacing=sp, rule=_rule(name, mc.MIDDLE[name]))
        once = name != TRACKED and (variant == 2 or (variant == 0 and n_pairs >= 16))
        assert lib.launch_count() - n0 == (3 if once else 2), "similarity (+ key decode) + the rule's finalize"
        assert res["match_count"].shape == (n_pairs,)
        for row in range(n_pairs):
            want = _single_pair(T, pipe, seq, single, name, row, row + sp)
            assert set(want) == set(res)
            for k in res:
                assert T.equal(res[k][row].view(T.int32), want[k].view(T.int32)), (k, sp, row)
        assert int(res["match_count"].sum()) > 0
    assert lib.lib().sslam_sim_argmax_workspace_bytes(500, 19) > 0 == lib.lib().sslam_sim_argmax_workspace_bytes(500, 5), "knob restored"


# ------------------------------------------------------------------------------------------------------ 4. pair lists
LISTS = {
    "reversed": [(9, 4), (26, 6), (1, 0)],
    "self": [(4, 4), (0, 1), (11, 11)],
    "listed_twice": [(2, 9), (5, 6), (2, 9)],
    "one_against_ten": [(13, j) for j in (0, 2, 5, 7, 11, 14, 17, 20, 23, 26)],
    "absent_few": [(-1, 3), (0, 1), (2, 7), (4, -1), (-1, -1), (5, 6), (12, -1)],
    "absent_many": [(-1, -1)] + [(i, i + 1) for i in range(8)] + [(-1, 4), (9, -1)] + [(i, i + 5) for i in range(10)] + [(3, -1), (-1, 0)],
}


@pytest.mark.parametrize("host_lists", [False, True], ids=["device_lists", "host_lists"])
@pytest.mark.parametrize("name", RULES)
def test_pair_lists(T, pipe, seq, single, name, host_lists):
    ex = seq["ex"]
    for tag, pairs in LISTS.items():
        first, second = [p[0] for p in pairs], [p[1] for p in pairs]
        if not host_lists:
            first, second = (T.tensor(x, dtype=T.int32, device="cuda") for x in (first, second))
        res = pipe.match_pairs(ex["descriptors"], ex["scores"], first=first, second=second, rule=_rule(name, mc.MIDDLE[name]))
        assert (len(pairs) >= 16) == (tag == "absent_many")    # both similarity forms meet absent pairs
        for row, (i, j) in enumerate(pairs):
            if -1 in (i, j):                                   # absent: count 0, zero rows, zeroed value (and arg-max arrays)
                assert int(res["match_count"][row]) == 0, (tag, row)
                for k in res:
                    assert not res[k][row].view(T.int32).any(), (tag, k, row)
                continue
            want = _single_pair(T, pipe, seq, single, name, i, j)
            for k in res:
                assert T.equal(res[k][row].view(T.int32), want[k].view(T.int32)), (tag, k, row, i, j)
            h = {k: res[k][row].cpu().numpy() for k in ("matches", "value", "match_count")}
            _check_row(h["matches"], h["value"], h["match_count"], _oracle(seq, name, mc.MIDDLE[name], i, j), (tag, i, j))


# ------------------------------------------------------------------------------------------------- 5. smallest shapes
def _small(seed, n1, n2):
    return synth.unit_descriptors(seed, n1), synth.unit_descriptors(seed + 1, n2)


@pytest.mark.parametrize("n1,n2", [(1, 70), (33, 1), (257, 64), (33, 70), (1, 1)])
def test_smallest_shapes(T, n1, n2):
    """n1 = 1; n2 = 1 (M2's runner-up is the reference's -1, M4 is refused, M5 is fine); n1 = 257: one lane into the second
    256-row pass of the compaction; 33 x 70: neither a multiple of any tile.  Random unit rows: similarities around 0, so the
    thresholds sit there."""
    from sslam_amd import lib
    d1, d2 = _small(300 + n1 + n2, n1, n2)
    d2[0] = d1[n1 - 1]                                         # one sure mutual pair with similarity 1: the last row, slot 256
    for name, params in ((RATIO, (0.8, 1.6, -2.0)), (MNN_RATIO, (0.9, 0.3, -0.5)), (TRACKED, (0.8, 0.1, -0.2))):
        for param in params:
            if name == MNN_RATIO and n2 < 2:
                with pytest.raises(ValueError):               # SSLAM_E_INVALID before any launch: the reference raises there
                    _lib_rule(T, name, param, d1, d2)
                continue
            n0 = lib.launch_count()
            mt, v, c, nn12 = _lib_rule(T, name, param, d1, d2)
            assert lib.launch_count() - n0 == 2
            assert mt.shape == (n1, 2) and 0 <= nn12.min() and nn12.max() < n2
            _check_row(mt, v, c, mc.oracle_rule(name, d1, d2, param), (name, param, n1, n2))
    if n2 == 1:                                                # the runner-up is the reference's -1: every row is mutual with
        mt, v, c, _ = _lib_rule(T, RATIO, 0.8, d1, d2)        # its only candidate's best row alone, and that row has sim 1 > -0.8
        assert c == 1 and tuple(mt[0]) == (n1 - 1, 0) and v[0] > np.float32(0.999)


def test_duplicated_descriptors_make_the_runner_up_the_best(T):
    """d2 holds every row of d1 twice: the runner-up of each row EQUALS its best (1 up to rounding), so M4's ratio is
    best / (best + 1e-8) = 1 in fp32 - rejected at 0.9, kept at 1.5 - and M2 at 1.0 rejects (best > best is false), at 0.8 keeps."""
    d1 = synth.unit_descriptors(77, 40)
    d2 = np.concatenate([d1, d1])
    for name, param, keeps in ((MNN_RATIO, 0.9, False), (MNN_RATIO, 1.5, True), (RATIO, 1.0, False), (RATIO, 0.8, True),
                               (TRACKED, 0.99, True)):
        mt, v, c, nn12 = _lib_rule(T, name, param, d1, d2)
        assert np.array_equal(nn12, np.arange(40)), "the first of two equal candidates wins"
        assert c == (40 if keeps else 0), (name, param, c)
        _check_row(mt, v, c, mc.oracle_rule(name, d1, d2, param), (name, param))


@pytest.mark.parametrize("where", ["d1", "d2"])
def test_a_nan_row_is_never_kept_and_every_index_stays_in_range(T, where):
    n1, n2, bad = 70, 33, 5
    d1, d2 = _small(500, n1, n2)
    (d1 if where == "d1" else d2)[bad] = np.nan
    for name, params in ((RATIO, (0.8, -2.0)), (MNN_RATIO, (0.9, 1e30)), (TRACKED, (0.8, -1e30))):
        for param in params:
            mt, v, c, nn12 = _lib_rule(T, name, param, d1, d2)
            assert 0 <= c <= n1 and 0 <= nn12.min() and nn12.max() < n2
            assert 0 <= mt[:c, 0].min(initial=0) and mt[:c, 0].max(initial=0) < n1 and mt[:c, 1].max(initial=0) < n2
            assert np.all(np.diff(mt[:c, 0]) > 0) and not mt[c:].any()
            assert not np.isnan(v[:c]).any()
            if where == "d1":
                assert bad not in mt[:c, 0], (name, param)     # every similarity of that row is NaN
            else:
                assert bad not in mt[:c, 1], (name, param)     # a NaN similarity never wins a row


# ---------------------------------------------------------------------------------------------------- 6. rows-only
@pytest.mark.parametrize("m", [3, 17])
def test_rows_only_similarity_equals_the_full_entries(T, pipe, seq, m):
    """3 pairs: the full entry runs its two-pass form; 17: S once + key reduction.  The rows-only launch gives the same nn12 / s12 /
    second12 either way, at 500 x 500 and at 33 x 70, strided and over pair lists (with an absent pair), in one launch."""
    from sslam_amd import lib
    d = seq["ex"]["descriptors"]
    k = d.shape[1]
    a = T.from_numpy(np.stack([synth.unit_descriptors(600 + p, 33) for p in range(m)])).cuda()
    b = T.from_numpy(np.stack([synth.unit_descriptors(700 + p, 70) for p in range(m)])).cuda()
    for d1, s1, n1, d2, s2, n2 in ((d, k * 128, k, d[2:], k * 128, k), (a, 33 * 128, 33, b, 70 * 128, 70), (a, 0, 33, b, 70 * 128, 70)):
        full = lib.sim_argmax(d1, s1, n1, d2, s2, n2, m, want_second=True, workspace=pipe.workspace(0, m))
        n0 = lib.launch_count()
        rows = lib.sim_argmax_rows(d1, s1, n1, d2, s2, n2, m, want_second=True)
        assert lib.launch_count() - n0 == 1
        for name, x, y in zip(("nn12", "s12", "second12"), rows, (full[0], full[1], full[4])):
            assert T.equal(x.view(T.int32), y.view(T.int32)), (name, n1, n2)
        lean = lib.sim_argmax_rows(d1, s1, n1, d2, s2, n2, m)
        assert lean[2] is None and T.equal(lean[0], full[0]) and T.equal(lean[1].view(T.int32), full[1].view(T.int32))
    for bank in (d, a):
        nb = bank.shape[0]
        first = T.arange(0, m, dtype=T.int32, device="cuda") % nb
        second = (first * 7 + 3) % nb
        first[1] = -1
        full = lib.sim_argmax_pairs(bank, first, second, want_second=True, workspace=pipe.workspace(0, m))
        n0 = lib.launch_count()
        rows = lib.sim_argmax_rows_pairs(bank, first, second, want_second=True)
        assert lib.launch_count() - n0 == 1
        for name, x, y in zip(("nn12", "s12", "second12"), rows, (full[0], full[1], full[4])):
            assert T.equal(x.view(T.int32), y.view(T.int32)), (name, tuple(bank.shape))
        assert not any(t[1].view(T.int32).any() for t in rows), "the absent pair's rows are zero"


# ---------------------------------------------------------------------------------------------------- 7. streaming
@pytest.mark.parametrize("name", RULES)
def test_streaming_sequence_under_a_rule(T, pipe, seq, name):
    from sslam_amd.harness import StreamingSequence
    sp, rule = (1, 5, 10), _rule(name, mc.MIDDLE[name])
    keys = ("matches", "value", "match_count")
    ref = None
    for chunk in (None, 4, 7):
        res = StreamingSequence(pipe, sp, rule=rule).run(seq["toks"], seq["imgs"], chunk=chunk)
        got = {s: {k: res[s][k].clone() for k in keys} for s in sp}
        assert all("quality" not in res[s] for s in sp)
        if ref is None:
            ref = got
        for s in sp:
            assert got[s]["match_count"].shape == (N - s,)
            for k in keys:
                assert T.equal(got[s][k].view(T.int32), ref[s][k].view(T.int32)), (chunk, s, k)
    ring = StreamingSequence(pipe, sp, rule=rule)
    ring.reset()
    outs = [ring.push(seq["toks"][a:a + 7], seq["imgs"][a:a + 7]) for a in range(0, N, 7)]
    for s in sp:
        for k in keys:
            cat = T.cat([o[s][k] for o in outs if s in o])
            assert T.equal(cat.view(T.int32), ref[s][k].view(T.int32)), ("ring", s, k)
        h = {k: ref[s][k].cpu().numpy() for k in keys}
        total = sum(_check_row(h["matches"][i], h["value"][i], h["match_count"][i], _oracle(seq, name, mc.MIDDLE[name], i, i + s),
                               (name, s, i)) for i in range(N - s))
        assert 0 < total < (N - s) * 500


# ------------------------------------------------------------------------------------------------------ 8. stepper
N_STEP = 12


@pytest.mark.parametrize("use_graph", [False, True], ids=["launches", "graph"])
@pytest.mark.parametrize("spacings", [None, (1, 3, 5)], ids=["one_spacing", "three_spacings"])
@pytest.mark.parametrize("name", RULES + (None,))
def test_rule_stepper_equals_the_streaming_harness(T, pipe, seq, name, spacings, use_graph):
    """12 frames, tokens in; with spacings (1, 3, 5) the ring of 5 slots wraps twice.  name None: RuleFrameStepper(rule=None) is the
    stepper of today - its matches / quality are those of the M1 harness."""
    from sslam_amd import lib
    from sslam_amd.harness import StreamingSequence
    from sslam_amd.online import RuleFrameStepper
    rule = None if name is None else _rule(name, mc.MIDDLE[name])
    val = "quality" if rule is None else "value"
    keys = ("matches", val, "match_count")
    toks, imgs = seq["toks"][:N_STEP], seq["imgs"][:N_STEP]
    sp = (1,) if spacings is None else spacings
    want = StreamingSequence(pipe, sp, rule=rule).run(toks, imgs)
    st = RuleFrameStepper(pipe, 480, 640, use_graph=use_graph, tokens_in=True, spacings=spacings, rule=rule)
    total = 0
    for t in range(N_STEP):
        n0 = lib.launch_count()
        o = st.step(imgs[t], toks[t])
        assert (lib.launch_count() - n0 == 0) == (use_graph and t > 0), "a replayed step issues no library call"
        assert ("value" in o) == (rule is not None) and ("quality" in o) == (rule is None)
        assert T.equal(o["descriptors"], want["frames"]["descriptors"][t]), t
        if spacings is None:
            if t == 0:
                assert o["matches"] is None and o[val] is None and o["match_count"] is None
                continue
            for k in keys:
                assert T.equal(o[k].view(T.int32), want[1][k][t - 1].view(T.int32)), (k, t)
            total += int(o["match_count"])
            continue
        assert o["pair_first"] == [t - s if t >= s else -1 for s in sp]
        for row, s in enumerate(sp):
            if t < s:
                assert int(o["match_count"][row]) == 0 and not o["matches"][row].any() and not o[val][row].view(T.int32).any(), (t, s)
            else:
                for k in keys:
                    assert T.equal(o[k][row].view(T.int32), want[s][k][t - s].view(T.int32)), (k, t, s)
                total += int(o["match_count"][row])
    assert total > 0
