"""CPU side of tests/test_gpu_sim_signs.py: every descriptor set of tests/sim_sign_cases.py is what its name says - judged from a
float64 product, not from the oracle - and the oracle's arg-max is the float64 arg-max wherever that one is decided by more than
1e-5.  The threshold cases keep a row at equality and one ulp to the keeping side in the ORACLE, so the GPU test compares decisions
that differ from one position to the next."""
import numpy as np
import pytest

import match_rules_cases as mc
import sim_sign_cases as ss
from oracle import ora

CASES = [(k, n1, n2, d) for k in ss.KINDS for (n1, n2) in ss.SHAPES for d in ss.WIDTHS]


def _s64(kind, n1, n2, d, seed=0):
    d1, d2 = ss.descriptor_set(kind, n1, n2, d, seed)
    assert d1.shape == (n1, d) and d2.shape == (n2, d) and d1.dtype == d2.dtype == np.float32
    for x in (d1, d2):
        assert np.abs(np.linalg.norm(x.astype(np.float64), axis=1) - 1).max() < 1e-6
    return d1.astype(np.float64) @ d2.astype(np.float64).T


def test_the_shapes_put_one_candidate_and_a_full_tile_in_the_last_stage():
    tails = {n2 - ss.last_stage_start(n2) for _, n2 in ss.SHAPES}
    assert {1, 6, 64} <= tails
    idle = {-n1 % 128 for n1, _ in ss.SHAPES}           # query lanes of the last block of 128 that hold no query
    assert {127, 126} <= idle
    assert (1, 1) in ss.SHAPES and any(n2 == 1 < n1 for n1, n2 in ss.SHAPES)


@pytest.mark.parametrize("kind,n1,n2,d", CASES)
def test_sets_are_what_their_names_say(kind, n1, n2, d):
    S = _s64(kind, n1, n2, d)
    L1, L2 = ss.last_stage_start(n1), ss.last_stage_start(n2)
    if kind == "all_negative":
        assert S.max() < -0.5
    elif kind == "mixed":
        rows_neg, cols_neg = S.max(axis=1) < -0.2, S.max(axis=0) < -0.2
        assert np.array_equal(rows_neg, (np.arange(n1) % 3 == 2) | (n2 < 2))
        assert cols_neg.any() and (n1 < 3 or rows_neg.any())
        if n2 >= 2:
            win = ~rows_neg
            assert win.any() and (S.max(axis=1)[win] > 0.2).all() and (~cols_neg).any()
            if n2 > ss.STAGE:
                assert (S.argmax(axis=1)[win] < L2).all(), "the positive winners lie in a stage before the last"
    elif kind == "last_stage":
        assert S.max() < -0.1
        assert (S.argmax(axis=1) >= L2).all() and (S.argmax(axis=0) >= L1).all()
    else:
        zero_rows, zero_cols = (S == 0).all(axis=1), (S == 0).all(axis=0)
        assert ((S == 0) | (S < -0.2)).all()
        if kind == "zero_rows":
            assert int(zero_rows.sum()) == n1 // 2 and np.array_equal(zero_rows, np.arange(n1) % 2 == 1) and not zero_cols.any()
            assert (S[~zero_rows] < -0.2).all()
        else:
            assert int(zero_cols.sum()) == n2 // 2 and np.array_equal(zero_cols, np.arange(n2) % 2 == 1)
            assert (S[:, ~zero_cols] < -0.2).all()


@pytest.mark.parametrize("kind,n1,n2,d", CASES)
def test_oracle_is_the_float64_argmax_where_that_is_decided(kind, n1, n2, d):
    S = _s64(kind, n1, n2, d)
    nn12, s12, nn21, s21, sec = ss.oracle(kind, n1, n2, d)
    decided = 0
    for M, nn, best in ((S, nn12, s12), (S.T, nn21, s21)):
        srt = np.sort(M, axis=1)
        gap = srt[:, -1] - srt[:, -2] if M.shape[1] > 1 else np.full(M.shape[0], np.inf)
        clear = gap > 1e-5
        assert np.array_equal(nn[clear], M.argmax(axis=1)[clear])
        assert np.abs(best - M.max(axis=1)).max() < 1e-6
        decided += int(clear.sum())
    assert decided > 0 or kind.startswith("zero")
    if n2 == 1:
        assert np.isneginf(sec).all()
    else:
        assert np.abs(sec - np.sort(S, axis=1)[:, -2]).max() < 1e-6
    if kind == "zero_rows":                       # exact zeros come out as +0.0f, and the first of the tied candidates wins
        z = np.arange(n1) % 2 == 1
        assert not s12[z].view(np.uint32).any() and not nn12[z].any()
        assert n2 == 1 or not sec[z].view(np.uint32).any()


def test_batches_hold_every_kind():
    for n_pairs in (3, 17):
        D1, D2, kinds = ss.batch(33, 70, 128, n_pairs)
        assert D1.shape == (n_pairs, 33, 128) and D2.shape == (n_pairs, 70, 128)
        assert set(kinds) == set(ss.KINDS[:n_pairs])
        assert np.array_equal(D1[1], ss.descriptor_set(kinds[1], 33, 70, 128, seed=1)[0])


# ------------------------------------------------------------------------------------------------ thresholds met exactly
def _m1(e, t, with_intensity=True):
    kw = dict(saliency_weight=0.3, min_saliency=float(t["sal"]), min_descriptor_sim=float(t["sim"]), min_intensity=float(t["int"]))
    if with_intensity:
        kw.update(intensity1=e["i1"], intensity2=e["i2"])
    return ora.match_with_quality(e["d1"], e["d2"], e["s1"], e["s2"], **kw)


def test_m1_thresholds_keep_at_equality_in_the_oracle():
    e = ss.edge_pair()
    assert len(e["mutual"]) >= 20
    everything, _ = _m1(e, ss.WIDE_OPEN)
    assert np.array_equal(everything[:, 0], e["mutual"]), "wide open thresholds keep every mutual row"
    for i in ss.edge_rows(e):
        exact = ss.m1_thresholds(e, i)
        for cond in ("sim", "sal", "int"):
            for pos, t in zip((-1, 0, 1), ss.three_positions(exact[cond])):
                mt, _ = _m1(e, dict(ss.WIDE_OPEN, **{cond: t}))
                assert (i in mt[:, 0]) == (pos <= 0), (i, cond, pos)


def test_rule_thresholds_are_strict_in_the_oracle():
    e = ss.edge_pair()
    for i in ss.edge_rows(e):
        for pos, t in zip((-1, 0, 1), ss.three_positions(e["s12"][i])):                    # M5: best > param
            mt, _ = mc.oracle_rule(mc.TRACKED, e["d1"], e["d2"], float(t))
            assert (i in mt[:, 0]) == (pos < 0), (i, pos)
        for pos, t in zip((-1, 0, 1), ss.three_positions(ss.m4_quotient(e, i))):               # M4: second / (best + 1e-8) < param
            mt, _ = mc.oracle_rule(mc.MNN_RATIO, e["d1"], e["d2"], float(t))
            assert (i in mt[:, 0]) == (pos > 0), (i, pos)
    d2 = np.concatenate([e["d1"], e["d1"]])                                         # M2: the runner-up equals the best
    for pos, t in zip((-1, 0, 1), ss.three_positions(1.0)):
        mt, _ = mc.oracle_rule(mc.RATIO, e["d1"], d2, float(t))
        assert len(mt) == (ss.N_EDGE if pos < 0 else 0), pos
