"""sslam_sim_argmax where no similarity, or only some, is positive - and the finalize kernels with a threshold met exactly.

1. Arg-max.  The descriptor sets of tests/sim_sign_cases.py (all negative, mixed signs, the winner in the last stage, rows / columns
   of exact zeros) at widths 128 and 256, at shapes that leave one candidate or a full tile in the last stage and 126 / 127 idle
   query lanes: nn12, s12, nn21, s21 and second12 BIT FOR BIT against oracle/ora.py, in both launch forms (SSLAM_M1_VARIANT 1 and
   2, and the rule of the batch size: 1 and 3 pairs two-pass, 17 single-evaluation with the workspace), through the strided entry,
   the pair-list entry with an absent pair among present ones, and the rows-only entries.  A padding row that is not masked, or an
   idle query lane that is not keyed below every similarity, wins here: it holds a zero and everything else is below it.
2. Thresholds.  match_finalize_kernel keeps a row on >=; the rule kernel's comparisons are strict.  Each threshold is set to the
   very fp32 value the kernel compares, then one ulp below and one above, one condition at a time.

tests/test_sim_sign_inputs.py shows on the CPU that the sets are what they are called and what the oracle decides at each
position.  No tolerances in this file."""
import numpy as np
import pytest

import match_rules_cases as mc
import sim_sign_cases as ss
from oracle import ora

pytestmark = pytest.mark.gpu

NAMES = ("nn12", "s12", "nn21", "s21", "second12")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def hip(T):
    from sslam_amd import lib
    lib.lib()
    return lib


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, names, tag):
    """Device tensors (one pair's rows) against the oracle's arrays, by bits."""
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (name, tag, g[:8], w[:8])


def _once(hip, n2, n_pairs):
    return int(hip.lib().sslam_sim_argmax_workspace_bytes(n2, n_pairs)) > 0


# ------------------------------------------------------------------------------------------------ 1. arg-max
@pytest.mark.parametrize("d", ss.WIDTHS)
@pytest.mark.parametrize("n1,n2", ss.SHAPES)
def test_strided_batches_in_both_forms_and_rows_only(T, hip, knob, n1, n2, d):
    """1 pair (every kind in a launch of its own), 3 and 17 pairs, under the batch-size rule and with either form forced."""
    D1, D2, kinds = ss.batch(n1, n2, d, 17)
    A, B = dev(T, D1), dev(T, D2)
    want = [ss.oracle(k, n1, n2, d, seed=p) for p, k in enumerate(kinds)]
    for variant in (0, 1, 2):
        knob("SSLAM_M1_VARIANT", variant)
        assert _once(hip, n2, 17) == (variant != 1) and _once(hip, n2, 3) == (variant == 2)
        for p in range(len(ss.KINDS)):
            got = hip.sim_argmax(A[p], 0, n1, B[p], 0, n2, 1, want_s21=True, want_second=True)
            _same([t[0] for t in got], want[p], NAMES, (variant, 1, kinds[p]))
        for n_pairs in (3, 17):
            got = hip.sim_argmax(A, n1 * d, n1, B, n2 * d, n2, n_pairs, want_s21=True, want_second=True)
            for p in range(n_pairs):
                _same([t[p] for t in got], want[p], NAMES, (variant, n_pairs, p, kinds[p]))
        lean = hip.sim_argmax(A, n1 * d, n1, B, n2 * d, n2, 17)          # the kernels without the runner-up, s21 NULL
        assert lean[3] is None and lean[4] is None
        for p in range(17):
            _same([t[p] for t in lean[:3]], want[p], NAMES[:3], (variant, "lean", p))
    for n_pairs in (3, 17):
        before = hip.launch_count()
        rows = hip.sim_argmax_rows(A, n1 * d, n1, B, n2 * d, n2, n_pairs, want_second=True)
        assert hip.launch_count() - before == 1
        for p in range(n_pairs):
            _same([t[p] for t in rows], (want[p][0], want[p][1], want[p][4]), ("nn12", "s12", "second12"), ("rows", n_pairs, p))
    if n2 == 1:
        assert all(np.isneginf(w[4]).all() for w in want), "no runner-up among one candidate"


@pytest.mark.parametrize("d", ss.WIDTHS)
@pytest.mark.parametrize("k", [1, 65, 130])
def test_pair_lists_with_an_absent_pair(T, hip, knob, k, d):
    """A bank of ten frames (d1, d2 of every kind); every kind's pair, two of them named the other way round too, one absent."""
    sets = [ss.descriptor_set(kind, k, k, d, seed=p) for p, kind in enumerate(ss.KINDS)]
    bank = dev(T, np.stack([x for s in sets for x in s]))
    pairs = [(0, 1), (2, 3), (-1, 5), (4, 5), (6, 7), (8, 9), (3, 2), (9, 8)]
    first, second = (T.tensor([p[i] for p in pairs], dtype=T.int32, device="cuda") for i in (0, 1))
    for variant in (1, 2):
        knob("SSLAM_M1_VARIANT", variant)
        got = hip.sim_argmax_pairs(bank, first, second, want_s21=True, want_second=True)
        rows = hip.sim_argmax_rows_pairs(bank, first, second, want_second=True)
        for row, (a, b) in enumerate(pairs):
            if a < 0:
                assert not any(t[row].view(T.int32).any() for t in got + rows), "an absent pair's rows are zero"
                continue
            p = min(a, b) // 2
            want = ss.oracle(ss.KINDS[p], k, k, d, seed=p, swap=a > b)
            _same([t[row] for t in got], want, NAMES, (variant, row, a, b))
            _same([t[row] for t in rows], (want[0], want[1], want[4]), ("nn12", "s12", "second12"), (variant, "rows", row))


# ------------------------------------------------------------------------------------------------ 2. thresholds met exactly
@pytest.fixture(scope="module")
def edge(T, hip):
    """The 70 x 70 pair on the device with its arg-max arrays (the oracle's, bit for bit) - strided and as a bank of two frames
    under the list (0, 1), (absent)."""
    e = ss.edge_pair()
    n = ss.N_EDGE
    a, b = dev(T, e["d1"]), dev(T, e["d2"])
    nn12, s12, nn21, _, sec = hip.sim_argmax(a, 0, n, b, 0, n, 1, want_second=True)
    assert np.array_equal(nn12.cpu().numpy()[0], e["nn12"]) and np.array_equal(nn21.cpu().numpy()[0], e["nn21"])
    assert np.array_equal(bits(s12.cpu().numpy()[0]), bits(e["s12"]))
    first, second = T.tensor([0, -1], dtype=T.int32, device="cuda"), T.tensor([1, 0], dtype=T.int32, device="cuda")
    listed = hip.sim_argmax_pairs(dev(T, np.stack([e["d1"], e["d2"]])), first, second)
    assert T.equal(listed[0][0], nn12[0]) and T.equal(listed[2][0], nn21[0]) and T.equal(listed[1][0].view(T.int32), s12[0].view(T.int32))
    return dict(e, dev=dict(nn12=nn12, s12=s12, nn21=nn21, sec=sec, s1=dev(T, e["s1"]), s2=dev(T, e["s2"]), i1=dev(T, e["i1"]),
                            i2=dev(T, e["i2"]), first=first, second=second, listed=listed,
                            scores=dev(T, np.stack([e["s1"], e["s2"]])), intensity=dev(T, np.stack([e["i1"], e["i2"]]))))


def _row_equals(matches, value, count, want, tag):
    """One pair's fixed-capacity arrays against the oracle's (matches, value): count, pairs, value bits, zeroed tail."""
    want_m, want_v = want
    matches, value, c = matches.cpu().numpy(), value.cpu().numpy(), int(count)
    assert c == len(want_m), (tag, c, len(want_m))
    assert np.array_equal(matches[:c], want_m) and np.array_equal(bits(value[:c]), bits(np.ascontiguousarray(want_v, np.float32))), tag
    assert not matches[c:].any() and not bits(value[c:]).any(), tag
    return matches[:c, 0]


def test_m1_thresholds_met_exactly(T, hip, edge):
    """t_sim = s12[i], t_sal = (s1[i] + s2[j]) / 2, t_int likewise: kept at equality and one ulp below, dropped one ulp above -
    through sslam_match_finalize and sslam_match_finalize_pairs, the whole list against ora.match_with_quality."""
    n, dv = ss.N_EDGE, edge["dev"]
    w_sal = 0.3
    for i in ss.edge_rows(edge):
        exact = ss.m1_thresholds(edge, i)
        for cond in ("sim", "sal", "int"):
            for pos, t in zip((-1, 0, 1), ss.three_positions(exact[cond])):
                th = {k: float(v) for k, v in dict(ss.WIDE_OPEN, **{cond: t}).items()}
                want = ora.match_with_quality(edge["d1"], edge["d2"], edge["s1"], edge["s2"], w_sal, th["sal"], th["sim"], edge["i1"],
                                              edge["i2"], th["int"])
                assert (i in want[0][:, 0]) == (pos <= 0)
                mt, q, cnt = hip.match_finalize(dv["nn12"], dv["s12"], dv["nn21"], n, n, 1, dv["s1"], 0, dv["s2"], 0, dv["i1"], dv["i2"],
                                                1.0 - w_sal, w_sal, th["sal"], th["sim"], th["int"])
                kept = _row_equals(mt[0], q[0], cnt[0], want, (i, cond, pos))
                assert (i in kept) == (pos <= 0), (i, cond, pos)
                ls = dv["listed"]
                mt, q, cnt = hip.match_finalize_pairs(ls[0], ls[1], ls[2], dv["first"], dv["second"], dv["scores"], dv["intensity"],
                                                      1.0 - w_sal, w_sal, th["sal"], th["sim"], th["int"])
                kept = _row_equals(mt[0], q[0], cnt[0], want, (i, cond, pos, "pairs"))
                assert (i in kept) == (pos <= 0), (i, cond, pos, "pairs")
                assert int(cnt[1]) == 0 and not mt[1].any() and not q[1].view(T.int32).any(), "the absent pair"


def test_rule_thresholds_met_exactly(T, hip, edge):
    """M5 at param = s12[i] and M4 at param = the rounded quotient are strict: dropped at equality, kept one ulp to the keeping side;
    M2 with the runner-up equal to the best keeps every row just below param = 1.0 and none at or above it."""
    n, dv = ss.N_EDGE, edge["dev"]
    d1, d2 = edge["d1"], edge["d2"]
    rows_only = hip.sim_argmax_rows(dev(T, d1), 0, n, dev(T, d2), 0, n, 1)
    for i in ss.edge_rows(edge):
        for pos, t in zip((-1, 0, 1), ss.three_positions(edge["s12"][i])):
            mt, v, c = hip.match_finalize_rule(rows_only[0], rows_only[1], None, None, n, n, 1, hip.RULE_TRACKED, float(t))
            kept = _row_equals(mt[0], v[0], c[0], mc.oracle_rule(mc.TRACKED, d1, d2, float(t)), ("m5", i, pos))
            assert (i in kept) == (pos < 0), ("m5", i, pos)
        for pos, t in zip((-1, 0, 1), ss.three_positions(ss.m4_quotient(edge, i))):
            mt, v, c = hip.match_finalize_rule(dv["nn12"], dv["s12"], dv["sec"], dv["nn21"], n, n, 1, hip.RULE_RATIO_SECOND, float(t))
            kept = _row_equals(mt[0], v[0], c[0], mc.oracle_rule(mc.MNN_RATIO, d1, d2, float(t)), ("m4", i, pos))
            assert (i in kept) == (pos > 0), ("m4", i, pos)
    twice = np.concatenate([d1, d1])
    nn12, s12, nn21, _, sec = hip.sim_argmax(dev(T, d1), 0, n, dev(T, twice), 0, 2 * n, 1, want_second=True)
    assert T.equal(s12.view(T.int32), sec.view(T.int32)), "the runner-up equals the best"
    for pos, t in zip((-1, 0, 1), ss.three_positions(1.0)):
        mt, v, c = hip.match_finalize_rule(nn12, s12, sec, nn21, n, 2 * n, 1, hip.RULE_RATIO_BEST, float(t))
        kept = _row_equals(mt[0], v[0], c[0], mc.oracle_rule(mc.RATIO, d1, twice, float(t)), ("m2", pos))
        assert len(kept) == (n if pos < 0 else 0), ("m2", pos)
