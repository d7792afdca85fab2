"""The ranking stage (sslam_match_rank: the best N matches of every pair, on the device) as far as a machine without a GPU can see
it: the entry against the header, the built library and sslam_amd.lib; the refusals of the C entry, of the binding, of
SequencePipeline.rank_matches and of RankedFrameStepper, all of which come before any device work; the signatures the stage leaves
alone; and the numpy reference of tests/match_rank_cases.py against the reference-held match lists of tests/golden/, on which the
GPU tests stand."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import match_rank_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sslam_match_rank"
E_INVALID, E_UNSUPPORTED = -1, -2
# never dereferenced: every call below is refused by the entry's own checks, which come before the launch
IN_M, IN_V, IN_C, OUT_M, OUT_V, OUT_C, OUT_S = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


def test_entry_is_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sslam_hip.h")).read()
    assert re.search(r"^int\s+" + ENTRY + r"\s*\(", hdr, flags=re.M), "not declared in include/sslam_hip.h"
    assert ENTRY in lib.EXPORTS
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT\s+" + ENTRY + r"$", dyn, flags=re.M), "not exported by the library"
    declared = set(re.findall(r"^(?:int|long long|const char \*)\s*(sslam_\w+)\s*\(", hdr, flags=re.M))
    exported = set(re.findall(r"\bT\s+(sslam_\w+)$", dyn, flags=re.M))
    assert ENTRY in declared & exported and declared <= exported, sorted(declared - exported)
    L = lib.lib()
    assert L.sslam_version() > 600, "a new entry raises the version"
    # three inputs, n1 / n_pairs / best / ascending, four outputs, stream
    assert len(L.sslam_match_rank.argtypes) == 12
    m = re.search(r"#define\s+SSLAM_RANK_MAX_N1\s+(\d+)", hdr)
    assert m and int(m.group(1)) == lib.RANK_MAX_N1 == rc.MAX_N1 == 4096
    # the header states the order and cites the reference lines the stage restates
    for text in ("visualize_matches_sequence.py:224-225", "visualize_matches.py:150-151", "ascending input slot", "NaN rows come last"):
        assert text in hdr, text


def _rank(L, matches=IN_M, value=IN_V, count=IN_C, n1=8, n_pairs=2, best=4, ascending=0, out_matches=OUT_M, out_value=OUT_V,
          out_count=OUT_C, out_slot=OUT_S):
    return L.sslam_match_rank(matches, value, count, n1, n_pairs, best, ascending, out_matches, out_value, out_count, out_slot, None)


def test_c_entry_refuses_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    before = lib.launch_count()
    bad = [dict(matches=None), dict(value=None), dict(count=None), dict(out_matches=None), dict(out_value=None), dict(out_count=None),
           dict(n1=0), dict(n1=-3), dict(n_pairs=0), dict(n_pairs=-1), dict(best=0), dict(best=-2), dict(best=9), dict(n1=4096, best=4097),
           dict(ascending=2), dict(ascending=-1),
           # an output base equal to an input base
           dict(out_matches=IN_M), dict(out_value=IN_V), dict(out_count=IN_C), dict(out_slot=IN_C), dict(out_slot=IN_V),
           dict(out_value=IN_M), dict(out_count=IN_V)]
    for kw in bad:
        assert _rank(L, **kw) == E_INVALID, kw
    for kw in (dict(n1=4097), dict(n1=4097, best=4097), dict(n1=1 << 20, best=50)):
        assert _rank(L, **kw) == E_UNSUPPORTED, kw
    assert _rank(L, n1=5000, best=5001) == E_INVALID, "best > n1 is an invalid argument at any n1"
    assert lib.launch_count() == before, "a refused call launches nothing"


def test_binding_refuses_malformed_arrays_before_any_device_work():
    from sslam_amd import lib
    m, v, c = torch.zeros((2, 8, 2), dtype=torch.int64), torch.zeros((2, 8)), torch.zeros((2,), dtype=torch.int32)   # host tensors
    before = lib.launch_count()
    for bad in (0, -1, 9, 2.0, "4", True):
        with pytest.raises(ValueError, match="best"):
            lib.match_rank(m, v, c, bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="ascending"):
            lib.match_rank(m, v, c, 4, ascending=bad)
    with pytest.raises(ValueError, match="matches"):
        lib.match_rank(m.int(), v, c, 4)
    with pytest.raises(ValueError, match="matches"):
        lib.match_rank(m[:, :, 0], v, c, 4)
    with pytest.raises(ValueError, match="value"):
        lib.match_rank(m, v[:, :7], c, 4)
    with pytest.raises(ValueError, match="value"):
        lib.match_rank(m, None, c, 4)
    with pytest.raises(ValueError, match="count"):
        lib.match_rank(m, v, c.long(), 4)
    with pytest.raises(ValueError, match="out `value`"):
        lib.match_rank(m, v, c, 4, out=(torch.zeros((2, 4, 2), dtype=torch.int64), torch.zeros((2, 5)), c.clone(), None))
    with pytest.raises(ValueError, match="out `slot`"):
        lib.match_rank(m, v, c, 4, out=(torch.zeros((2, 4, 2), dtype=torch.int64), torch.zeros((2, 4)), c.clone(),
                                        torch.zeros((2, 4), dtype=torch.int64)))
    with pytest.raises(ValueError, match="out `count`"):
        lib.match_rank(m, v, c, 4, out=(torch.zeros((2, 4, 2), dtype=torch.int64), torch.zeros((2, 4)), None, None))
    big = torch.zeros((1, 4097, 2), dtype=torch.int64)
    with pytest.raises(lib.SslamHipError, match="4096"):
        lib.match_rank(big, torch.zeros((1, 4097)), torch.zeros((1,), dtype=torch.int32), 50)
    with pytest.raises(ValueError):                             # well-formed host tensors: refused for where they live
        lib.match_rank(m, v, c, 4)
    assert lib.launch_count() == before


def test_pipeline_and_stepper_refuse_before_touching_a_pipeline():
    from sslam_amd import lib
    from sslam_amd.online import RankedFrameStepper
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    pipe = SequencePipeline.__new__(SequencePipeline)          # no packing, no device: the checks come first
    pipe.cfg = ExtractorConfig()
    k = pipe.cfg.num_keypoints
    m = {"matches": torch.zeros((3, k, 2), dtype=torch.int64), "quality": torch.zeros((3, k)), "match_count": torch.zeros((3,), dtype=torch.int32)}
    mv = {("value" if key == "quality" else key): t for key, t in m.items()}
    before = lib.launch_count()
    for bad in (0, -5, k + 1, 50.0, "50", True):
        with pytest.raises(ValueError, match="best"):
            pipe.rank_matches(m, bad)
        with pytest.raises(ValueError, match="best"):
            pipe.alloc_ranked(3, bad)
        with pytest.raises(ValueError, match="best"):
            RankedFrameStepper(pipe, 480, 640, tokens_in=True, best=bad)
    for bad in (0.8, "mnn_ratio", lib.RULE_RATIO_SECOND):
        with pytest.raises(ValueError, match="MatchRule"):
            pipe.rank_matches(mv, 50, rule=bad)
        with pytest.raises(ValueError, match="MatchRule"):
            RankedFrameStepper(pipe, 480, 640, tokens_in=True, rule=bad, best=50)
    with pytest.raises(ValueError, match="value"):              # an M1 dictionary ranked as a rule's, and the other way round
        pipe.rank_matches(m, 50, rule=MatchRule.ratio())
    with pytest.raises(ValueError, match="quality"):
        pipe.rank_matches(mv, 50)
    with pytest.raises(ValueError):
        pipe.rank_matches({"quality": m["quality"]}, 50)
    assert lib.launch_count() == before


def test_the_stage_leaves_the_pinned_signatures_alone():
    import matching
    from sslam_amd import harness, lib
    from sslam_amd.online import FrameStepper, RankedFrameStepper, RuleFrameStepper
    from sslam_amd.pipeline import SequencePipeline
    sig = lambda f: list(inspect.signature(f).parameters.values())       # noqa: E731
    assert [p.name for p in sig(SequencePipeline.match)] == ["self", "desc", "scores", "intensity", "spacing", "out", "rule"]
    assert [p.name for p in sig(SequencePipeline.match_pairs)] == ["self", "desc", "scores", "intensity", "first", "second", "out", "rule"]
    assert [(p.name, p.default) for p in sig(SequencePipeline.rank_matches)[1:]] == [("m", inspect.Parameter.empty), ("best", None),
                                                                                      ("rule", None), ("out", None)]
    assert [(p.name, p.default) for p in sig(SequencePipeline.alloc_ranked)[3:]] == [("k", None), ("rule", None)]
    assert [(p.name, p.default) for p in sig(lib.match_rank)[3:]] == [("best", None), ("ascending", False), ("out", None), ("want_slot", True)]
    # the same arguments as the parent, in the same order, plus a trailing best = the script's --max_matches default
    r, parent = sig(RankedFrameStepper.__init__), sig(RuleFrameStepper.__init__)
    assert [(p.name, p.default) for p in r[:-1]] == [(p.name, p.default) for p in parent]
    assert (r[-1].name, r[-1].default) == ("best", 50)
    assert issubclass(RankedFrameStepper, RuleFrameStepper) and sig(FrameStepper.__init__)[-1].name == "spacings"
    # visualize_matches.py:131
    assert [(p.name, p.default) for p in sig(matching.best_matches)] == [("matches", inspect.Parameter.empty), ("values", inspect.Parameter.empty),
                                                                         ("max_matches", 100), ("ascending", False)]
    assert [(p.name, p.default) for p in sig(harness.rank_result)] == [("pipe", inspect.Parameter.empty), ("result", inspect.Parameter.empty),
                                                                       ("best", inspect.Parameter.empty), ("rule", None)]


# ---------------------------------------------------------------------------- the numpy reference on the reference-held lists
def test_reference_m1_lists_rank_as_the_reference_ranks_them():
    """All 60 M1 lists at best 50, 100 and count: the kept values are the largest, bit for bit; where the qualities are pairwise
    distinct - where the reference's np.argsort(-q) has one answer - the kept rows are its rows.  That there are at least 51 such
    lists and that no list ties across the cut at 50 or 100 is asserted, so neither comparison can go vacuous."""
    pairs = rc.m1_pairs()
    assert len(pairs) == 60
    distinct = 0
    for tag, mt, q in pairs:
        c = len(q)
        m, v, cnt = rc.padded(mt, q)
        ranked = np.sort(q)[::-1]
        is_distinct = len(np.unique(q)) == c
        distinct += is_distinct
        for best in sorted({min(50, c), min(100, c), c}):
            om, ov, oc, osl = rc.rank_ref(m, v, cnt, best)
            kept = min(c, best)
            assert oc[0] == kept and rc.same_bits(ov[0, :kept], ranked[:kept]), (tag, best)
            assert np.array_equal(om[0, :kept], mt[osl[0, :kept]]) and not om[0, kept:].any() and not ov[0, kept:].any(), (tag, best)
            if best < c:
                assert ranked[best - 1] > ranked[best], (tag, best, "a tie across the cut")
            if is_distinct:
                order = np.argsort(-q)[:best]                 # the reference's expression: ties impossible here
                assert np.array_equal(osl[0, :kept], order) and np.array_equal(om[0, :kept], mt[order]), (tag, best)
    assert distinct >= 51, distinct


def test_reference_m2_and_m4_lists_rank_as_python_sorts_them():
    m2, m4 = rc.rule_lists("m2"), rc.rule_lists("m4")
    assert len(m2) >= 5 and len(m4) >= 5
    for tag, ij, sim in m2:
        rows = [(int(a), int(b), s) for (a, b), s in zip(ij, sim)]
        want = sorted(rows, key=lambda x: x[2], reverse=True)                 # visualize_matches.py:150
        for best in (100, len(sim)):
            om, ov, oc, _ = rc.rank_ref(*rc.padded(ij, sim), min(best, len(sim)))
            kept = int(oc[0])
            assert kept == min(best, len(sim))
            assert [tuple(r) for r in om[0, :kept].tolist()] == [(a, b) for a, b, _ in want[:kept]], tag
            assert rc.same_bits(ov[0, :kept], np.array([s for *_, s in want[:kept]], np.float32)), tag
    for tag, mt, dist in m4:
        om, ov, oc, osl = rc.rank_ref(*rc.padded(mt, dist), len(dist), ascending=True)
        assert np.all(np.diff(ov[0]) >= 0) and rc.same_bits(ov[0], np.sort(dist)), tag
        assert np.array_equal(om[0], mt[np.argsort(dist, kind="stable")]), tag
        ties = np.diff(ov[0]) == 0
        assert np.all(np.diff(osl[0])[ties] > 0), (tag, "equal distances keep their input order")


def test_rank_ref_states_the_order_on_the_edge_values():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    v = np.array([[0.0, nan, -0.0, inf, 1.0, -inf, 1.0, -nan, 0.0]], np.float32)
    m = rc.slot_matches(1, 9)
    for asc, want in ((False, [3, 4, 6, 0, 2, 8, 5, 1, 7]), (True, [5, 0, 2, 8, 4, 6, 3, 1, 7])):
        om, ov, oc, osl = rc.rank_ref(m, v, np.array([9]), 9, ascending=asc)
        assert osl[0].tolist() == want and oc[0] == 9 and rc.same_bits(ov[0], v[0, want])
    # the count is clamped, the tail zeroed
    for count, kept in ((-5, 0), (0, 0), (4, 4), (16, 5)):
        om, ov, oc, osl = rc.rank_ref(m, v, np.array([count]), 5)
        assert oc[0] == kept and not om[0, kept:].any() and not ov[0, kept:].view(np.uint32).any() and not osl[0, kept:].any()
