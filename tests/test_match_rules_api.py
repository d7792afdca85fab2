"""The rule matchers (M2 / M4 / M5 as a device-side finalize stage) and the rows-only similarity, as far as a machine without a GPU
can see them: the four entries against the header, the built library and sslam_amd.lib; the host-side refusals of the C entries,
which return before anything is launched; MatchRule's ValueErrors and the IndexError of M4 on one candidate, which come before
any device work; the signatures `rule=None` leaves alone; and the condition on the inputs of tests/test_gpu_match_rules.py -
checked on the oracle alone - that every rule's middle threshold keeps some rows and rejects others."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import match_rules_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sslam_match_finalize_rule", "sslam_match_finalize_rule_pairs", "sslam_sim_argmax_rows", "sslam_sim_argmax_rows_pairs")
E_INVALID = -1
RATIO_BEST, RATIO_SECOND, TRACKED = 1, 2, 3
# never dereferenced: every call below is refused by the entry's own checks, which come before the launch
GOOD, GOOD2, ODD = 0x10000, 0x20000, 0x10004


def test_rule_entries_are_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sslam_hip.h")).read()
    so = ctypes.CDLL(lib.SO_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, flags=re.M), f"{name} is not declared in include/sslam_hip.h"
        assert name in lib.EXPORTS
        assert hasattr(so, name), f"{name} is not exported by the library"
    for macro, v in (("SSLAM_RULE_RATIO_BEST", 1), ("SSLAM_RULE_RATIO_SECOND", 2), ("SSLAM_RULE_TRACKED", 3)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(v) + r"\b", hdr), macro
    assert (lib.RULE_RATIO_BEST, lib.RULE_RATIO_SECOND, lib.RULE_TRACKED) == (1, 2, 3)
    L = lib.lib()
    # finalize: the four arg-max arrays, sizes, rule + param, three outputs, stream; the pair-list form adds the lists and n_bank
    assert len(L.sslam_match_finalize_rule.argtypes) == 13
    assert len(L.sslam_match_finalize_rule_pairs.argtypes) == 15
    # rows-only: the full entries without nn21, s21 (and, having no single-evaluation form, without the workspace pair)
    assert len(L.sslam_sim_argmax_rows.argtypes) == len(L.sslam_sim_argmax.argtypes) - 2
    assert len(L.sslam_sim_argmax_rows_pairs.argtypes) == len(L.sslam_sim_argmax_pairs.argtypes) - 4
    assert L.sslam_version() > 400, "a new entry raises the version"
    # the header cites the reference lines each rule restates
    for cite in ("visualize_matches.py:102-124", "test/test_descriptor_quality.py:97-142", "test/test_tracking.py:158-161"):
        assert cite in hdr, cite


def _fin(L, nn12=GOOD, s12=GOOD, second12=GOOD, nn21=GOOD, n1=4, n2=4, n_pairs=2, rule=RATIO_BEST, matches=GOOD, value=GOOD, count=GOOD):
    return L.sslam_match_finalize_rule(nn12, s12, second12, nn21, n1, n2, n_pairs, rule, ctypes.c_float(0.8), matches, value, count, None)


def _fin_pairs(L, nn12=GOOD, s12=GOOD, second12=GOOD, nn21=GOOD, K=4, n_bank=4, first=GOOD2, second=GOOD2, n_pairs=2, rule=RATIO_BEST,
               matches=GOOD, value=GOOD, count=GOOD):
    return L.sslam_match_finalize_rule_pairs(nn12, s12, second12, nn21, K, n_bank, first, second, n_pairs, rule, ctypes.c_float(0.8),
                                             matches, value, count, None)


def _rows(L, d1=GOOD, stride1=512, n1=4, d2=GOOD, stride2=512, n2=4, n_pairs=2, nn12=GOOD):
    return L.sslam_sim_argmax_rows(d1, stride1, n1, d2, stride2, n2, n_pairs, nn12, None, None, None)


def _rows_pairs(L, bank=GOOD, stride=512, n_bank=4, K=4, first=GOOD2, second=GOOD2, n_pairs=2, nn12=GOOD):
    return L.sslam_sim_argmax_rows_pairs(bank, stride, n_bank, K, first, second, n_pairs, nn12, None, None, None)


def test_c_entries_refuse_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    before = lib.launch_count()
    bad_fin = [dict(nn12=None), dict(s12=None), dict(matches=None), dict(value=None), dict(count=None),
               dict(n_pairs=0), dict(n_pairs=-2), dict(rule=0), dict(rule=4), dict(rule=-1)]
    # a NULL array the rule reads; M4 on fewer than two candidates (the reference raises there), whatever else is right
    bad_fin += [dict(rule=r, second12=None) for r in (RATIO_BEST, RATIO_SECOND)]
    bad_fin += [dict(rule=r, nn21=None) for r in (RATIO_BEST, RATIO_SECOND)]
    for kw in bad_fin + [dict(n1=0), dict(n2=0), dict(rule=RATIO_SECOND, n2=1)]:
        assert _fin(L, **kw) == E_INVALID, kw
    for kw in bad_fin + [dict(K=0), dict(n_bank=0), dict(rule=RATIO_SECOND, K=1), dict(first=None), dict(second=None),
                         dict(first=GOOD2 + 2), dict(second=GOOD2 + 1)]:
        assert _fin_pairs(L, **kw) == E_INVALID, kw
    for kw in (dict(d1=None), dict(d2=None), dict(nn12=None), dict(n1=0), dict(n2=-1), dict(n_pairs=0), dict(d1=ODD), dict(d2=ODD),
               dict(stride1=510), dict(stride2=2)):
        assert _rows(L, **kw) == E_INVALID, kw
    for kw in (dict(bank=None), dict(first=None), dict(second=None), dict(nn12=None), dict(n_pairs=0), dict(K=0), dict(n_bank=0),
               dict(bank=ODD), dict(stride=510), dict(first=GOOD2 + 2), dict(second=GOOD2 + 1)):
        assert _rows_pairs(L, **kw) == E_INVALID, kw
    assert lib.launch_count() == before, "a refused call launches nothing"


def test_binding_refuses_malformed_arrays_before_any_device_work():
    from sslam_amd import lib
    nn = torch.zeros((2, 4), dtype=torch.int32)                # host tensors: a check that let them through would fail on the device
    first, second = torch.tensor([0, 1], dtype=torch.int32), torch.tensor([1, 2], dtype=torch.int32)
    before = lib.launch_count()
    with pytest.raises(ValueError, match="int32"):
        lib.match_finalize_rule_pairs(nn, nn.float(), nn.float(), nn, first.long(), second.long(), 3, lib.RULE_RATIO_BEST, 0.8)
    with pytest.raises(ValueError, match="second12"):
        lib.match_finalize_rule_pairs(nn, nn.float(), None, nn, first, second, 3, lib.RULE_RATIO_BEST, 0.8)
    with pytest.raises(ValueError, match="nn21"):
        lib.match_finalize_rule_pairs(nn, nn.float(), nn.float(), None, first, second, 3, lib.RULE_RATIO_SECOND, 0.9)
    with pytest.raises(ValueError, match="s12"):
        lib.match_finalize_rule_pairs(nn, nn.float()[:, :3], None, None, first, second, 3, lib.RULE_TRACKED, 0.8)
    with pytest.raises(ValueError, match="value"):
        lib.match_finalize_rule(nn, nn.float(), None, None, 4, 4, 2, lib.RULE_TRACKED, 0.8,
                                out=(torch.zeros((2, 4, 2), dtype=torch.int64), torch.zeros((2, 3)), torch.zeros((2,), dtype=torch.int32)))
    # the strided binding checks the arrays the kernel reads and writes row for row like the pair-list one
    with pytest.raises(ValueError, match="nn12"):
        lib.match_finalize_rule(nn.long(), nn.float(), None, None, 4, 4, 2, lib.RULE_TRACKED, 0.8)
    with pytest.raises(ValueError, match="s12"):
        lib.match_finalize_rule(nn, nn.float()[:1], None, None, 4, 4, 2, lib.RULE_TRACKED, 0.8)
    with pytest.raises(ValueError, match="second12"):
        lib.match_finalize_rule(nn, nn.float(), None, nn, 4, 4, 2, lib.RULE_RATIO_BEST, 0.8)
    with pytest.raises(ValueError, match="nn21"):
        lib.match_finalize_rule(nn, nn.float(), nn.float(), nn[:, :3], 4, 4, 2, lib.RULE_RATIO_SECOND, 0.9)
    d = torch.zeros((2, 4, lib.D_OUT))
    with pytest.raises(ValueError, match="s12"):
        lib.sim_argmax_rows(d, 4 * lib.D_OUT, 4, d, 4 * lib.D_OUT, 4, 2, out=(nn, nn.float()[:, :2], None))
    with pytest.raises(ValueError, match="nn12"):
        lib.sim_argmax_rows(d, 4 * lib.D_OUT, 4, d, 4 * lib.D_OUT, 4, 2, out=(nn.float(), nn.float(), None))
    with pytest.raises(ValueError, match="bank"):
        lib.sim_argmax_rows_pairs(torch.zeros((3, 4, 64)), first, second)
    with pytest.raises(ValueError, match="unequal"):
        lib.sim_argmax_rows_pairs(torch.zeros((3, 4, lib.D_OUT)), first, second[:1])
    with pytest.raises(ValueError):                             # well-formed host tensors: refused for where they live
        lib.sim_argmax_rows_pairs(torch.zeros((3, 4, lib.D_OUT)), first, second)
    assert lib.launch_count() == before


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), "0.8", None, True, [0.8], 1e39, 1 + 2j])
def test_match_rule_refuses_bad_parameters(bad):
    from sslam_amd.pipeline import MatchRule
    for make in (MatchRule.ratio, MatchRule.mnn_ratio, MatchRule.tracked):
        with pytest.raises(ValueError):
            make(bad)


def test_match_rule_constructors_are_the_references():
    from sslam_amd import lib
    from sslam_amd.pipeline import MatchRule
    # names and defaults: visualize_matches.py:102, test/test_descriptor_quality.py:101, test/test_tracking.py (match_threshold=0.8)
    for make, arg, default, kind in ((MatchRule.ratio, "ratio_thresh", 0.8, lib.RULE_RATIO_BEST),
                                     (MatchRule.mnn_ratio, "ratio_threshold", 0.9, lib.RULE_RATIO_SECOND),
                                     (MatchRule.tracked, "match_threshold", 0.8, lib.RULE_TRACKED)):
        (p,) = inspect.signature(make).parameters.values()
        assert (p.name, p.default) == (arg, default)
        r = make()
        assert r.kind == kind and r.param == float(np.float32(default)), "the parameter is rounded to fp32 once"
        assert make(**{arg: np.float32(0.75)}).param == 0.75 and make(1).param == 1.0
        with pytest.raises(Exception):                          # frozen
            r.param = 0.5
    with pytest.raises(ValueError):
        MatchRule(7, 0.5)
    with pytest.raises(ValueError):
        MatchRule(lib.RULE_TRACKED, 0.8)                        # 0.8 is no fp32 value: the constructors round


def test_rule_none_leaves_the_signatures_alone():
    from sslam_amd.harness import StreamingSequence, run_directory, run_frames
    from sslam_amd.online import FrameStepper, RuleFrameStepper
    from sslam_amd.pipeline import SequencePipeline
    sig = lambda f: list(inspect.signature(f).parameters.values())       # noqa: E731
    m, mp = sig(SequencePipeline.match), sig(SequencePipeline.match_pairs)
    assert [p.name for p in m] == ["self", "desc", "scores", "intensity", "spacing", "out", "rule"]
    assert [p.name for p in mp] == ["self", "desc", "scores", "intensity", "first", "second", "out", "rule"]
    assert [p.default for p in m[3:]] == [None] * 4 and [p.default for p in mp[3:]] == [None] * 5
    for f in (StreamingSequence.__init__, run_frames, run_directory, RuleFrameStepper.__init__):
        assert sig(f)[-1].name == "rule" and sig(f)[-1].default is None, f
    # FrameStepper's constructor is pinned (test_match_pairs_api.py): the rule comes through RuleFrameStepper, the same
    # arguments in the same order + rule
    assert [p.name for p in sig(RuleFrameStepper.__init__)][:-1] == [p.name for p in sig(FrameStepper.__init__)]
    assert [p.default for p in sig(RuleFrameStepper.__init__)][4:-1] == [p.default for p in sig(FrameStepper.__init__)][4:]
    assert FrameStepper.rule is None and issubclass(RuleFrameStepper, FrameStepper)


def test_pipeline_refuses_bad_rules_before_any_device_work():
    from sslam_amd import lib
    from sslam_amd.online import RuleFrameStepper
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    pipe = SequencePipeline.__new__(SequencePipeline)          # no packing, no device: the checks come first
    pipe.cfg = ExtractorConfig()
    before = lib.launch_count()
    desc, scores = torch.zeros((3, 4, lib.D_OUT)), torch.zeros((3, 4))
    for bad in (0.8, "tracked", lib.RULE_TRACKED):
        with pytest.raises(ValueError, match="MatchRule"):
            pipe.match(desc, scores, rule=bad)
        with pytest.raises(ValueError, match="MatchRule"):
            pipe.match_pairs(desc, scores, first=[0], second=[1], rule=bad)
        with pytest.raises(ValueError, match="MatchRule"):
            RuleFrameStepper(pipe, 480, 640, tokens_in=True, rule=bad)
    # M4 on one candidate per row: the reference's np.sort(sim_matrix, axis=1)[:, 1] raises IndexError
    one, one_s = torch.zeros((3, 1, lib.D_OUT)), torch.zeros((3, 1))
    with pytest.raises(IndexError, match="index 1 is out of bounds"):
        pipe.match(one, one_s, rule=MatchRule.mnn_ratio())
    with pytest.raises(IndexError, match="index 1 is out of bounds"):
        pipe.match_pairs(one, one_s, first=[0], second=[1], rule=MatchRule.mnn_ratio())
    # an empty batch gives empty arrays under the rule's keys: `value`, and no `quality` to mistake a distance for
    empty = pipe.match(desc[:1], scores[:1], spacing=1, rule=MatchRule.mnn_ratio())
    assert set(empty) == {"matches", "value", "match_count"} and empty["value"].shape == (0, 4)
    assert set(pipe.match(desc[:1], scores[:1], spacing=1)) == {"matches", "quality", "match_count"}
    assert lib.launch_count() == before


def test_streaming_scheduler_calls_a_rule_less_pipeline_as_before():
    """rule=None adds no argument to the pipeline calls (pipelines other than SequencePipeline may not know `rule`); a rule is
    handed to alloc_match and match."""
    from sslam_amd.harness import StreamingSequence
    seen = []

    class _Pipe:
        def alloc_extract(self, n, with_intensity):
            return {"descriptors": torch.zeros((n,)), "scores": torch.zeros((n,))}

        def alloc_match(self, n_pairs, **kw):
            seen.append(("alloc", kw))
            return {"match_count": torch.zeros((n_pairs,), dtype=torch.int32)}

        def extract(self, tokens, images=None, out=None, images_ready=None):
            return out if out is not None else {"descriptors": tokens.clone(), "scores": tokens.clone()}

        def match(self, desc, scores, intensity=None, spacing=1, out=None, **kw):
            seen.append(("match", kw))
            return dict(out) if out is not None else self.alloc_match(desc.shape[0] - spacing)

    frames = torch.arange(5, dtype=torch.float32)
    StreamingSequence(_Pipe(), (1, 2)).run(frames)
    assert seen and all(kw == {} for _, kw in seen)
    del seen[:]
    ring = StreamingSequence(_Pipe(), (1, 2), rule="R")
    ring.run(frames)
    ring.reset()
    ring.push(frames)
    assert {what for what, _ in seen} == {"alloc", "match"} and all(kw == {"rule": "R"} for what, kw in seen if what == "match")
    assert all(kw in ({}, {"rule": "R"}) for what, kw in seen if what == "alloc") and ("alloc", {"rule": "R"}) in seen


def test_middle_thresholds_select_on_the_synthetic_sequence():
    """The input condition of test_gpu_match_rules.py, on the oracle alone: on pairs (0, 1), (0, 2), (0, 5) of the 6 extracted
    frames every rule's middle threshold keeps a count strictly between 0 and the count its loosest threshold keeps."""
    assert np.array_equal(mc.synth.token_sequence(27, 28)[:mc.N_COND], mc.synth.token_sequence(mc.N_COND, 28)), \
        "the GPU tests take the 6 frames as the head of their 27-frame sequence"
    desc = mc.oracle_descriptors()
    for name, ths in mc.THRESHOLDS.items():
        for i, j in mc.CONDITION_PAIRS:
            counts = {th: len(mc.oracle_rule(name, desc[i], desc[j], th)[0]) for th in ths}
            assert 0 < counts[mc.MIDDLE[name]] < counts[mc.LOOSEST[name]] <= mc.K, (name, i, j, counts)
            assert max(counts.values()) == counts[mc.LOOSEST[name]]
