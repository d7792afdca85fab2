"""Where the operands lie: every entry of libsslam_hip.so that takes device pointers, run with each operand at the LEAST alignment
include/sslam_hip.h states for it and at the loosest strides it accepts (tests/loose_table.py is that contract as a table;
tests/test_loose_operands_table.py holds the table against the header and against sslam_amd.lib.EXPORTS).

The rest of the GPU suite hands the entries whole torch allocations - 256-byte aligned - and dense strides.  A kernel that rounds
an address down, assumes a row starts on a cache line, or assumes frames a multiple of 512 bytes apart is right there and wrong
for a caller that carves its buffers from one arena.  Here every CASE of the guarded tests (tests/test_gpu_guarded_outputs.py,
the four pose files: their builders, their oracles, their assertions - called, not copied) runs under a guarded.Placement:

  placement   every operand of the call at once at its stated alignment a and no better, twice: a bytes past a 256-byte boundary
              ("lo") and a bytes before one ("hi"; a = 1: 1 and 3 bytes past).  Workspaces too, at their advertised size.  The
              case's own assertions hold: guards intact, every payload element written, inputs unchanged, the oracle bit for
              bit.  Cases without an exact oracle also equal their own aligned run byte for byte.
  strides     for the entries with a stride argument: dense + 4 floats, no multiple of the row width, frames narrower than the
              stride, 0 on each side, negative (served: include/sslam_hip.h); the gaps hold NaN bits; the oracle per pair on the
              dense data.
  refusals    every pointer of the entry once at half its alignment, inside a real guarded buffer: SSLAM_E_INVALID, nothing
              launched over all of them, every output still the sentinel.

The entry under test is caught at sslam_amd.lib._run, through which every call of the package goes: that is where a row checks
that its entry ran, where the entries without a width or form argument are reached from the cases of their _d / _form siblings
(the call is re-sent to them with that argument dropped), and where the refusals are made with the case's own arguments.

Run on the GPU box: python -m pytest tests/test_gpu_loose_operands.py -m gpu -q
"""
import ctypes as C

import numpy as np
import pytest

import guarded as gd
import loose_table as lt
import test_gpu_guarded_outputs as go
from test_gpu_guarded_outputs import Bufs, assert_bits

pytestmark = pytest.mark.gpu


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


class _Refused(Exception):
    """Ends a case once its entry's refusals are made."""


class Catch:
    """sslam_amd.lib._run for the time of one case: counts the calls of `entry`, re-sends a sibling's call to it, makes the refusals."""

    def __init__(self, T, hip, entry, via=None, refuse=False):
        self.T, self.hip, self.entry, self.via, self.refuse = T, hip, entry, via, refuse
        self.ran, self.refused, self.orig = 0, [], hip._run

    def __call__(self, what, fn, tensors, *args):
        name = fn.__name__
        if gd.placement is None:          # a plain call a case compares with (_unplaced): not the call under test
            return self.orig(what, fn, tensors, *args)
        if self.via is not None and name == self.via[0]:
            fn, args, name = getattr(self.hip.lib(), self.entry), self.via[1](args), self.entry
        if name == self.entry:
            if self.refuse:
                self.refusals(fn, tensors, args)
                raise _Refused()
            self.ran += 1
        return self.orig(what, fn, tensors, *args)

    def direct(self, fn):
        """For the one wrapper that calls its entry itself (it turns SSLAM_E_UNSUPPORTED into None): what to put in the loaded
        library's place of `fn` - the same catch, the stream being the call's last argument."""
        def call(*args):
            if self.refuse:
                self.refusals(fn, None, args[:-1])
                raise _Refused()
            self.ran += 1
            return fn(*args)
        return call

    def refusals(self, fn, tensors, args):
        T, hip, p = self.T, self.hip, gd.placement
        dev = hip.common_device(*tensors) if tensors is not None else T.device("cuda", T.cuda.current_device())
        n0, mine = hip.launch_count(), []
        for i, arg in enumerate(args):
            if not isinstance(arg, C.c_void_p) or not arg.value:
                continue
            rec = [r for r in p.made if r["middle"].numel() and
                   r["middle"].data_ptr() <= arg.value < r["middle"].data_ptr() + r["middle"].numel() * r["middle"].element_size()]
            assert len(rec) == 1, f"{self.entry}: pointer argument {i} is no placed operand of the case"
            a = rec[0]["align"]
            mine.append(rec[0])
            if a == 1:
                continue
            bad = args[:i] + (C.c_void_p(arg.value + a // 2),) + args[i + 1:]
            with T.cuda.device(dev):
                rc = fn(*bad, C.c_void_p(T.cuda.current_stream(dev).cuda_stream))
            want = hip.E_UNSUPPORTED if (self.entry, rec[0]["name"]) in lt.REFUSED_AS_UNSUPPORTED else hip.E_INVALID
            assert rc == want, f"{self.entry}: {rec[0]['name']} {a // 2} bytes off its {a}-byte alignment returned {rc}, not {want}"
            self.refused.append(rec[0]["name"])
        T.cuda.synchronize()
        assert hip.launch_count() == n0, f"{self.entry}: a refused call launched something"
        for r in mine:          # the outputs of THIS call (a case may have run a sibling entry before)
            if r["kind"] == "out":
                gd.assert_guards(r["whole"], r["middle"], f"{self.entry} refused: {r['name']}")
                idt, sentinel = gd._int_view(T, r["middle"].dtype)
                assert bool((r["middle"].reshape(-1).view(idt) == sentinel).all()), f"{self.entry}: a refused call wrote {r['name']}"


def _aligns(entry, also=()):
    out = {}
    for e in (entry,) + tuple(also):
        for k, v in lt.ALIGN[e].items():
            assert out.setdefault(k, v) == v, f"{k} of {e} is stated otherwise for another entry of the same case"
    return out


def _outputs(T, p):
    return [go._bytes(go._host(T, r["middle"])).copy() for r in p.made if r["kind"] == "out"]


def _at_its_alignment(p):
    for r in p.made:
        a, at = r["align"], r["middle"].data_ptr()
        assert not r["middle"].numel() or a == 1 or (at % a == 0 and at % (2 * a) != 0), (r["name"], a, at % 256)


DIRECT = ("sslam_preprocess_u8_patches",)          # called by its wrapper without lib._run


def _caught(monkeypatch, hip, catch, case):
    """The case with `catch` in lib._run's place (and, for a DIRECT entry, in the entry's own)."""
    with monkeypatch.context() as m:
        m.setattr(hip, "_run", catch)
        if catch.entry in DIRECT:
            m.setattr(hip.lib(), catch.entry, catch.direct(getattr(hip.lib(), catch.entry)))
        case()


def run_placed(T, hip, monkeypatch, entry, case, via=None, also=(), aligned_too=False):
    """The case with every operand at its least alignment, just past and just before a 256-byte boundary."""
    aligns, runs = _aligns(entry, also), {}
    for mode in (("aligned",) if aligned_too else ()) + ("lo", "hi"):
        catch = Catch(T, hip, entry, via)
        with gd.placed(gd.Placement(aligns, mode)) as p:
            _caught(monkeypatch, hip, catch, case)
        assert catch.ran >= 1, f"the case never called {entry}"
        assert p.made, "the case placed nothing"
        if mode != "aligned":
            _at_its_alignment(p)
        runs[mode] = _outputs(T, p)
    if aligned_too:
        for mode in ("lo", "hi"):
            assert len(runs[mode]) == len(runs["aligned"])
            for k, (a, b) in enumerate(zip(runs["aligned"], runs[mode])):
                assert np.array_equal(a, b), f"{entry}: output {k} at placement '{mode}' differs from the aligned run"


def run_refusals(T, hip, monkeypatch, entry, case, via=None, also=()):
    """Every pointer of the entry at half its alignment, with the case's own arguments; the case must pass every pointer."""
    catch = Catch(T, hip, entry, via, refuse=True)
    with gd.placed(gd.Placement(_aligns(entry, also), "aligned")):
        with pytest.raises(_Refused):
            _caught(monkeypatch, hip, catch, case)
    want = sorted(k for k, a in lt.ALIGN[entry].items() if a > 1)
    assert sorted(catch.refused) == want, f"{entry}: refused {sorted(catch.refused)}, the table names {want}"


# ================================================================================================================ the table
# entry -> dict(cases={id: callable(F)}, refuse=id of the case that passes every pointer, via=(sibling, its arguments -> the
# entry's), also=other entries the cases call with guarded operands, aligned_too=no exact oracle).  F: the fixtures (T, hip, knob).
class F:
    def __init__(self, T, hip, knob):
        self.T, self.hip, self.knob = T, hip, knob


def _drop(*idx):
    """Arguments with the positions idx (negative: from the end) removed: a _d or _form call as its sibling takes it."""
    return lambda args: tuple(a for i, a in enumerate(args) if i not in idx and i - len(args) not in idx)


_same = lambda args: args          # the ViT wrappers add the form themselves (lib._with_form): the sibling takes the call as it stands
TABLE = {}


def row(entry, cases, refuse=None, via=None, also=(), aligned_too=False):
    assert entry in lt.ALIGN and entry not in TABLE, entry
    TABLE[entry] = dict(cases=cases, refuse=refuse or next(iter(cases)), via=via, also=tuple(also), aligned_too=aligned_too)


# ---- A0 / A9: every shape of the guarded file reaches another kernel form
row("sslam_preprocess_u8", {f"{h}x{w}_{s}": (lambda f, a=(h, w, s): go.test_preprocess_u8(f.T, f.hip, *a, 0)) for h, w, s in go.A0_SHAPES})
row("sslam_preprocess_u8_patches",
    {f"{h}x{w}_{s}": (lambda f, a=(h, w, s): go.test_preprocess_u8_patches(f.T, f.hip, *a, 0)) for h, w, s in go.A0_SHAPES})
row("sslam_keypoint_intensity",
    {f"{h}x{w}_{s}": (lambda f, a=(h, w, s): go.test_keypoint_intensity(f.T, f.hip, *a, 0)) for h, w, s in go.A0_SHAPES[2:4]})

# ---- A2: the three register forms (one grid each), three sweeps by size, and the three other ways into the sweep kernel
_BN = [(3, "register"), (28, "register"), (40, "register"), (60, "register"), (61, "register"), (29, "sweeps_knob"), (29, "sweeps_group2"),
       (29, "sweeps_eval")]
row("sslam_bn_tokens", {f"g{g}_{form}": (lambda f, a=(g, form): go.test_bn_tokens(f.T, f.hip, f.knob, *a, 5, False)) for g, form in _BN},
    refuse="g28_register")
row("sslam_bn_tokens_bf16copy", {f"g{g}_{form}": (lambda f, a=(g, form): go.test_bn_tokens(f.T, f.hip, f.knob, *a, 5, True)) for g, form in _BN},
    refuse="g28_register")

# ---- A3: every form at 28 x 28 x 3, the per-frame tiling at 44, hs 128
_SEL = [(28, 3, 256, form) for form in go.SEL_FORMS] + [(44, 3, 256, "throughput"), (44, 3, 256, "throughput_tail"), (5, 2, 256, "latency2"),
                                                         (28, 2, 128, "stage_v0"), (28, 2, 128, "throughput")]
_sel_cases = {f"g{g}x{n}_hs{hs}_{form}": (lambda f, a=(g, n, hs, form): go.test_selector_saliency(f.T, f.hip, f.knob, *a)) for g, n, hs, form in _SEL}
row("sslam_selector_saliency_ws", _sel_cases, refuse="g28x3_hs256_latency2", also=("sslam_selector_saliency",))
row("sslam_selector_saliency", _sel_cases, refuse="g28x3_hs256_latency", also=("sslam_selector_saliency_ws",))
row("sslam_selector_saliency_bf16",
    {f"g{g}x{n}_{form}": (lambda f, a=(g, n, form): go.test_selector_saliency_bf16(f.T, f.hip, f.knob, *a))
     for g, n, form in [(28, 3, form) for form in go.BF_FORMS] + [(44, 3, "halo"), (5, 2, "halo_tail2")]})
row("sslam_f32_to_bf16", {f"n{n}": (lambda f, n=n: go.test_f32_to_bf16(f.T, f.hip, n)) for n in (8, 8 * 257)})

# ---- A4 / A5
row("sslam_select_keypoints",
    {f"{name}_{opt}": (lambda f, a=(name, opt): go.test_select_keypoints(f.T, f.hip, *a))
     for name, opt in [("g7_k20", "idx_px"), ("g7_k60", "idx_px"), ("g64_k4096", "idx_px"), (go.SELECT_TAGS[0], "idx_px"), ("g7_k20", "neither")]})

# ---- A6 / A7: ragged tiles in one and in several workgroups, both widths, the direct and the distinct-row launch
_REF = [go.REF_SHAPES[1], go.REF_SHAPES[2]]
row("sslam_gather", {f"g{g}_k{k}x{n}": (lambda f, a=(g, k, n): go.test_gather(f.T, f.hip, *a)) for g, k, n in _REF})
_refine = lambda width: {f"g{g}_k{k}x{n}_depth{d}": (lambda f, a=(g, k, n, width, d): go.test_refine(f.T, f.hip, *a)) for g, k, n in _REF for d in (0, 2)}
_gr = lambda width: {f"g{g}_k{k}x{n}_depth{d}_distinct{x}": (lambda f, a=(g, k, n, width, d, x): go.test_gather_refine(f.T, f.hip, f.knob, *a))
                     for g, k, n in _REF for d in (0, 2) for x in (0, 1)}
_gr_all = {**{"w128_" + k: v for k, v in _gr(128).items()}, **{"w256_" + k: v for k, v in _gr(256).items()}}
row("sslam_refine_d", {**{"w128_" + k: v for k, v in _refine(128).items()}, **{"w256_" + k: v for k, v in _refine(256).items()}})
row("sslam_refine", _refine(128), via=("sslam_refine_d", _drop(-1)))
row("sslam_gather_refine_ws_d", _gr_all, refuse="w128_g28_k129x3_depth2_distinct1")
row("sslam_gather_refine_ws", _gr(128), refuse="g28_k129x3_depth2_distinct1", via=("sslam_gather_refine_ws_d", _drop(-1)))
row("sslam_gather_refine_d", {k: v for k, v in _gr_all.items() if k.endswith("distinct0")}, via=("sslam_gather_refine_ws_d", _drop(-3, -2)),
    also=("sslam_gather_refine_ws_d",))
row("sslam_gather_refine", {k: v for k, v in _gr(128).items() if k.endswith("distinct0")}, via=("sslam_gather_refine_ws_d", _drop(-3, -2, -1)),
    also=("sslam_gather_refine_ws_d",))
_bf = {f"g{g}_k{k}x{n}_depth{d}": (lambda f, a=(g, k, n, d): go.test_refine_bf16_and_gather_refine_bf16(f.T, f.hip, *a)) for g, k, n in _REF for d in (0, 2)}
row("sslam_refine_bf16", _bf, also=("sslam_gather_refine_bf16",), aligned_too=True)
row("sslam_gather_refine_bf16", _bf, also=("sslam_refine_bf16",), aligned_too=True)

# ---- M1: both launch forms, both widths, ragged query blocks; the siblings without width / workspace through the same cases
_SIM = [(33, 70), (129, 65)]
_sim = lambda widths: {f"{n1}x{n2}_w{w}_{form}": (lambda f, a=(n1, n2, w, form): go.test_sim_argmax_strided(f.T, f.hip, f.knob, *a, "s21_second"))
                       for n1, n2 in _SIM for w in widths for form in go.SIM_FORMS}
_listed = lambda widths: {f"k{k}_w{w}_{form}": (lambda f, a=(k, w, form): go.test_sim_argmax_listed(f.T, f.hip, f.knob, *a, "s21_second"))
                          for k in (33, 129) for w in widths for form in go.SIM_FORMS}
_rows = lambda widths: {f"{n1}x{n2}_w{w}_p{p}": (lambda f, a=(n1, n2, w, p): go.test_sim_argmax_rows(f.T, f.hip, *a, True))
                        for n1, n2 in _SIM for w in widths for p in (3, 17)}
_rowsp = lambda widths: {f"k{k}_w{w}_p{p}": (lambda f, a=(k, w, p): go.test_sim_argmax_rows_pairs(f.T, f.hip, *a, True))
                         for k in (33, 129) for w in widths for p in (3, 17)}
_one_pass = lambda cases: {k: v for k, v in cases.items() if not k.endswith("two_pass_3")}
_two_pass = lambda cases: {k: v for k, v in cases.items() if k.endswith("two_pass_3")}
row("sslam_sim_argmax_ws_d", _sim((128, 256)), refuse="33x70_w128_default_17")
row("sslam_sim_argmax_ws", _sim((128,)), refuse="33x70_w128_default_17", via=("sslam_sim_argmax_ws_d", _drop(-1)))
row("sslam_sim_argmax_d", _two_pass(_sim((128, 256))), via=("sslam_sim_argmax_ws_d", _drop(-3, -2)))
row("sslam_sim_argmax", _two_pass(_sim((128,))), via=("sslam_sim_argmax_ws_d", _drop(-3, -2, -1)))
row("sslam_sim_argmax_pairs_d", _listed((128, 256)), refuse="k33_w128_default_17")
row("sslam_sim_argmax_pairs", _listed((128,)), refuse="k33_w128_default_17", via=("sslam_sim_argmax_pairs_d", _drop(-1)))
row("sslam_sim_argmax_rows_d", _rows((128, 256)))
row("sslam_sim_argmax_rows", _rows((128,)), via=("sslam_sim_argmax_rows_d", _drop(-1)))
row("sslam_sim_argmax_rows_pairs_d", _rowsp((128, 256)))
row("sslam_sim_argmax_rows_pairs", _rowsp((128,)), via=("sslam_sim_argmax_rows_pairs_d", _drop(-1)))

_RUN = "cli"          # the run of test_oracle_golden.RUNS that passes both intensity arrays
assert "intensity1" in go.RUNS[_RUN](None, None)
row("sslam_match_finalize", {f"{n1}x{n2}_p{p}": (lambda f, a=(n1, n2, p): go.test_match_finalize(f.T, f.hip, *a, _RUN)) for n1, n2 in _SIM for p in (3, 17)})
row("sslam_match_finalize_pairs", {f"k{k}_p{p}": (lambda f, a=(k, p): go.test_match_finalize_pairs(f.T, f.hip, *a, _RUN)) for k in (33, 129) for p in (3, 17)})
row("sslam_match_finalize_rule",
    {f"{n1}x{n2}_p{p}_{rule}": (lambda f, a=(n1, n2, p, rule): go.test_match_finalize_rule(f.T, f.hip, *a)) for n1, n2 in _SIM for p in (3, 17) for rule in go.RULES},
    refuse=f"33x70_p3_{go.mc.RATIO}")
row("sslam_match_finalize_rule_pairs",
    {f"k{k}_p{p}_{rule}": (lambda f, a=(k, p, rule): go.test_match_finalize_rule_pairs(f.T, f.hip, *a)) for k in (33, 129) for p in (3, 17) for rule in go.RULES},
    refuse=f"k33_p3_{go.mc.RATIO}")

# ---- A1: no exact oracle - the bars of tests/test_gpu_vit_reference.py, and the aligned run byte for byte
_vit = lambda entry: {f"{s}x{n}_{form}": (lambda f, a=(s, n, form, entry): go.test_vit_forward_bf16(f.T, f.hip, *a)) for s, n in go.VIT_SHAPES
                      for form in ("throughput", "few_frame")}
_vit32 = {f"{s}x{n}_{att}": (lambda f, a=(s, n, att): go.test_vit_forward_f32(f.T, f.hip, *a)) for s, n in go.VIT_SHAPES for att in ("one_pass", "key_split")}
row("sslam_vit_forward_form", _vit("images"), aligned_too=True)
row("sslam_vit_forward_patches_form", _vit("patches"), aligned_too=True)
row("sslam_vit_forward", {k: v for k, v in _vit("images").items() if k.endswith("throughput")}, via=("sslam_vit_forward_form", _same), aligned_too=True)
row("sslam_vit_forward_patches", {k: v for k, v in _vit("patches").items() if k.endswith("throughput")},
    via=("sslam_vit_forward_patches_form", _same), aligned_too=True)
row("sslam_vit_forward_f32_form", _vit32, aligned_too=True)
row("sslam_vit_forward_f32", {k: v for k, v in _vit32.items() if k.endswith("key_split")}, via=("sslam_vit_forward_f32_form", _same), aligned_too=True)


# ---- the pose entries: the guarded cases of their four files
def _pose_eval(f, posed):
    """The first group of tests/golden/pose_eval.npz without a homography (H = NULL) and the first with one."""
    import pose_eval_ref as pr
    import test_gpu_pose_eval as pe
    name = next(n for n in pr.group_names() if (pr.group(n)["H"] is not None) == posed)
    return pe.test_entries_equal_the_reference_and_the_restatement(f.T, name)


def _pose_depth(which, arg):
    import test_gpu_pose_depth as pd
    return lambda f: getattr(pd, which)(f.T, arg)


def _ransac(f, k=0):
    import test_gpu_pose_ransac as ra
    return ra.test_every_output_equals_the_restatement_bit_for_bit(f.T, *ra.CASE_SEEDS[k])


def _pose_refine(f, k=0):
    import pose_refine_cases as cases
    import test_gpu_pose_refine as rf
    return rf.test_every_output_equals_the_restatement_bit_for_bit(f.T, cases.NAMES[k])


_pe = {"raw": lambda f: _pose_eval(f, False), "posed": lambda f: _pose_eval(f, True)}
row("sslam_pose_nn_pairs", _pe, refuse="posed", also=("sslam_match_score_pairs",))
row("sslam_match_score_pairs", _pe, also=("sslam_pose_nn_pairs",))
row("sslam_keypoint_depth", {f"case{i}": _pose_depth("test_depth_gather_equals_the_restatement", i) for i in (0, 3)})
row("sslam_pose_depth_nn_pairs", {f"warp{i}": _pose_depth("test_warp_and_search_equal_the_restatement", i) for i in (0, 1)})
row("sslam_match_score_known_pairs", {"count": _pose_depth("test_score_entry_counts_unknown_rows_apart", "count")}, also=("sslam_match_score_pairs",))
row("sslam_pose_ransac_pairs", {"case0": _ransac, "last": lambda f: _ransac(f, -1)})
row("sslam_pose_refine_pairs", {"case0": _pose_refine, "last": lambda f: _pose_refine(f, -1)})


# ---- rank.hip and validate.hip: their own files guard only rows; here the cases of those files' builders in guarded buffers.
# rank: the reference order of tests/match_rank_cases.py bit for bit.  validate: no exact oracle - tests/test_gpu_validation_edges.py
# holds the plain call to float64; a placed call must give that plain call's bytes.
def _unplaced(fn):
    """fn() with the placement lifted: the plain call a placed one is compared with."""
    p, gd.placement = gd.placement, None
    try:
        return fn()
    finally:
        gd.placement = p


def rank_case(f, n1=300, best=100, ascending=False):
    import match_rank_cases as rc
    counts = [0, 1, n1 // 2, n1, 7]
    v, m = rc.random_values(n1, len(counts), n1), rc.slot_matches(len(counts), n1)
    want = rc.rank_ref(m, v, counts, best, ascending)
    b = Bufs(f.T)
    out = (b.o("out_matches", (len(counts), best, 2), f.T.int64), b.o("out_value", (len(counts), best)), b.o("out_count", (len(counts),), f.T.int32),
           b.o("out_slot", (len(counts), best), f.T.int32))
    f.hip.match_rank(b.i("matches", m), b.i("value", v), b.i("count", np.asarray(counts, np.int32)), best, ascending=ascending, out=out)
    b.check(f"match_rank n1 {n1} best {best}")
    for got, w, name in zip(out, want, ("out_matches", "out_value", "out_count", "out_slot")):
        assert_bits(f.T, got, np.asarray(w, go._host(f.T, got).dtype), name)


row("sslam_match_rank", {"n300_best100": rank_case, "n1000_all_ascending": lambda f: rank_case(f, 1000, 1000, True), "n64_best1": lambda f: rank_case(f, 64, 1)})


def _val_pair(n1=129, n2=37, width=128):
    import val_edge_cases as vec
    first, second = vec.rect_pair(n1, n2)
    if width == 256:
        first, second = (np.concatenate([x, x[..., ::-1]], -1) / np.float32(np.sqrt(2.0)) for x in (first, second))
    return np.ascontiguousarray(first, np.float32), np.ascontiguousarray(second, np.float32)


def _plain_pair(f, first, second, temperature=0.1):
    """The plain calls on dense, library-allocated tensors: (nn12, s12, nn21, lse, ce, s00) as numpy, per pair."""
    T, hip = f.T, f.hip
    P, n1, d = first.shape
    n2 = second.shape[1]

    def go_():
        d1, d2 = T.from_numpy(first).cuda(), T.from_numpy(second).cuda()
        nn12, s12, nn21, _, _ = hip.sim_argmax(d1, n1 * d, n1, d2, n2 * d, n2, P)
        lse, ce, s00 = hip.row_lse(d1, n1 * d, n1, d2, n2 * d, n2, P, s12, temperature)
        return [t.cpu().numpy() for t in (nn12, s12, nn21, lse, ce, s00)]
    return _unplaced(go_)


def row_lse_case(f, width=128, listed=False, temperature=0.1):
    T, hip = f.T, f.hip
    first, second = _val_pair(width=width)
    if listed:          # a bank of the two first frames and one more, pairs (0, 1), absent, (2, 0), (1, 1): n1 = n2 = K
        bank = np.ascontiguousarray(np.stack([first[0], first[1], np.roll(first[0], 5, axis=0)]))
        pf, ps = np.array([0, -1, 2, 1], np.int32), np.array([1, 0, 0, 1], np.int32)
        ok = [0, 2, 3]
        a, s = bank[pf[ok]], bank[ps[ok]]
        nn12, s12, nn21, lse, ce, s00 = _plain_pair(f, np.ascontiguousarray(a), np.ascontiguousarray(s), temperature)
        full = lambda x: np.stack([x[ok.index(p)] if p in ok else np.zeros_like(x[0]) for p in range(4)])
        b = Bufs(T)
        out = (b.o("lse", (4, bank.shape[1])), b.o("ce", (4, bank.shape[1])), b.o("s00", (4,)))
        hip.row_lse_pairs(b.i("bank", bank, guard=go._guard(width)), b.i("pair_first", pf), b.i("pair_second", ps), b.i("s12", full(s12)), temperature, out=out)
        b.check(f"row_lse_pairs width {width}")
        for got, w, name in zip(out, (lse, ce, s00), ("lse", "ce", "s00")):
            assert_bits(T, got, full(w), name)
        return
    P, n1, d = first.shape
    n2 = second.shape[1]
    nn12, s12, nn21, lse, ce, s00 = _plain_pair(f, first, second, temperature)
    b = Bufs(T)
    out = (b.o("lse", (P, n1)), b.o("ce", (P, n1)), b.o("s00", (P,)))
    hip.row_lse(b.i("desc1", first, guard=go._guard(width)), n1 * d, n1, b.i("desc2", second, guard=go._guard(width)), n2 * d, n2, P, b.i("s12", s12),
                temperature, out=out)
    b.check(f"row_lse width {width}")
    for got, w, name in zip(out, (lse, ce, s00), ("lse", "ce", "s00")):
        assert_bits(T, got, w, name)


row("sslam_row_lse_d", {"w128": row_lse_case, "w256": lambda f: row_lse_case(f, 256)})
row("sslam_row_lse", {"w128": row_lse_case}, via=("sslam_row_lse_d", _drop(-1)))
row("sslam_row_lse_pairs_d", {"w128": lambda f: row_lse_case(f, 128, True), "w256": lambda f: row_lse_case(f, 256, True)})
row("sslam_row_lse_pairs", {"w128": lambda f: row_lse_case(f, 128, True)}, via=("sslam_row_lse_pairs_d", _drop(-1)))


def _direct(f, what, entry, tensors, *args):
    f.hip._run(what, getattr(f.hip.lib(), entry), tensors, *args)


def edge_pool_case(f, size=544, n=2):
    import val_edge_cases as vec
    T, hip = f.T, f.hip
    img = vec.images(vec.KINDS[0], size, n)
    want = _unplaced(lambda: [t.cpu().numpy() for t in hip.edge_pool(T.from_numpy(np.ascontiguousarray(img)).cuda())])
    b = Bufs(T)
    out = (b.o("pooled", (n, size // 16, size // 16)), b.o("edge_max", (n,)))
    hip.edge_pool(b.i("images_chw", img, guard=gd.GUARD_WIDE), out=out)
    b.check(f"edge_pool {size} x {n}")
    for got, w, name in zip(out, want, ("pooled", "edge_max")):
        assert_bits(T, got, w, name)


row("sslam_edge_pool", {"s544x2": edge_pool_case, "s512x1": lambda f: edge_pool_case(f, 512, 1)})


def frame_stats_case(f, width=128, G=5, K=37, n=2):
    import synth
    T, hip = f.T, f.hip
    r = np.random.default_rng(G * K)
    sal = r.uniform(0, 1, (n, G, G)).astype(np.float32)
    pooled, emax = r.uniform(0, 3, (n, G, G)).astype(np.float32), r.uniform(3, 4, (n,)).astype(np.float32)
    desc = np.stack([synth.unit_descriptors(300 + fr, K, width, 0) for fr in range(n)]).astype(np.float32)
    dev = lambda x: T.from_numpy(np.ascontiguousarray(x)).cuda()
    want = _unplaced(lambda: [t.cpu().numpy() for t in hip.val_frame_stats(dev(sal), dev(pooled), dev(emax), descriptors=dev(desc))])
    b = Bufs(T)
    ins = (b.i("saliency", sal), b.i("pooled", pooled), b.i("edge_max", emax), b.i("descriptors", desc, guard=go._guard(width)))
    out = (b.o("stats", (n, hip.VAL_FRAME_STATS)), b.o("desc_mean", (n, width)), b.o("desc_m2", (n, width)))
    dp = hip._dp
    _direct(f, "val_frame_stats", "sslam_val_frame_stats_d", ins + out, *(dp(t) for t in ins), n, G, K, *(dp(t) for t in out), width)
    b.check(f"val_frame_stats width {width}")
    for got, w, name in zip(out, want, ("stats", "desc_mean", "desc_m2")):
        assert_bits(T, got, w, name)


row("sslam_val_frame_stats_d", {"w128": frame_stats_case, "w256": lambda f: frame_stats_case(f, 256)})
row("sslam_val_frame_stats", {"w128": frame_stats_case}, via=("sslam_val_frame_stats_d", _drop(-1)))


def pair_stats_case(f, listed=False, pattern=None, n1=300, n2=129, temperature=0.1):
    import val_edge_cases as vec
    T, hip = f.T, f.hip
    z = vec.pair_arrays(pattern or vec.PATTERNS[-1], n1, n2)
    dev = lambda x: T.from_numpy(np.ascontiguousarray(x)).cuda()
    want = _unplaced(lambda: [t.cpu().numpy() for t in hip.val_pair_stats(*(dev(z[k]) for k in ("sal1", "sal2", "nn12", "nn21", "s12", "ce", "s00")), temperature)])
    P, G = z["sal1"].shape[0], z["sal1"].shape[1]
    b = Bufs(T)
    arr = tuple(b.i(k, z[k]) for k in ("nn12", "nn21", "s12", "ce", "s00"))
    out = (b.o("stats", (P, hip.VAL_PAIR_STATS)), b.o("n_matches", (P,), T.int32))
    dp = hip._dp
    if listed:          # the bank holds sal1's frames, then sal2's: pair p = (p, P + p), as the strided call pairs them
        assert n1 == n2, "the listed form has n1 = n2 = K"
        bank = b.i("saliency_bank", np.concatenate([z["sal1"], z["sal2"]]))
        lists = (b.i("pair_first", np.arange(P, dtype=np.int32)), b.i("pair_second", np.arange(P, 2 * P, dtype=np.int32)))
        _direct(f, "val_pair_stats_pairs", "sslam_val_pair_stats_pairs", (bank,) + out, dp(bank), G, 2 * P, *(dp(t) for t in lists), *(dp(t) for t in arr),
                n1, P, C.c_float(temperature), *(dp(t) for t in out))
    else:
        sals = (b.i("saliency1", z["sal1"]), b.i("saliency2", z["sal2"]))
        _direct(f, "val_pair_stats", "sslam_val_pair_stats", sals + out, *(dp(t) for t in sals), G, *(dp(t) for t in arr), n1, n2, P,
                C.c_float(temperature), *(dp(t) for t in out))
    b.check(f"val_pair_stats listed {listed}")
    for got, w, name in zip(out, want, ("stats", "n_matches")):
        assert_bits(T, got, w, name)


row("sslam_val_pair_stats", {"n300x129": pair_stats_case})
row("sslam_val_pair_stats_pairs", {"k129": lambda f: pair_stats_case(f, True, n1=129, n2=129)})


# ================================================================================================================ the sweep
def test_the_table_covers_every_row_of_the_contract():
    assert set(TABLE) == set(lt.ALIGN), sorted(set(TABLE) ^ set(lt.ALIGN))


CASES = [(entry, name) for entry, r in TABLE.items() for name in r["cases"]]


@pytest.mark.parametrize("entry,name", CASES, ids=[f"{e[6:]}-{n}" for e, n in CASES])
def test_every_operand_at_its_least_alignment(T, hip, knob, monkeypatch, entry, name):
    r = TABLE[entry]
    run_placed(T, hip, monkeypatch, entry, lambda: r["cases"][name](F(T, hip, knob)), via=r["via"], also=r["also"], aligned_too=r["aligned_too"])


@pytest.mark.parametrize("entry", list(TABLE), ids=[e[6:] for e in TABLE])
def test_every_pointer_at_half_its_alignment_is_refused(T, hip, knob, monkeypatch, entry):
    r = TABLE[entry]
    run_refusals(T, hip, monkeypatch, entry, lambda: r["cases"][r["refuse"]](F(T, hip, knob)), via=r["via"], also=r["also"])


# ================================================================================================================== strides
# The descriptor entries on the cases of the guarded file, (33, 70) x 3 pairs at width 128 and (129, 65) x 17 at 256 for the form
# that needs a workspace; listed pairs over the bank of 4 frames.  `kind` names what lies between the frames:
#   pad4      dense + 4 floats                     odd      dense + 132 floats: no multiple of the row width
#   narrow    three rows more than a frame holds   zero1 / zero2   stride 0 on that side: frame 0 against every frame of the other
#   negative  -(dense + 4): the base is the LAST frame's address and pair p reads frame P - 1 - p
# Gaps hold NaN bits (gd.spread).  The oracle is the dense case's, pair by pair.
KINDS = ("pad4", "odd", "narrow", "zero1", "zero2", "negative")


def _stride(kind, rows, width, side):
    dense = rows * width
    if kind in ("zero1", "zero2"):
        return 0 if kind == f"zero{side}" else dense
    return {"pad4": dense + 4, "odd": dense + 132, "narrow": (rows + 3) * width, "negative": -(dense + 4)}[kind]


def _sim_want(c, kind, P):
    """The oracle's five arrays for the pairs the strides name."""
    if kind == "negative":
        return {k: c[k][::-1] for k in ("nn12", "s12", "nn21", "s21", "second12")}
    if kind in ("zero1", "zero2"):
        per = [go._pair_arrays(c["d1"][0 if kind == "zero1" else p], c["d2"][0 if kind == "zero2" else p]) for p in range(P)]
        return {k: np.stack([r[i] for r in per]) for i, k in enumerate(("nn12", "s12", "nn21", "s21", "second12"))}
    return c


def strided_sim_case(f, kind, entry="ws", n1=33, n2=70, width=128, form="two_pass_3"):
    """sslam_sim_argmax_ws_d (entry "ws"), sslam_sim_argmax_rows_d ("rows") or sslam_row_lse_d ("lse") with strided frames."""
    T, hip = f.T, f.hip
    variant, P = go.SIM_FORMS[form]
    if variant is not None:
        f.knob("SSLAM_M1_VARIANT", variant)
    c = go.sim_case(n1, n2, width, P)
    s1, s2 = _stride(kind, n1, width, 1), _stride(kind, n2, width, 2)
    want = _sim_want(c, kind, P)
    b, dp = Bufs(T), hip._dp
    d1, p1 = b.frames("desc1", c["d1"], s1, guard=go._guard(width))
    d2, p2 = b.frames("desc2", c["d2"], s2, guard=go._guard(width))
    head = (C.c_void_p(p1), s1, n1, C.c_void_p(p2), s2, n2, P)
    if entry == "ws":
        need = int(hip.lib().sslam_sim_argmax_workspace_bytes(n2, P))
        out = go._sim_outputs(b, T, P, n1, n2, True, True)
        ws = gd.dirty(T, need, 0xFF) if need else None
        hip._run("sim_argmax", hip.lib().sslam_sim_argmax_ws_d, (d1, d2, out[0]), *head, *(dp(t) for t in out), dp(ws), need, width)
        b.check(f"sim_argmax strides {kind}")
        go._check_sim(T, out, want)
    elif entry == "rows":
        out = (b.o("nn12", (P, n1), T.int32), b.o("s12", (P, n1)), b.o("second12", (P, n1)))
        hip._run("sim_argmax_rows", hip.lib().sslam_sim_argmax_rows_d, (d1, d2, out[0]), *head, *(dp(t) for t in out), width)
        b.check(f"sim_argmax_rows strides {kind}")
        go._check_sim(T, out, want, ("nn12", "s12", "second12"))
    else:          # no exact oracle: the bytes of the plain, dense call on the frames the strides name
        pick = lambda a, side: np.ascontiguousarray(a[::-1] if kind == "negative" else np.repeat(a[:1], P, 0) if kind == f"zero{side}" else a)
        nn12, s12, nn21, lse, ce, s00 = _plain_pair(f, pick(c["d1"], 1), pick(c["d2"], 2))
        assert np.array_equal(go._bytes(s12), go._bytes(np.ascontiguousarray(want["s12"]))), "the plain row maxima are the oracle's"
        out = (b.o("lse", (P, n1)), b.o("ce", (P, n1)), b.o("s00", (P,)))
        hip._run("row_lse", hip.lib().sslam_row_lse_d, (d1, d2, out[0]), *head, dp(b.i("s12", s12)), C.c_float(0.1), *(dp(t) for t in out), width)
        b.check(f"row_lse strides {kind}")
        for got, w, name in zip(out, (lse, ce, s00), ("lse", "ce", "s00")):
            assert_bits(T, got, w, name)


def strided_listed_case(f, kind, entry="ws", K=33, width=128, form="two_pass_3"):
    """The listed-pair siblings with a frame_stride above K * d (pad4, odd, narrow) or below 0 (the bank's address is its LAST
    frame's and frame i lies i strides before it: the lists are read as they stand)."""
    T, hip = f.T, f.hip
    variant, P = go.SIM_FORMS[form]
    if variant is not None:
        f.knob("SSLAM_M1_VARIANT", variant)
    c = go.bank_case(K, width, P)
    fs = _stride(kind, K, width, 0)
    bank_np = c["bank"][::-1] if kind == "negative" else c["bank"]          # stored backwards, so that frame i is frame i of the case
    b, dp = Bufs(T), hip._dp
    bank, p0 = b.frames("bank", np.ascontiguousarray(bank_np), abs(fs), guard=go._guard(width))
    if kind == "negative":
        p0 += 4 * abs(fs) * 3
    first, second = b.i("pair_first", c["first"]), b.i("pair_second", c["second"])
    head = (C.c_void_p(p0), fs, 4, K, dp(first), dp(second), P)
    if entry == "ws":
        need = int(hip.lib().sslam_sim_argmax_workspace_bytes(K, P))
        out = go._sim_outputs(b, T, P, K, K, True, True)
        ws = gd.dirty(T, need, 0xFF) if need else None
        hip._run("sim_argmax_pairs", hip.lib().sslam_sim_argmax_pairs_d, (bank, out[0]), *head, *(dp(t) for t in out), dp(ws), need, width)
        b.check(f"sim_argmax_pairs frame_stride {kind}")
        go._check_sim(T, out, c)
    elif entry == "rows":
        out = (b.o("nn12", (P, K), T.int32), b.o("s12", (P, K)), b.o("second12", (P, K)))
        hip._run("sim_argmax_rows_pairs", hip.lib().sslam_sim_argmax_rows_pairs_d, (bank, out[0]), *head, *(dp(t) for t in out), width)
        b.check(f"sim_argmax_rows_pairs frame_stride {kind}")
        go._check_sim(T, out, c, ("nn12", "s12", "second12"))
    else:
        ok = [p for p, present in enumerate(c["present"]) if present]
        a, s = (np.ascontiguousarray(c["bank"][c[k][ok]]) for k in ("first", "second"))
        nn12, s12, nn21, lse, ce, s00 = _plain_pair(f, a, s)
        full = lambda x: np.stack([x[ok.index(p)] if p in ok else np.zeros_like(x[0]) for p in range(P)])
        assert np.array_equal(go._bytes(full(s12)), go._bytes(np.ascontiguousarray(c["s12"])))
        out = (b.o("lse", (P, K)), b.o("ce", (P, K)), b.o("s00", (P,)))
        hip._run("row_lse_pairs", hip.lib().sslam_row_lse_pairs_d, (bank, out[0]), *head, dp(b.i("s12", full(s12))), C.c_float(0.1), *(dp(t) for t in out), width)
        b.check(f"row_lse_pairs frame_stride {kind}")
        for got, w, name in zip(out, (lse, ce, s00), ("lse", "ce", "s00")):
            assert_bits(T, got, full(w), name)


def strided_finalize_case(f, kind, listed=False, n1=33, n2=70, P=3):
    """sslam_match_finalize[_pairs] with its score (and intensity) arrays strided: any count of floats is accepted, so pad4 is
    dense + 4, odd is dense + 1, narrow dense + 37; 0 on each side; negative.  The arg-max arrays are dense, as the entry has them."""
    T, hip = f.T, f.hip
    off = {"pad4": 4, "odd": 1, "narrow": 37, "negative": 5}
    if listed:
        K = n1
        c = go.bank_case(K, 128, P)
        st = (-1 if kind == "negative" else 1) * (K + off[kind])
        rev = (lambda x: np.ascontiguousarray(x[::-1])) if kind == "negative" else np.ascontiguousarray
        per = []
        for a, s, ok in zip(c["first"], c["second"], c["present"]):
            kw, thr = go._m1_kw(_RUN, c["intensity"][a % 4], c["intensity"][s % 4])
            per.append(go._full(K, *go.ora.match_with_quality(c["bank"][a], c["bank"][s], c["scores"][a], c["scores"][s], **kw)) if ok
                       else go._full(K, np.zeros((0, 2), np.int64), np.zeros(0, np.float32)))
        b, dp = Bufs(T), hip._dp
        sc, ps = b.frames("scores_bank", rev(c["scores"]), abs(st), guard=gd.GUARD)
        it, pi = b.frames("intensity_bank", rev(c["intensity"]), abs(st), guard=gd.GUARD)
        if kind == "negative":
            ps, pi = ps + 4 * abs(st) * 3, pi + 4 * abs(st) * 3
        ins = (b.i("nn12", c["nn12"]), b.i("s12", c["s12"]), b.i("nn21", c["nn21"]))
        lists = (b.i("pair_first", c["first"]), b.i("pair_second", c["second"]))
        out = go._finalize_out(b, T, P, K)
        hip._run("match_finalize_pairs", hip.lib().sslam_match_finalize_pairs, ins + out, *(dp(t) for t in ins), K, 4, *(dp(t) for t in lists), P,
                 C.c_void_p(ps), st, C.c_void_p(pi), *(C.c_float(v) for v in thr), *(dp(t) for t in out))
        b.check(f"match_finalize_pairs score_stride {kind}")
        go._check_finalize(T, out, go._stack(per), f"match_finalize_pairs score_stride {kind}")
        return
    c = go.sim_case(n1, n2, 128, P)
    frame = lambda side, p: 0 if kind == f"zero{side}" else P - 1 - p if kind == "negative" else p
    stride = lambda side, n: 0 if kind == f"zero{side}" else n if kind.startswith("zero") else (-1 if kind == "negative" else 1) * (n + off[kind])
    s1, s2 = stride(1, n1), stride(2, n2)
    per = []
    for p in range(P):          # the arg-max arrays are pair p's; the scores and intensities those of the frames the strides name
        a, s = frame(1, p), frame(2, p)
        kw, thr = go._m1_kw(_RUN, c["i1"][a], c["i2"][s])
        per.append(go._full(n1, *go.ora.match_with_quality(c["d1"][p], c["d2"][p], c["s1"][a], c["s2"][s], **kw)))
    b, dp = Bufs(T), hip._dp
    placed = [b.frames(name, c[key], st, guard=gd.GUARD) for name, key, st in (("scores1", "s1", s1), ("scores2", "s2", s2),
                                                                                  ("intensity1", "i1", s1), ("intensity2", "i2", s2))]
    ins = (b.i("nn12", c["nn12"]), b.i("s12", c["s12"]), b.i("nn21", c["nn21"]))
    out = go._finalize_out(b, T, P, n1)
    ptr = [C.c_void_p(p) for _, p in placed]
    hip._run("match_finalize", hip.lib().sslam_match_finalize, ins + out, *(dp(t) for t in ins), n1, n2, P, ptr[0], s1, ptr[1], s2, ptr[2], ptr[3],
             *(C.c_float(v) for v in thr), *(dp(t) for t in out))
    b.check(f"match_finalize sstride {kind}")
    go._check_finalize(T, out, go._stack(per), f"match_finalize sstride {kind}")


_WS_FORM = dict(n1=129, n2=65, width=256, form="default_17")          # the one-pass form: a workspace, 17 pairs, two query blocks
STRIDED = {}
for _kind in KINDS:
    for _e, _sym in (("ws", "sslam_sim_argmax_ws_d"), ("rows", "sslam_sim_argmax_rows_d"), ("lse", "sslam_row_lse_d")):
        STRIDED[_sym, _kind] = lambda f, k=_kind, e=_e: strided_sim_case(f, k, e)
    STRIDED["sslam_match_finalize", _kind] = lambda f, k=_kind: strided_finalize_case(f, k)
    if not _kind.startswith("zero"):
        for _e, _sym in (("ws", "sslam_sim_argmax_pairs_d"), ("rows", "sslam_sim_argmax_rows_pairs_d"), ("lse", "sslam_row_lse_pairs_d")):
            STRIDED[_sym, _kind] = lambda f, k=_kind, e=_e: strided_listed_case(f, k, e)
        STRIDED["sslam_match_finalize_pairs", _kind] = lambda f, k=_kind: strided_finalize_case(f, k, listed=True)
for _kind in ("pad4", "odd", "negative"):
    STRIDED["sslam_sim_argmax_ws_d", _kind + "_one_pass_w256"] = lambda f, k=_kind: strided_sim_case(f, k, "ws", **_WS_FORM)
    STRIDED["sslam_sim_argmax_pairs_d", _kind + "_one_pass_w256"] = lambda f, k=_kind: strided_listed_case(f, k, "ws", K=129, width=256, form="default_17")
# the siblings without a width, a workspace or both: the same calls with those arguments dropped
for (_sym, _kind), _case in list(STRIDED.items()):
    if _kind == "odd":
        for _sib in [e for e, r in TABLE.items() if r["via"] and r["via"][0] == _sym and e in lt.STRIDES]:
            STRIDED[_sib, _kind] = _case
STRIDED_IDS = list(STRIDED)


@pytest.mark.parametrize("entry,kind", STRIDED_IDS, ids=[f"{e[6:]}-{k}" for e, k in STRIDED_IDS])
def test_every_stride_the_header_names(T, hip, knob, monkeypatch, entry, kind):
    """Strided operands, each still at its least alignment: just past and just before a 256-byte boundary."""
    r = TABLE[entry]
    run_placed(T, hip, monkeypatch, entry, lambda: STRIDED[entry, kind](F(T, hip, knob)), via=r["via"])


def test_every_entry_with_a_stride_has_strided_rows():
    for entry, names in lt.STRIDES.items():
        kinds = {k for e, k in STRIDED if e == entry}
        assert "odd" in kinds, entry
        if not TABLE[entry]["via"]:
            want = set(KINDS) - ({"zero1", "zero2"} if "frame_stride" in names or "score_stride" in names else set())
            assert want <= kinds, (entry, sorted(want - kinds))


@pytest.mark.parametrize("entry", [e for e in lt.STRIDES if any(s in lt.DESCRIPTOR_STRIDES for s in lt.STRIDES[e]) and not TABLE[e]["via"]])
def test_a_descriptor_stride_that_is_no_multiple_of_four_floats_is_refused(T, hip, knob, monkeypatch, entry):
    """stride1 / stride2 / frame_stride of dense + 2 and of -2 floats: SSLAM_E_INVALID, nothing launched, nothing written."""
    seen = []

    def bad_strides(what, fn, tensors, *args):
        if fn.__name__ != entry or gd.placement is None:
            return orig(what, fn, tensors, *args)
        n0 = hip.launch_count()
        at = [{"stride1": 1, "stride2": 4, "frame_stride": 1}[s] for s in lt.STRIDES[entry]]          # where the prototype has them
        assert all(isinstance(args[i], int) and args[i] > 0 for i in at), (entry, at)
        for i in at:
            for v in (args[i] + 2, -2):
                bad = args[:i] + (v,) + args[i + 1:]
                with T.cuda.device(0):
                    assert fn(*bad, C.c_void_p(T.cuda.current_stream().cuda_stream)) == hip.E_INVALID, (entry, i, v)
                seen.append((i, v))
        T.cuda.synchronize()
        assert hip.launch_count() == n0
        for r in gd.placement.made:
            if r["kind"] == "out":
                idt, sentinel = gd._int_view(T, r["middle"].dtype)
                assert bool((r["middle"].reshape(-1).view(idt) == sentinel).all()), f"{entry}: a refused call wrote {r['name']}"
        raise _Refused()

    orig = hip._run
    monkeypatch.setattr(hip, "_run", bad_strides)
    with gd.placed(gd.Placement(_aligns(entry), "aligned")):
        with pytest.raises(_Refused):
            TABLE[entry]["cases"][TABLE[entry]["refuse"]](F(T, hip, knob))
    monkeypatch.setattr(hip, "_run", orig)
    assert len(seen) == 2 * len(lt.STRIDES[entry])
