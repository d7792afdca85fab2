"""Online loop closures without a GPU: the interface of libsslam_place.so - include/sslam_place.h,
sslam_amd.lib.PLACE_EXPORTS and tests/place_table.py hold the same entries; the built library's symbols are tests/test_libraries_cpu.py -, one past each size limit and every
invalid operand refused before a launch, the host-side checks of every layer, the restatement (tests/place_ref.py) held to the
batch entries' restatement (tests/loop_ref.py) row by row, the numpy drop-ins held to the restatement, the edge log's contract
rows, and the planted study DESIGN.md §4n records."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import loop_cases as lc
import loop_ref
import place_cases as pcs
import place_ref as ref
import place_table as pt
import pose_graph_cases as pc
import pose_graph_ref as pg
import window_cases as wc
import window_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sslam_place.h")
PLACE, LOG = "sslp_place_step", "sslp_edge_log_step"


# ---------------------------------------------------------------------------------------------------------------- the interface
def _header(name="sslam_place.h"):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_symbols_exports_and_table_agree():
    """The table, the constants and the key lists against the export list; that list against the header and the built library is
    tests/test_libraries_cpu.py."""
    from sslam_amd import lib
    declared = lib.PLACE_EXPORTS
    assert set(pt.ALIGN) | set(pt.HOST_ONLY) == set(declared) and not set(pt.ALIGN) & set(pt.HOST_ONLY) and set(pt.LIMITS) == set(pt.ALIGN)
    consts = {k: int(v) for k, v in re.findall(r"#define (SSLP_\w+) (\d+)", open(HEADER).read())}
    assert consts == dict(SSLP_MAX_CAPACITY=pt.MAX_CAPACITY, SSLP_MAX_K=pt.MAX_K, SSLP_MAX_PER_FRAME=pt.MAX_PER_FRAME, SSLP_MAX_SLOTS=pt.MAX_SLOTS,
                          SSLP_FRAMES_PER_GROUP=pt.FRAMES_PER_GROUP)
    assert (lib.PLACE_MAX_CAPACITY, lib.PLACE_MAX_K, lib.PLACE_MAX_PER_FRAME, lib.PLACE_MAX_SLOTS) == \
        (pt.MAX_CAPACITY, pt.MAX_K, pt.MAX_PER_FRAME, pt.MAX_SLOTS) == (ref.MAX_CAPACITY, ref.MAX_K, ref.MAX_PER_FRAME, ref.MAX_SLOTS)
    assert (pt.MAX_CAPACITY, pt.MAX_K, pt.MAX_PER_FRAME, pt.FRAMES_PER_GROUP) == \
        (loop_ref.MAX_FRAMES, loop_ref.MAX_K, loop_ref.MAX_PER_FRAME, loop_ref.FRAMES_PER_GROUP), "the bank's limits are the batch entries'"
    assert lib.PLACE_STATE_KEYS == ref.STATE_KEYS and lib.PLACE_OUT_KEYS == ref.OUT_KEYS
    assert lib.EDGE_LOG_STATE_KEYS == ref.LOG_STATE_KEYS and lib.EDGE_LOG_OUT_KEYS == ref.LOG_OUT_KEYS
    assert list(lib.PLACE_STATE_KEYS) == list(pt.ALIGN[PLACE])[:3] and list(lib.PLACE_OUT_KEYS) == list(pt.ALIGN[PLACE])[6:]
    assert list(lib.EDGE_LOG_STATE_KEYS) == list(pt.ALIGN[LOG])[:5] and list(lib.EDGE_LOG_OUT_KEYS) == list(pt.ALIGN[LOG])[10:]


def test_the_header_states_both_tables_line_for_line():
    elem = {"int32_t": 4, "float": 4, "double": 8, "void": 4}         # the workspace holds float32 words
    for entry in (PLACE, LOG):
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*?)\)\s*;", _header())
        args = [re.match(r"(.*?)(\w+)$", " ".join(a.split())).groups() for a in m.group(1).split(",")]
        pointers = [(t.strip(), n) for t, n in args if "*" in t and n != "stream"]
        assert [n for _, n in pointers] == list(pt.ALIGN[entry])
        for t, n in pointers:
            assert pt.ALIGN[entry][n] == elem[t.replace("const", "").replace("*", "").strip()], n
    raw = open(HEADER).read()
    for title, lines in (("ALIGNMENT, every entry", pt.header_lines()), ("SIZE LIMITS: the expressions", pt.limit_lines())):
        start = raw.index(title)
        stated = re.sub(r"\n \*\s+", " ", raw[start:raw.index("*/", start)]).strip()
        for line in lines:
            assert line + " " in stated + " ", f"include/sslam_place.h does not state: {line}"
        assert len(re.findall(r"\bsslp_\w+: ", stated)) == 2
    for text in ("sum[c] = (t == 0 ? +0.0f : sum[c]) + raw[t][c]", "mean[c] = sum[c] / (float)(t + 1)", "fmaxf(sqrtf(ss_j), 1e-12f)",
                 "acc = fmaf(sig_t[c], sig_j[c], acc)", "status = 4", "STATE IS UNTOUCHED", "0 <= slot_first[e] < t", "new_status[e] != 3",
                 "Row t * E + e", "logged[e] equals sslw_window_step's admitted[e]", "Every refusal comes before anything is launched and writes nothing"):
        assert text in raw, text
    assert 4 * (pt.FRAMES_PER_GROUP * 257 + 256 + 4) <= 64 * 1024 and 4 * pt.MAX_CAPACITY + 64 <= 64 * 1024, "both kernels' static LDS fits 64 KB"
    assert (pt.MAX_CAPACITY - 1) * 256 + 255 < 2 ** 31 and (pt.MAX_K - 1) * 256 + 255 < 2 ** 31, "frame * d and keypoint * d fit 31 bits"


# ------------------------------------------------------------------------------------------------------------ the size limits
P = [0x10000 * (i + 1) for i in range(12)]       # never dereferenced: every call below is refused before the launch


def _place(L, capacity=100, k=5, d=128, min_gap=30, min_sim=0.3, per_frame=2, suppress=5, ptr=None):
    p = list(P) if ptr is None else ptr
    return L.sslp_place_step(*p[:5], capacity, k, d, min_gap, C.c_float(min_sim), per_frame, suppress, *p[5:], None)


def _log(L, n_slots=4, n_odometry=2, min_inliers=12, loop_min_inliers=12, capacity=100, ptr=None):
    p = list(P) if ptr is None else ptr
    return L.sslp_edge_log_step(*p[:10], n_slots, n_odometry, min_inliers, loop_min_inliers, capacity, *p[10:], None)


def test_one_past_each_size_limit_and_every_invalid_operand_is_refused_with_nothing_launched():
    from sslam_amd import lib
    L = lib.place()
    before = L.sslp_launch_count()
    for call, entry in ((_place, PLACE), (_log, LOG)):
        for name, largest in pt.LIMITS[entry]["largest"].items():
            assert call(L, **{name: largest + 1}) == pt.E_UNSUPPORTED, name
    assert _place(L, d=64) == _place(L, d=192) == _place(L, d=512) == pt.E_UNSUPPORTED
    assert _log(L, n_slots=16, n_odometry=0, capacity=pt.MAX_LOG_CAPACITY // 16 + 1) == pt.E_UNSUPPORTED, "the capacity limit divides by n_slots"
    for kw in (dict(capacity=0), dict(capacity=-1), dict(k=0), dict(d=0), dict(d=-128), dict(min_gap=0), dict(min_gap=-3), dict(per_frame=0),
               dict(suppress=-1), dict(min_sim=float("nan")), dict(min_sim=float("inf")), dict(min_sim=float("-inf"))):
        assert _place(L, **kw) == pt.E_INVALID, kw
    for kw in (dict(n_slots=0), dict(n_slots=-1), dict(n_odometry=-1), dict(n_odometry=5), dict(min_inliers=-1), dict(loop_min_inliers=-1),
               dict(capacity=0), dict(capacity=-5)):
        assert _log(L, **kw) == pt.E_INVALID, kw
    for cap in (0, -1, pt.MAX_CAPACITY + 1):
        assert L.sslp_place_workspace_bytes(cap) == 0, cap
    past = {PLACE: dict(capacity=pt.MAX_CAPACITY + 1), LOG: dict(n_slots=pt.MAX_SLOTS + 1)}
    for call, entry in ((_place, PLACE), (_log, LOG)):
        for k, (name, align) in enumerate(pt.ALIGN[entry].items()):        # a NULL, and a pointer that misses its alignment
            p = list(P)
            p[k] = None
            assert call(L, ptr=p) == pt.E_INVALID, name
            p[k] = P[k] + align // 2
            assert call(L, ptr=p) == pt.E_INVALID, name
            p[k] = P[k] + align
            assert call(L, ptr=p, **past[entry]) == pt.E_UNSUPPORTED, name     # at its alignment: judged by size
    assert L.sslp_launch_count() == before, "a refused call launches nothing"
    for cap in (1, 3, 1024, pt.MAX_CAPACITY):
        assert L.sslp_place_workspace_bytes(cap) == pt.workspace_bytes(cap) == lib.place_workspace_bytes(cap), cap


def test_every_wrapper_check_comes_before_the_library_is_loaded(monkeypatch):
    import torch
    from sslam_amd import lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were judged")
    monkeypatch.setattr(lib, "place", boom)
    f32, f64, i32 = dict(dtype=torch.float32), dict(dtype=torch.float64), dict(dtype=torch.int32)
    state = lib.alloc_place_state(10, 128, device="cpu")
    assert int(state["t"]) == 0 and {k: (tuple(v.shape), v.dtype) for k, v in state.items()} == lib.place_state_shapes(10, 128)
    out = lib.alloc_place_out(2, 128, device="cpu")
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == lib.place_out_shapes(2, 128) and tuple(out) == lib.PLACE_OUT_KEYS
    assert (out["first"] == -1).all() and (out["second"] == -1).all()
    ok = dict(state=state, descriptors=torch.zeros((5, 128), **f32), scores=torch.zeros(5, **f32))
    bad = [dict(state={k: v for k, v in state.items() if k != "t"}), dict(state=dict(state, raw=state["raw"].double())),
           dict(state=dict(state, sum=state["sum"][:64])), dict(state=dict(state, t=torch.zeros(2, **i32))), dict(state=None),
           dict(descriptors=torch.zeros((5, 256), **f32)), dict(descriptors=torch.zeros((5, 128), **f64)), dict(descriptors=torch.zeros((2, 5, 128), **f32)),
           dict(descriptors=np.zeros((5, 128), np.float32)), dict(scores=torch.zeros(4, **f32)), dict(scores=torch.zeros(5, **f64)), dict(min_gap=0),
           dict(min_gap=1.5), dict(min_sim=float("nan")), dict(per_frame=0), dict(per_frame=9), dict(suppress=-1), dict(out=dict(out, extra=out["sim"])),
           dict(out=dict(out, sig=out["sig"][:64])), dict(out=dict(out, status=out["status"].long())), dict(workspace=torch.zeros(39, dtype=torch.uint8))]
    for change in bad:
        with pytest.raises(ValueError):
            lib.place_step(**dict(ok, **change))
    with pytest.raises(ValueError, match="CUDA"):                    # well-formed host tensors: refused, still nothing loaded
        lib.place_step(**ok)
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.place_step(**dict(ok, descriptors=torch.zeros((4097, 128), **f32), scores=torch.zeros(4097, **f32)))
    for args in ((0,), (-1,), (True,), (4.0,), (10, 64), (10, 192)):
        with pytest.raises(ValueError):
            lib.alloc_place_state(*args, device="cpu")
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.alloc_place_state(4097, device="cpu")
    for args in ((0,), (9,), (2, 100)):
        with pytest.raises(ValueError):
            lib.alloc_place_out(*args, device="cpu")

    E = 4
    log = lib.alloc_edge_log(10, E, device="cpu")
    assert int(log["t"]) == 0 and (log["log_first"] == -1).all() and {k: (tuple(v.shape), v.dtype) for k, v in log.items()} == lib.edge_log_shapes(10, E)
    lo = {k: torch.zeros(shape, dtype=dt) for k, (shape, dt) in lib.edge_log_out_shapes(E).items()}
    ok = dict(state=log, slot_first=torch.zeros(E, **i32), new_T=torch.zeros((E, 12), **f64), new_info=torch.zeros((E, 21), **f64),
              new_status=torch.zeros(E, **i32), new_inliers=torch.zeros(E, **i32), n_odometry=2)
    bad = [dict(state={k: v for k, v in log.items() if k != "log_T"}), dict(state=dict(log, log_T=log["log_T"].float())),
           dict(state=dict(log, log_second=log["log_second"][:36])), dict(state=dict(log, log_first=log["log_first"][:39], log_second=log["log_second"][:39])),
           dict(slot_first=torch.zeros(E, dtype=torch.int64)), dict(slot_first=[0] * E), dict(new_T=torch.zeros((E, 11), **f64)),
           dict(new_T=torch.zeros((E, 12), **f32)), dict(new_info=torch.zeros((E - 1, 21), **f64)), dict(new_status=torch.zeros(E + 1, **i32)),
           dict(new_inliers=torch.zeros(E, dtype=torch.int64)), dict(n_odometry=-1), dict(n_odometry=E + 1), dict(n_odometry=1.0),
           dict(min_inliers=-1), dict(loop_min_inliers=-1), dict(loop_min_inliers=2.5), dict(out=dict(lo, extra=lo["status"])),
           dict(out=dict(lo, logged=lo["logged"][:3]))]
    for change in bad:
        with pytest.raises(ValueError):
            lib.edge_log_step(**dict(ok, **change))
    with pytest.raises(ValueError, match="CUDA"):
        lib.edge_log_step(**ok)
    for args in ((0, 4), (10, 0), (True, 4), (10, 4.0)):
        with pytest.raises(ValueError):
            lib.alloc_edge_log(*args, device="cpu")
    for args in ((10, 17), (pt.MAX_LOG_CAPACITY // 4 + 1, 4)):
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.check_edge_log_sizes(*args)


# ------------------------------------------------------------------------------------------------------------ the restatement
def batch_row(raw, t, c, full=False):
    """Row t of loop_ref.candidates over loop_ref.finish_signatures of the raw sums of the frames 0 .. t, and that row's signature.
    full: loop_ref.candidates forms the whole similarity matrix itself; otherwise it is handed one whose row t alone is filled -
    by loop_ref's own chain -, the only row of it that the rows asked for here read."""
    sig = loop_ref.finish_signatures(raw[:t + 1])
    S = None
    if not full:
        S = np.zeros((t + 1, t + 1), np.float32)
        for col in range(sig.shape[1]):
            S[t] = loop_ref.fmaf32(sig[t, col], sig[:, col], S[t])
    r = loop_ref.candidates(sig, c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"], S=S)
    per = c["per_frame"]
    return dict(first=r["first"][t * per:(t + 1) * per], second=r["second"][t * per:(t + 1) * per], sim=r["sim"][t * per:(t + 1) * per],
                count=r["count"][t:t + 1], sig=sig[t])


FULL_ROWS = {"frames_300_copies": (255, 256, 257, 299), "frames_70_d_256": (0, 31, 32, 33, 64, 65, 69)}


@pytest.mark.parametrize("name", pcs.BANK_NAMES)
def test_step_t_of_the_restatement_is_row_t_of_the_batch_entries_on_the_prefix(name):
    """The contract sentence of the header, on the restatements: for EVERY t of every case, first / second / sim / count of step t
    are row t of loop_ref.candidates over loop_ref.finish_signatures of the frames 0 .. t, and sig is that row's signature - the
    running sum holds the bits of the batch mean's sum.  The raw sums equal loop_ref.raw_signatures' too."""
    c = pcs.bank(name)
    outs, state = pcs.bank_expected(name)
    n = min(len(c["desc"]), c["capacity"])
    raw = loop_ref.raw_signatures(c["desc"][:n], c["scores"][:n])
    assert state["raw"][:n].tobytes() == raw.tobytes() and int(state["t"]) == n
    small = n <= 14
    for t in range(n):
        for full in {small or t in FULL_ROWS.get(name, ()), False}:
            want = batch_row(raw, t, c, full)
            for k in want:
                assert outs[t][k].dtype == want[k].dtype and outs[t][k].tobytes() == want[k].tobytes(), (name, t, k, full)
        assert outs[t]["status"][0] == 0
    for o in outs[n:]:                                               # the bank is full
        assert o["status"][0] == 4 and (o["first"] == -1).all() and (o["second"] == -1).all() and o["count"][0] == 0
        assert o["sim"].tobytes() == np.zeros(c["per_frame"], np.float32).tobytes() and o["sig"].tobytes() == np.zeros(c["desc"].shape[2], np.float32).tobytes()


def test_contract_rows_of_the_place_bank():
    """The plantings do what they were planted for - checked on the restatement the device is held to."""
    outs, state = pcs.bank_expected("capacity_3_k_1")
    assert [int(o["status"][0]) for o in outs] == [0, 0, 0, 4, 4] and int(state["t"]) == 3
    assert [int(o["count"][0]) for o in outs] == [0, 1, 1, 0, 0] and outs[1]["first"][0] == 0 and outs[2]["second"][0] == 2
    assert outs[0]["sig"].tobytes() == np.zeros(128, np.float32).tobytes(), "one frame: the centred sum is zero"
    st = ref.fresh_state(3, 128)
    c = pcs.bank("capacity_3_k_1")
    for t in (-1, 3, 2 ** 31 - 1):
        st["t"][...] = np.int32(t)
        before = {k: v.copy() for k, v in st.items()}
        assert ref.step(st, c["desc"][0], c["scores"][0], 1, -2.0, 1, 0)["status"][0] == 4
        assert all(before[k].tobytes() == st[k].tobytes() for k in st)
    c, (outs, _) = pcs.bank("frames_70_d_256"), pcs.bank_expected("frames_70_d_256")
    lo, hi = c["twins"]
    seen = 0
    for t in range(hi + c["min_gap"], 70):
        f = outs[t]["first"].tolist()
        assert (lo in f) == (hi in f)
        if lo in f:
            assert f.index(hi) == f.index(lo) + 1 and outs[t]["sim"][f.index(lo)].tobytes() == outs[t]["sim"][f.index(hi)].tobytes()
            seen += 1
    assert seen >= 5, "equal similarities, the lower j first"
    assert max(int(o["count"][0]) for o in outs) == 8 and min(int(o["count"][0]) for o in outs[40:]) >= 3
    c, (outs, _) = pcs.bank("frames_300_copies"), pcs.bank_expected("frames_300_copies")
    start, back = c["copies"]
    for t in range(start, 300):
        assert outs[t]["first"][0] == t - back and outs[t]["second"][0] == t and outs[t]["sim"][0] > 0.999, t
        assert outs[t]["count"][0] == 2 and abs(int(outs[t]["first"][1]) - (t - back)) > c["suppress"]
    assert sum(int(o["count"][0]) for o in outs[:start]) > 100 and all(o["count"][0] == 0 for o in outs[:30])
    c, (outs, _) = pcs.bank("nan_score_at_8"), pcs.bank_expected("nan_score_at_8")
    assert all(o["count"][0] > 0 for o in outs[3:8]) and all(o["count"][0] == 0 and (o["first"] == -1).all() and not o["sim"].any() for o in outs[8:])
    assert np.isnan(outs[8]["sig"]).all() and np.isnan(outs[13]["sig"]).all() and all(o["status"][0] == 0 for o in outs)
    outs, _ = pcs.bank_expected("frames_40_k_500")
    assert sum(int(o["count"][0]) for o in outs) >= 40


def test_contract_rows_of_the_edge_log():
    E = 4
    outs, st = pcs.log_expected("base")
    c = pcs.log("base")
    assert [o["logged"].tolist() for o in outs[:3]] == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0]] and all(o["logged"].all() for o in outs[5:])
    assert int(st["t"]) == 10 and st["log_second"].reshape(10, E).tolist() == [[t] * E for t in range(10)]
    assert st["log_first"].reshape(10, E)[7].tolist() == c["slot_first"][7].tolist() and st["log_T"][7 * E + 2].tobytes() == c["T"][7, 2].tobytes()
    assert st["log_info"][9 * E + 3].tobytes() == c["info"][9, 3].tobytes()
    for name, t, e in (("status_3", 7, 1), ("status_3_loop", 7, 3), ("nan_in_T", 6, 0), ("inf_in_info", 8, 2), ("first_is_t", 5, 2), ("first_past_t", 5, 3),
                       ("first_below_minus_1", 6, 1)):
        o, s = pcs.log_expected(name)
        assert o[t]["logged"].tolist() == [int(j != e) for j in range(E)], name
        row = t * E + e
        assert s["log_first"][row] == -1 and s["log_second"][row] == t and not s["log_T"][row].any() and not s["log_info"][row].any(), name
        assert all(a["logged"].tolist() == b["logged"].tolist() for i, (a, b) in enumerate(zip(o, outs)) if i != t), name
    o, s = pcs.log_expected("thresholds")                          # inliers 29, 30 against 30 in front of n_odometry; 49, 50 against 50 behind it
    assert all(x["logged"].tolist() == [0, 1, 0, 1] for x in o[5:]) and o[1]["logged"].tolist() == [0, 0, 0, 0] and o[2]["logged"].tolist() == [0, 1, 0, 0]
    o, s = pcs.log_expected("full_log")
    assert [int(x["status"][0]) for x in o] == [0] * 6 + [4] * 4 and all(not x["logged"].any() for x in o[6:]) and int(s["t"]) == 6
    assert all(s[k].tobytes() == st[k][:len(s[k])].tobytes() for k in ("log_first", "log_second", "log_T", "log_info"))
    for t in (-1, 10, 2 ** 31 - 1):
        s = ref.fresh_log(10, E)
        s["t"][...] = np.int32(t)
        before = {k: v.copy() for k, v in s.items()}
        r = ref.log_step(s, c["slot_first"][9], c["T"][9], c["info"][9], c["status"][9], c["inliers"][9], 2)
        assert r["status"][0] == 4 and not r["logged"].any() and all(before[k].tobytes() == s[k].tobytes() for k in s)
    o, _ = pcs.log_expected("loops_only")
    assert not any(x["logged"].any() for x in o[:4]) and all(x["logged"].all() for x in o[4:])


def test_the_odometry_slots_are_logged_as_the_window_admits_them():
    """For e < n_odometry and a spacing below the window, logged[e] equals sslw_window_step's admitted[e] - on the window's own
    contract cases, each reason an edge is refused among them."""
    for name in ("base", "status_3", "few_inliers", "nan_in_T", "inf_in_info", "lost_frame", "window_21_five_spacings"):
        c = wc.case(name)
        outs, _ = wc.expected(name)
        S = len(c["spacings"])
        log = ref.fresh_log(len(c["T"]), S)
        for t in range(len(c["T"])):
            first = np.array([t - int(s) if t >= int(s) else -1 for s in c["spacings"]], np.int32)
            r = ref.log_step(log, first, c["T"][t], c["info"][t], c["status"][t], c["inliers"][t], S, c["min_inliers"])
            assert r["logged"].tolist() == outs[t]["admitted"].tolist(), (name, t)


# ------------------------------------------------------------------------------------------------------------------ the layers
@pytest.mark.parametrize("name", pcs.BANK_NAMES)
def test_the_place_bank_drop_in_equals_the_restatement(name):
    """evaluation.PlaceBank - its own statement of the header, its own fused multiply-add, sharing no code with the tests'
    restatement - gives that restatement's bits at every step of every case, state included."""
    import evaluation as dropin
    c = pcs.bank(name)
    want, state = pcs.bank_expected(name)
    b = dropin.PlaceBank(c["capacity"], c["desc"].shape[2], c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"])
    for i in range(len(c["desc"])):
        got = b.step(c["desc"][i], c["scores"][i])
        assert tuple(got) == ref.OUT_KEYS
        for k in ref.OUT_KEYS:
            assert got[k].dtype == want[i][k].dtype and got[k].shape == want[i][k].shape and got[k].tobytes() == want[i][k].tobytes(), (name, i, k)
    assert all(b.state[k].tobytes() == state[k].tobytes() for k in ref.STATE_KEYS)
    b.reset()
    assert int(b.state["t"]) == 0


def test_the_drop_in_fma_is_the_restatements_on_hard_operands():
    """Both make fmaf from float64 arithmetic, by different routes (round to odd; a two-sum and the half-way case): equal on operands
    built to land on and beside the half-way points of float32."""
    from sslam_amd import place_numpy as pn
    rng = np.random.default_rng(11)
    a, b = rng.standard_normal(200000).astype(np.float32), rng.standard_normal(200000).astype(np.float32)
    c = rng.standard_normal(200000).astype(np.float32) * np.float32(2.0) ** rng.integers(-30, 30, 200000).astype(np.float32)
    one, h = np.float32(1.0), np.float32(2.0 ** -12)
    a = np.concatenate([a, np.full(4, one + h)])                       # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: half an ulp above a float32
    b = np.concatenate([b, np.full(4, one + h)])
    c = np.concatenate([c, np.array([0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -24], np.float32)])
    with np.errstate(all="ignore"):
        assert pn._fma32(a, b, c).tobytes() == loop_ref.fmaf32(a, b, c).tobytes()
    tail = pn._fma32(a[-4:], b[-4:], c[-4:])
    assert tail[1] > tail[2] and tail[0] in (tail[1], tail[2]), "a term of 2^-60 decides the half-way case either way"


@pytest.mark.parametrize("name", pcs.LOG_NAMES)
def test_the_edge_log_drop_in_equals_the_restatement(name):
    import evaluation as dropin
    c = pcs.log(name)
    want, state = pcs.log_expected(name)
    E = c["slot_first"].shape[1]
    log = dropin.EdgeLog(c["capacity"], E, c["n_odometry"], c["min_inliers"], c["loop_min_inliers"])
    for t in range(len(c["T"])):
        got = log.step(c["slot_first"][t], c["T"][t].reshape(E, 3, 4), np.stack([pg.full_info(h) for h in c["info"][t]]), c["status"][t], c["inliers"][t])
        assert tuple(got) == ref.LOG_OUT_KEYS
        for k in ref.LOG_OUT_KEYS:
            assert got[k].dtype == want[t][k].dtype and got[k].tobytes() == want[t][k].tobytes(), (name, t, k)
    assert all(log.state[k].tobytes() == state[k].tobytes() for k in ref.LOG_STATE_KEYS)
    n = min(len(c["T"]), c["capacity"])
    assert all(a.tobytes() == state[k][:n * E].tobytes() for a, k in zip(log.edges(), ("log_first", "log_second", "log_T", "log_info")))


def test_the_layers_judge_their_arguments_first(monkeypatch):
    import torch
    import evaluation as dropin
    from sslam_amd import lib, online
    from sslam_amd.pipeline import SequencePipeline

    def boom(*a, **kw):
        raise AssertionError("something was allocated, or the library loaded, before the arguments were judged")
    for name in ("place", "window", "alloc_place_state", "alloc_place_out", "alloc_edge_log", "alloc_window_state", "alloc_window_out"):
        monkeypatch.setattr(lib, name, boom)
    ok = dict(pipe=None, height=48, width=64, depth_height=480, depth_width=640)
    for change, match in ((dict(loops=5), "loops"), (dict(loops=dict(gap=3)), "loops"), (dict(loops=dict(min_gap=0)), "min_gap"),
                          (dict(loops=dict(per_frame=9)), "per_frame"), (dict(loops=dict(min_sim=float("nan"))), "min_sim"),
                          (dict(loops=dict(min_inliers=-1)), "min_inliers"), (dict(capacity=0), "capacity"), (dict(capacity=2.0), "capacity"),
                          (dict(spacings=(1, 1)), "spacings"), (dict(window=1), "window"), (dict(huber_chi=0.0), "huber_chi")):
        with pytest.raises(ValueError, match=match):
            online.LoopWindowPoseFrameStepper(**dict(ok, **change))
    for change in (dict(capacity=4097), dict(spacings=tuple(range(1, 10))), dict(spacings=(1, 2, 3, 4, 5, 6, 7, 8), window=9, loops=dict(per_frame=8), capacity=2 ** 62)):
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            online.LoopWindowPoseFrameStepper(**dict(ok, **change))
    pipe = SequencePipeline.__new__(SequencePipeline)
    for args in ((0,), (10, 0), (10, 30, float("inf")), (10, 30, 0.3, 9), (10, 30, 0.3, 2, -1)):
        with pytest.raises(ValueError):
            pipe.alloc_place_bank(*args)
    for args in ((0, 4), (10, 0), (10, 2.0)):
        with pytest.raises(ValueError):
            pipe.alloc_edge_log(*args)
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        pipe.alloc_edge_log(10, 17)
    for state in (None, {}, {"state": {}}):
        with pytest.raises(ValueError, match="alloc_place_bank"):
            SequencePipeline.place_step(state, torch.zeros((5, 128)), torch.zeros(5))
    for log, refined in ((None, {}), ({"state": {}}, {})):
        with pytest.raises(ValueError, match="alloc_edge_log"):
            SequencePipeline.edge_log_step(log, torch.zeros(2, dtype=torch.int32), refined, 1)
    with pytest.raises(ValueError, match="refined"):
        SequencePipeline.edge_log_step({"state": {}, "out": {}}, torch.zeros(2, dtype=torch.int32), {"T": 1}, 1)
    for kw in (dict(capacity=0), dict(d=64), dict(min_gap=0), dict(per_frame=9), dict(min_sim=float("nan")), dict(suppress=-1)):
        with pytest.raises(ValueError):
            dropin.PlaceBank(**kw)
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        dropin.PlaceBank(capacity=4097)
    b = dropin.PlaceBank(4)
    for args in ((np.zeros((5, 64)), np.zeros(5)), (np.zeros((5, 128)), np.zeros(4)), (np.zeros(128), np.zeros(1))):
        with pytest.raises(ValueError):
            b.step(*args)
    for kw in (dict(capacity=0), dict(n_slots=0), dict(n_odometry=8), dict(n_odometry=-1), dict(min_inliers=-1), dict(loop_min_inliers=1.5)):
        with pytest.raises(ValueError):
            dropin.EdgeLog(**kw)
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        dropin.EdgeLog(n_slots=17, n_odometry=5)
    log = dropin.EdgeLog(4, 2, 1)
    for args in (([0, 0], np.zeros((2, 12)), np.zeros((2, 6, 6)), [0, 0], [0, 0]), ([0, 0], np.zeros((2, 4, 4)), np.zeros((2, 21)), [0, 0], [0, 0]),
                 ([0], np.zeros((2, 4, 4)), np.zeros((2, 6, 6)), [0, 0], [0, 0])):
        with pytest.raises(ValueError):
            log.step(*args)
    assert (dropin.PlaceBank().capacity, dropin.PlaceBank().per_frame, dropin.EdgeLog().n_slots) == (1024, 2, 7)


# ------------------------------------------------------------------------------------------------------------------ the study
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_planted_study_the_logged_loop_edges_pay_off_online(seed):
    """tests/loop_cases.study_case(seed): 420 frames on a circle that closes after about 370, the five spacings, 3 % gross outliers,
    noise x 3, and 30 loop edges (a, a + 370).  The frames are fed ONE BY ONE: the five spacing pairs of frame t through
    window_ref.step (window 21, two steps per frame) and, with the one loop slot of the frame - filled at the step of the edge's
    second frame, t = a + 370 -, through the edge-log restatement; the odometry slots are logged exactly as the window admits
    them.  Then loop_ref.optimize(..., 4.0, 0.0, 8, 600, 1e-3) runs over the log, IN LOG ORDER, from the window's committed
    trajectory - what LoopWindowPoseFrameStepper.close_loops does on the device - and once more with the loop slots made absent.
    Position rmse after rigid alignment, metres, measured with these restatements in log order, seeds 0 - 3:
        window's committed trajectory   0.1858  0.2722  0.2336  0.2961
        sparse graph, odometry only     0.0743  0.0407  0.0388  0.0521
        sparse graph, with the loops    0.0402  0.0339  0.0312  0.0327
    (the figures of study_case's own edge order to the four digits shown).  Asserted, as conditions and not as measured bars: in
    every seed the solve with the loop slots is below the window's trajectory and below the same solve without them."""
    c = lc.study_case(seed)
    S, n, n_odo = pc.SPACINGS, 420, c["n_odometry"]
    p = pc.planted(n, S, seed, outliers=0.03, sigma_t=0.03, sigma_r=0.012)
    assert p["T"].tobytes() == c["T"][:n_odo].tobytes()
    T, info, status, inliers = wc.frame_inputs(p, S, n, seed)
    loops = {int(b): e for e, (a, b) in enumerate(zip(c["first"][n_odo:], c["second"][n_odo:]), start=n_odo)}
    E = len(S) + 1
    win, log = window_ref.fresh_state(21, len(S), n), ref.fresh_log(n, E)
    sp = np.array(S, np.int32)
    for t in range(n):
        w = window_ref.step(win, sp, T[t], info[t], status[t], inliers[t], None, 12, 4.0, 0.0, 2)
        e = loops.get(t)
        first = np.array([t - s if t >= s else -1 for s in S] + [-1 if e is None else int(c["first"][e])], np.int32)
        Tt = np.concatenate([T[t], (window_ref.IDENTITY if e is None else c["T"][e])[None]])
        it = np.concatenate([info[t], (np.zeros(21) if e is None else c["info"][e])[None]])
        r = ref.log_step(log, first, Tt, it, np.append(status[t], 3 if e is None else 0), np.append(inliers[t], 0 if e is None else 100), len(S), 12, 12)
        assert r["logged"][:len(S)].tolist() == w["admitted"].tolist() and r["logged"][-1] == (e is not None), t
    is_loop = np.arange(n * E) % E == E - 1
    assert int(((log["log_first"] >= 0) & is_loop).sum()) == 30 and int((log["log_first"] >= 0).sum()) == n_odo + 30
    traj = win["trajectory"]
    solve = lambda first: loop_ref.optimize(first, log["log_second"], log["log_T"], log["log_info"], traj, 4.0, 0.0, 8, 600, 1e-3)
    with_loops, without = solve(log["log_first"]), solve(np.where(is_loop, -1, log["log_first"]).astype(np.int32))
    assert with_loops["status"] == 0 and without["status"] == 0 and with_loops["used_edges"] == without["used_edges"] + 30
    a_win, a_odo, a_loop = (pc.ate_rmse(x, c["truth"]) for x in (traj, without["C"], with_loops["C"]))
    print(f"online loop study, seed {seed}, log order: window {a_win:.4f} m, sparse odometry only {a_odo:.4f} m, with the 30 loop edges {a_loop:.4f} m")
    assert a_loop < a_win and a_loop < a_odo, (a_win, a_odo, a_loop)
