"""The sliding-window estimator without a GPU: the interface of libsslam_window.so - include/sslam_window.h,
sslam_amd.lib.WINDOW_EXPORTS and tests/window_table.py hold the same entries; the built library's symbols are tests/test_libraries_cpu.py -, one past each size limit and
every invalid operand refused before a launch, the host-side checks of every layer, the restatement's (tests/window_ref.py)
contract rows, and the planted study DESIGN.md §4m records."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_graph_cases as pc
import pose_graph_ref as pg
import window_cases as wc
import window_ref as ref
import window_table as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sslam_window.h")
ENTRY = "sslw_window_step"


# ---------------------------------------------------------------------------------------------------------------- the interface
def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_header_symbols_exports_and_table_agree():
    """The table, the constants and the key lists against the export list; that list against the header and the built library is
    tests/test_libraries_cpu.py."""
    from sslam_amd import lib
    declared = lib.WINDOW_EXPORTS
    assert set(wt.ALIGN) | set(wt.HOST_ONLY) == set(declared) and not set(wt.ALIGN) & set(wt.HOST_ONLY) and set(wt.LIMITS) == set(wt.ALIGN)
    consts = {k: int(v) for k, v in re.findall(r"#define (SSLW_\w+) (\d+)", open(HEADER).read())}
    assert consts == dict(SSLW_MAX_WINDOW=wt.MAX_WINDOW, SSLW_MAX_SPACINGS=wt.MAX_SPACINGS, SSLW_MAX_WINDOWS=wt.MAX_WINDOWS, SSLW_MAX_FRAME=wt.MAX_FRAME)
    assert (lib.WINDOW_MAX_WINDOW, lib.WINDOW_MAX_SPACINGS, lib.WINDOW_MAX_WINDOWS, lib.WINDOW_MAX_FRAME) == \
        (wt.MAX_WINDOW, wt.MAX_SPACINGS, wt.MAX_WINDOWS, wt.MAX_FRAME) == (ref.MAX_WINDOW, ref.MAX_SPACINGS, ref.MAX_WINDOWS, ref.MAX_FRAME)
    assert lib.WINDOW_OUT_KEYS == ref.OUT_KEYS and lib.WINDOW_STATE_KEYS == ref.STATE_KEYS and wt.MAX_ITER == lib.GRAPH_MAX_ITER == pg.MAX_ITER
    assert list(lib.WINDOW_STATE_KEYS) == list(wt.ALIGN[ENTRY])[:7] and list(lib.WINDOW_OUT_KEYS) == list(wt.ALIGN[ENTRY])[14:]


def test_the_header_states_both_tables_line_for_line():
    elem = {"int32_t": 4, "double": 8, "void": 8}
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^;{]*?)\)\s*;", _header())
    args = [re.match(r"(.*?)(\w+)$", " ".join(a.split())).groups() for a in m.group(1).split(",")]
    pointers = [(t.strip(), n) for t, n in args if "*" in t and n != "stream"]
    assert [n for _, n in pointers] == list(wt.ALIGN[ENTRY])
    for t, n in pointers:
        assert wt.ALIGN[ENTRY][n] == elem[t.replace("const", "").replace("*", "").strip()], n
    raw = open(HEADER).read()
    for title, lines in (("ALIGNMENT, every entry", wt.header_lines()), ("SIZE LIMITS: the expressions", wt.limit_lines())):
        start = raw.index(title)
        stated = re.sub(r"\n \*\s+", " ", raw[start:raw.index("*/", start)]).strip()
        for line in lines:
            assert line + " " in stated + " ", f"include/sslam_window.h does not state: {line}"
        assert len(re.findall(r"\bsslw_\w+: ", stated)) == 1
    for text in ("base = max(0, t - W + 1)", "(t mod W) * S + k", "band = W - 1", "status = 4", "new_inliers[k] >= min_inliers",
                 f"{wt.lds_bytes(32) // 1000} {wt.lds_bytes(32) % 1000} bytes at W = 32", f"{wt.lds_bytes(21) // 1000} {wt.lds_bytes(21) % 1000}"):
        assert text in raw, text
    assert wt.lds_bytes(wt.MAX_WINDOW) + 4096 <= 160 * 1024, "the triangle, g, y, delta and the static words fit a CU's LDS"


# ------------------------------------------------------------------------------------------------------------ the size limits
P = [0x10000 * (i + 1) for i in range(28)]       # never dereferenced: every call below is refused before the launch


def _call(L, n_windows=1, window=4, n_spacings=3, min_inliers=12, chi=4.0, damping=0.0, n_iter=2, capacity=100, ptr=None):
    p = list(P) if ptr is None else ptr
    return L.sslw_window_step(*p[:13], n_windows, window, n_spacings, min_inliers, C.c_double(chi), C.c_double(damping), n_iter, capacity,
                              *p[13:], None)


def test_one_past_each_size_limit_and_every_invalid_operand_is_refused_with_nothing_launched():
    from sslam_amd import lib
    L = lib.window()
    before = L.sslw_launch_count()
    for name, largest in wt.LIMITS[ENTRY]["largest"].items():
        assert _call(L, **{name: largest + 1}) == wt.E_UNSUPPORTED, name
    assert _call(L, n_windows=2, capacity=wt.MAX_CAPACITY // 2 + 1) == wt.E_UNSUPPORTED, "the capacity limit divides by n_windows"
    for shape in ((wt.MAX_WINDOWS + 1, 4, 2), (1, wt.MAX_WINDOW + 1, 2), (1, 4, wt.MAX_SPACINGS + 1), (0, 4, 2), (1, 1, 2), (1, 4, 0)):
        assert L.sslw_window_workspace_bytes(*shape) == 0, shape
    for kw in (dict(n_windows=0), dict(window=1), dict(window=0), dict(n_spacings=0), dict(min_inliers=-1), dict(chi=0.0), dict(chi=float("nan")),
               dict(chi=float("inf")), dict(damping=-1.0), dict(damping=float("nan")), dict(damping=float("inf")), dict(n_iter=-1),
               dict(n_iter=wt.MAX_ITER + 1), dict(capacity=0), dict(capacity=-5)):
        assert _call(L, **kw) == wt.E_INVALID, kw
    for k, (name, align) in enumerate(wt.ALIGN[ENTRY].items()):            # a NULL, and a pointer that misses its alignment
        p = list(P)
        p[k] = None
        if name in wt.MAY_BE_NULL:                                 # never a call that would be accepted: the pointers are not memory
            assert _call(L, ptr=p, window=wt.MAX_WINDOW + 1) == wt.E_UNSUPPORTED, "a NULL C_start is judged by size like any call"
        else:
            assert _call(L, ptr=p) == wt.E_INVALID, name
        p[k] = P[k] + align // 2
        assert _call(L, ptr=p) == wt.E_INVALID, name
        p[k] = P[k] + align
        assert _call(L, window=wt.MAX_WINDOW + 1, ptr=p) == wt.E_UNSUPPORTED, name      # at its alignment: judged by size
    assert L.sslw_launch_count() == before, "a refused call launches nothing"
    for shape in ((1, 2, 1), (3, 21, 5), (1, 32, 8), (wt.MAX_WINDOWS, wt.MAX_WINDOW, wt.MAX_SPACINGS)):
        assert L.sslw_window_workspace_bytes(*shape) == wt.workspace_bytes(*shape) == lib.window_workspace_bytes(*shape), shape
    n = 6 * (wt.MAX_WINDOW - 1)
    assert n * (n + 1) // 2 < 2 ** 31 and wt.MAX_WINDOW * wt.MAX_SPACINGS <= 256, "a row offset fits 31 bits; the slots are staged in one pass"


def test_every_wrapper_check_comes_before_the_library_is_loaded(monkeypatch):
    import torch
    from sslam_amd import lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were judged")
    monkeypatch.setattr(lib, "window", boom)
    W, S = 4, 3
    state = lib.alloc_window_state(W, S, 10, device="cpu")
    assert int(state["t"]) == 0 and (state["ring_first"] == -1).all() and {k: (tuple(v.shape), v.dtype) for k, v in state.items()} == \
        lib.window_state_shapes(1, W, S, 10)
    out = lib.alloc_window_out(W, S, device="cpu")
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == lib.window_out_shapes(1, W, S) and tuple(out) == lib.WINDOW_OUT_KEYS
    f64, i32 = dict(dtype=torch.float64), dict(dtype=torch.int32)
    ok = dict(state=state, spacings=torch.tensor([1, 2, 3], **i32), new_T=torch.zeros((S, 12), **f64), new_info=torch.zeros((S, 21), **f64),
              new_status=torch.zeros(S, **i32), new_inliers=torch.zeros(S, **i32))
    bad = [dict(state={k: v for k, v in state.items() if k != "t"}), dict(state=dict(state, ring_T=state["ring_T"].float())),
           dict(state=dict(state, ring_first=state["ring_first"][:, :5])), dict(state=dict(state, t=torch.zeros(2, **i32))),
           dict(spacings=torch.tensor([1, 2, 3])), dict(spacings=[1, 2, 3]), dict(new_T=torch.zeros((S, 11), **f64)), dict(new_T=ok["new_T"].float()),
           dict(new_info=torch.zeros((S - 1, 21), **f64)), dict(new_status=torch.zeros(S, dtype=torch.int64)), dict(new_inliers=torch.zeros(S + 1, **i32)),
           dict(C_start=torch.zeros(11, **f64)), dict(C_start=torch.zeros(12)), dict(min_inliers=-1), dict(min_inliers=1.5), dict(huber_chi=0.0),
           dict(huber_chi=float("nan")), dict(damping=-1.0), dict(damping=float("inf")), dict(iterations=-1), dict(iterations=17),
           dict(iterations=True), dict(out=dict(out, extra=out["status"])), dict(out=dict(out, status=out["status"].long())),
           dict(out=dict(out, C_window=out["C_window"][:, :3])), dict(workspace=torch.zeros(8, dtype=torch.uint8))]
    for change in bad:
        with pytest.raises(ValueError):
            lib.window_step(**dict(ok, **change))
    with pytest.raises(ValueError, match="CUDA"):                    # well-formed host tensors: refused, still nothing loaded
        lib.window_step(**ok)
    for args in ((1, 1, 10), (4, 0, 10), (4, 3, 0), (4, 3, 10, 0), (True, 3, 10), (4.0, 3, 10)):
        with pytest.raises(ValueError):
            lib.alloc_window_state(*args, device="cpu")
    for args in ((33, 3, 10), (4, 9, 10), (4, 3, 10, 65536), (4, 3, wt.MAX_CAPACITY + 1)):
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.alloc_window_state(*args, device="cpu")
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.alloc_window_out(33, 3, device="cpu")


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_contract_rows_of_the_restatement():
    """What the header promises, on the restatement the device is held to bit for bit (tests/test_gpu_window.py)."""
    outs, state = wc.expected("base")
    c = wc.case("base")
    assert outs[0]["status"] == 3 and outs[0]["n_nodes"] == 1 and outs[0]["lost"] == 0 and outs[0]["predicted_from"] == -1
    assert outs[0]["C_window"][0].tobytes() == ref.IDENTITY.tobytes() and (outs[0]["C_window"][1:] == 0).all()
    assert [int(o["base"]) for o in outs] == [0, 0, 0, 0, 1, 2, 3, 4, 5] and [int(o["n_nodes"]) for o in outs] == [1, 2, 3, 4, 4, 4, 4, 4, 4]
    assert [o["admitted"].tolist() for o in outs[:4]] == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]] and int(state["t"]) == 9
    assert all(o["predicted_from"] == 0 and o["lost"] == 0 and o["status"] == 0 for o in outs[1:])
    assert [int(o["dropped_edges"]) for o in outs] == [0, 0, 0, 0, 3, 5, 6, 6, 6], "the slots whose first frame has left: 3 + 2 + 1 once every row is full"
    assert [int(o["used_edges"]) for o in outs] == [0, 1, 3, 6, 6, 6, 6, 6, 6]
    assert state["ring_second"].reshape(4, 3).tolist() == [[8] * 3, [5] * 3, [6] * 3, [7] * 3], "frame j's pairs sit in row j mod W"
    assert state["ring_first"].reshape(4, 3).tolist() == [[7, 6, 5], [4, 3, 2], [5, 4, 3], [6, 5, 4]]
    for t, o in enumerate(outs):
        assert o["C_window"][0].tobytes() == (outs[t - 1]["C_window"][int(o["base"]) - int(outs[t - 1]["base"])].tobytes() if t else ref.IDENTITY.tobytes()), \
            "the anchor is the oldest frame at its last estimate"
    assert state["trajectory"][8].tobytes() == outs[8]["C_window"][3].tobytes() and state["trajectory"][2].tobytes() == outs[5]["C_window"][0].tobytes()
    outs_s, state_s = wc.expected("start_given")
    assert outs_s[0]["C_window"][0].tobytes() == c["truth"][3].tobytes() == state_s["trajectory"][0].tobytes()
    for name, t, k in (("status_3", 5, 0), ("few_inliers", 6, 1), ("nan_in_T", 7, 0), ("inf_in_info", 4, 2)):
        o, st = wc.expected(name)
        assert o[t]["admitted"].tolist() == [int(j != k) for j in range(3)], name
        assert o[t]["predicted_from"] == (1 if k == 0 else 0) and o[t]["used_edges"] == 5 and np.isfinite(o[t]["C_window"]).all(), name
        if t >= len(o) - 4:                                       # the slot is still in the ring at the end: zeroed, absent
            slot = (t % 4) * 3 + k
            assert st["ring_first"][slot] == -1 and st["ring_second"][slot] == t and not st["ring_T"][slot].any() and not st["ring_info"][slot].any(), name
    o, st = wc.expected("lost_frame")
    assert o[5]["lost"] == 1 and o[5]["predicted_from"] == -1 and not o[5]["admitted"].any()
    assert o[5]["C_window"][3].tobytes() == o[5]["C_window"][2].tobytes() == o[4]["C_window"][3].tobytes(), \
        "a lost frame stands where the frame before it stood"
    assert o[5]["status"] == 2 and o[5]["failed_row"] == 12, "no edge reaches the lost frame: its first pivot is zero, nothing moves"
    assert o[6]["lost"] == 0 and o[6]["status"] == 0
    o, _ = wc.expected("no_iterations")
    assert all(x["status"] == 1 and x["iterations"] == 0 and x["cost"] == x["cost_in"] for x in o[1:])
    o, _ = wc.expected("zero_info")
    assert all(x["status"] == 2 and x["failed_row"] == 0 and x["iterations"] == 0 and x["cost_in"] == 0 for x in o[1:])
    full, short = wc.expected("base"), wc.expected("short_trajectory")
    assert short[1]["trajectory"].shape == (5, 12) and short[1]["trajectory"].tobytes() == full[1]["trajectory"][:5].tobytes()
    assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(full[0], short[0]) for k in ref.OUT_KEYS)
    for t in (-1, 2 ** 31 - 1):
        st = ref.fresh_state(4, 3, 9)
        st["t"][...] = np.int32(t)
        before = {k: v.copy() for k, v in st.items()}
        assert ref.step(st, c["spacings"], c["T"][0], c["info"][0], c["status"][0], c["inliers"][0]) == dict(status=4)
        assert all(before[k].tobytes() == st[k].tobytes() for k in st)


def test_a_window_that_holds_every_frame_is_the_batch_graph():
    """While the window has not slid, a step's solve is the batch graph over the edges so far: pose_graph_ref.optimize on the global
    edge list from the same poses gives the same bits up to the order of the slots - checked through the cost, which sums the same
    terms in another order, to 1e-12 relative, and through the poses to 1e-9 (two Gauss-Newton steps from the same start)."""
    c = wc.window_case("wide", 12, (1, 2, 4), 12, 21)
    state = ref.fresh_state(12, 3, 12)
    for t in range(12):
        before = state["ring_C"].copy()
        o = ref.step(state, c["spacings"], c["T"][t], c["info"][t], c["status"][t], c["inliers"][t])
        if t == 0:
            continue
        edges = [(t2 - s, t2, k) for t2 in range(t + 1) for k, s in enumerate((1, 2, 4)) if t2 >= s]
        C_in = np.concatenate([before[:t], pg.compose(c["T"][t, 0], before[t - 1])[None]])      # the prediction: spacing 1 is admitted
        r = pg.optimize([a for a, _, _ in edges], [b for _, b, _ in edges], np.stack([c["T"][b, k] for _, b, k in edges]),
                        np.stack([c["info"][b, k] for _, b, k in edges]), C_in, 11, 4.0, 0.0, 2)
        assert r["status"] == o["status"] and r["iterations"] == o["iterations"] and r["used_edges"] == o["used_edges"]
        assert abs(r["cost"] - o["cost"]) <= 1e-12 * max(o["cost_in"], 1e-300) and np.abs(r["C"] - o["C_window"][:t + 1]).max() <= 1e-9


# ------------------------------------------------------------------------------------------------------------------ the study
def test_planted_study_the_window_beats_the_chain_in_every_seed():
    """20 planted 120-frame trajectories at the five spacings with 3 % gross outliers (tests/pose_graph_cases.py), window 21, two
    steps per frame, every pair admitted.  Position rmse after rigid alignment of the committed trajectory, measured with this
    restatement, median over the seeds: the spacing-1 chain 0.2654 m, the window 0.0319 m (the tightest seed 0.0293 m against its
    chain's 0.0871 m), the batch graph at chi = 4 0.0101 m (tests/test_pose_graph_cpu.py).  Asserted, as a condition and not a
    measured bar: the window's error is below the chain's in all 20 seeds."""
    chain, window = [], []
    for seed in range(20):
        c = wc.window_case("study", 21, wc.SPACINGS, 120, seed, outliers=0.03)
        _, state = ref.run(c)
        chain.append(pc.ate_rmse(c["C_chain"], c["truth"]))
        window.append(pc.ate_rmse(state["trajectory"], c["truth"]))
    tight = int(np.argmax(np.array(window) / np.array(chain)))
    print(f"planted study, median ate rmse over 20 seeds: chain {np.median(chain):.4f} m, window {np.median(window):.4f} m; "
          f"tightest seed {tight}: window {window[tight]:.4f} m, chain {chain[tight]:.4f} m")
    assert all(w < c for w, c in zip(window, chain)), list(zip(window, chain))


# ------------------------------------------------------------------------------------------------------------------ the layers
DROPIN_CASES = tuple(c["name"] for c in wc.shape_cases() + wc.contract_cases())      # every case the device is held to


@pytest.mark.parametrize("name", DROPIN_CASES)
def test_the_numpy_drop_in_equals_the_restatement(name):
    """evaluation.PoseWindow - its own statement of both headers, sharing no code with the tests' restatement - gives that
    restatement's bits at every step of every case: outputs, and the trajectory at the end."""
    import evaluation as dropin
    c = wc.case(name)
    want, _ = wc.expected(name)
    S = len(c["spacings"])
    start = None if c["C_start"] is None else c["C_start"].reshape(3, 4)
    w = dropin.PoseWindow(c["window"], tuple(int(s) for s in c["spacings"]), c["capacity"], c["min_inliers"], c["chi"], c["damping"], c["n_iter"], start)
    n = len(c["T"])
    state = ref.fresh_state(c["window"], S, c["capacity"])
    for i in range(n):
        got = w.step(c["T"][i].reshape(S, 3, 4), np.stack([pg.full_info(h) for h in c["info"][i]]), c["status"][i], c["inliers"][i])
        assert tuple(got) == ref.OUT_KEYS
        for k in ref.OUT_KEYS:
            assert got[k].dtype == want[i][k].dtype and got[k].shape == want[i][k].shape and got[k].tobytes() == want[i][k].tobytes(), (name, i, k)
        ref.step(state, c["spacings"], c["T"][i], c["info"][i], c["status"][i], c["inliers"][i], c["C_start"], c["min_inliers"], c["chi"], c["damping"],
                 c["n_iter"])
    m = min(n, c["capacity"])
    assert w.trajectory().shape == (m, 4, 4) and w.trajectory().tobytes() == pg.trajectory(state["trajectory"][:m]).tobytes()
    w.reset()
    assert int(w.state["t"]) == 0 and w.trajectory().shape == (0, 4, 4)


def test_the_layers_judge_their_arguments_first(monkeypatch):
    import torch
    import evaluation as dropin
    from sslam_amd import lib, online
    from sslam_amd.pipeline import SequencePipeline

    def boom(*a, **kw):
        raise AssertionError("something was allocated, or the library loaded, before the arguments were judged")
    for name in ("window", "alloc_window_state", "alloc_window_out"):
        monkeypatch.setattr(lib, name, boom)
    ok = dict(pipe=None, height=48, width=64, depth_height=480, depth_width=640)
    for change, match in ((dict(spacings=()), "spacings"), (dict(spacings=(1, 1)), "spacings"), (dict(spacings=(0, 2)), "spacings"), (dict(spacings=5), "spacings"),
                          (dict(spacings=(1, 2 ** 31), window=4), "spacings"),      # kept as int32 on the device: refused before the bank is made
                          (dict(window=1), "window"), (dict(window=2.0), "window"), (dict(threshold=-1.0), "threshold"), (dict(hypotheses=0), "hypotheses"),
                          (dict(huber=0.0), "huber"), (dict(iterations=17), "iterations"), (dict(min_inliers=-1), "min_inliers"),
                          (dict(huber_chi=float("nan")), "huber_chi"), (dict(damping=-1.0), "damping"), (dict(graph_iterations=17), "iterations"),
                          (dict(capacity=0), "capacity"), (dict(depth_height=24, depth_width=32), "camera describes")):
        with pytest.raises(ValueError, match=match):
            online.WindowPoseFrameStepper(**dict(ok, **change))
    for change in (dict(window=33), dict(spacings=tuple(range(1, 10))), dict(spacings=(1, 40))):      # window = max(spacings) + 1 = 41
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            online.WindowPoseFrameStepper(**dict(ok, **change))
    pipe = SequencePipeline.__new__(SequencePipeline)                  # alloc_pose_window reads the device alone, after the checks
    for args in ((1, (1,)), (4, ()), (4, (1, 1)), (4, (1, 2), 0), (4, (1, 2), 10, 0), (4, [1.0]), (4, (2 ** 31,))):
        with pytest.raises(ValueError):
            pipe.alloc_pose_window(*args)
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        pipe.alloc_pose_window(33, (1,))
    for state, refined in ((None, {}), ({"state": {}}, {}), (dict(state={"t": torch.zeros(1)}, out={}, spacings=torch.zeros(2), workspace=None), {"T": 1})):
        with pytest.raises(ValueError):
            SequencePipeline.pose_window_step(state, refined)
    st = dict(state={"t": torch.zeros(1, dtype=torch.int32)}, out={}, spacings=torch.zeros(2, dtype=torch.int32), workspace=None)
    rows = dict(T=torch.zeros((2, 12), dtype=torch.float64), info=torch.zeros((2, 21), dtype=torch.float64), status=torch.zeros(2, dtype=torch.int32),
                inlier_count=torch.zeros(2, dtype=torch.int32))
    for change in (dict(T=rows["T"][:1]), dict(info=torch.zeros((2, 6, 6), dtype=torch.float64)), dict(status=[0, 0])):
        with pytest.raises(ValueError, match="refined"):
            SequencePipeline.pose_window_step(st, dict(rows, **change))
    for kw in (dict(window=1), dict(spacings=(2, 2)), dict(capacity=0), dict(min_inliers=1.5), dict(huber_chi=0.0), dict(damping=float("inf")),
               dict(iterations=-1), dict(C_start=np.zeros(12))):
        with pytest.raises(ValueError):
            dropin.PoseWindow(**kw)
    w = dropin.PoseWindow(3, (1, 2))
    for args in ((np.zeros((2, 12)), np.zeros((2, 6, 6)), [0, 0], [0, 0]), (np.zeros((2, 4, 4)), np.zeros((2, 21)), [0, 0], [0, 0]),
                 (np.zeros((2, 4, 4)), np.zeros((2, 6, 6)), [0], [0, 0])):
        with pytest.raises(ValueError):
            w.step(*args)
    assert dropin.PoseWindow().window == 21 and dropin.PoseWindow().spacings == (1, 5, 10, 15, 20)


@pytest.mark.parametrize("seed", [0, 15])
def test_the_drop_in_reproduces_the_planted_study(seed):
    """Two seeds of the planted study - the first, and seed 15, the tightest of the twenty - through evaluation.PoseWindow, the
    shipped code: its trajectory is the restatement's bit for bit, so the figures DESIGN.md section 4m quotes are figures the
    package computes, and the window's ATE is below the chain's there too."""
    import evaluation as dropin
    c = wc.window_case("study", 21, wc.SPACINGS, 120, seed, outliers=0.03)
    _, state = ref.run(c)
    w = dropin.PoseWindow(21, wc.SPACINGS, 120)
    for i in range(120):
        w.step(c["T"][i].reshape(5, 3, 4), np.stack([pg.full_info(h) for h in c["info"][i]]), c["status"][i], c["inliers"][i])
    assert w.state["trajectory"].tobytes() == state["trajectory"].tobytes() and w.trajectory().tobytes() == pg.trajectory(state["trajectory"]).tobytes()
    assert pc.ate_rmse(w.state["trajectory"], c["truth"]) < pc.ate_rmse(c["C_chain"], c["truth"])
