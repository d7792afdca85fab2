"""libsslam_window.so on the device against its float64 restatement (tests/window_ref.py), bit for bit: the shapes at which the
ring can go wrong, the contract's rows, several windows in one launch, every step against sslg_pose_graph on the window-local
operands, every pointer at its least alignment, state, outputs and workspace in poisoned guarded buffers (tests/guarded.py) with
exactly the stated elements changing, a captured graph - and online.WindowPoseFrameStepper through the layers."""
import numpy as np
import pytest

import guarded
import window_cases as wc
import window_ref as ref
import window_table as wt

pytestmark = pytest.mark.gpu
ENTRY = "sslw_window_step"


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _raw(T, t):
    return t.view(T.int64) if t.dtype == T.float64 else t


def _buf(T, shape, dtype, name):
    """A poisoned guarded buffer; float64 travels as int64 bits (tests/guarded.py has no float64 sentinel) -> (whole, middle)."""
    if dtype == T.float64:
        whole, mid = guarded.guarded(T, shape, T.int64, name=name)
        return whole, mid.view(T.float64)
    return guarded.guarded(T, shape, dtype, name=name)


def _assert_same(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    bad = np.flatnonzero(_bits(g).reshape(-1) != _bits(w).reshape(-1))
    assert bad.size == 0, f"{what} differs from the restatement in {bad.size} elements, the first at flat index {bad[0]}: " \
                          f"{g.reshape(-1)[bad[0]]!r} for {w.reshape(-1)[bad[0]]!r}"


class Device:
    """n_windows windows of one shape on the device: state, step inputs, outputs and workspace each in a poisoned guarded buffer,
    the state made fresh (t = 0, ring_first = -1; everything else stays poison: nothing of it is read before it is written)."""

    def __init__(self, T, window, n_spacings, capacity, n_windows=1, with_start=False):
        from sslam_amd import lib
        self.T, self.lib, self.W, self.S, self.cap, self.n = T, lib, window, n_spacings, capacity, n_windows
        self.state = {k: _buf(T, shape, dt, k) for k, (shape, dt) in lib.window_state_shapes(n_windows, window, n_spacings, capacity).items()}
        self.state["t"][1].zero_()
        self.state["ring_first"][1].fill_(-1)
        f64, i32 = T.float64, T.int32
        self.ins = dict(spacings=_buf(T, (n_spacings,), i32, "spacings"), T=_buf(T, (n_windows, n_spacings, 12), f64, "new_T"),
                        info=_buf(T, (n_windows, n_spacings, 21), f64, "new_info"), status=_buf(T, (n_windows, n_spacings), i32, "new_status"),
                        inliers=_buf(T, (n_windows, n_spacings), i32, "new_inliers"))
        self.start = _buf(T, (n_windows, 12), f64, "C_start") if with_start else None
        self.outs = {k: _buf(T, shape, dt, k) for k, (shape, dt) in lib.window_out_shapes(n_windows, window, n_spacings).items()}
        self.ws = guarded.guarded(T, lib.window_workspace_bytes(n_windows, window, n_spacings), T.uint8, name="workspace")

    def pairs(self):
        extra = [("C_start", self.start)] if self.start is not None else []
        return list(self.state.items()) + list(self.ins.items()) + list(self.outs.items()) + extra + [("workspace", self.ws)]

    def state_np(self):
        return {k: v[1].cpu().numpy() for k, v in self.state.items()}

    def step(self, spacings, Tm, info, status, inliers, C_start, min_inliers, chi, damping, n_iter, what, written=True):
        """One guarded launch -> (outputs, state before, state after) as dicts of numpy arrays with the window axis."""
        T, lib = self.T, self.lib
        for key, a in (("spacings", spacings), ("T", Tm), ("info", info), ("status", status), ("inliers", inliers)):
            self.ins[key][1].copy_(T.from_numpy(np.ascontiguousarray(a)).reshape(self.ins[key][1].shape))
        if self.start is not None:
            self.start[1].copy_(T.from_numpy(np.ascontiguousarray(C_start)).reshape(self.n, 12))
        for whole, mid in self.outs.values():                      # poisoned again: this step writes every element
            _raw(T, mid).fill_(guarded._int_view(T, _raw(T, mid).dtype)[1])
        before = self.state_np()
        n0, counts = lib.window_launch_count(), (lib.launch_count(), lib.graph_launch_count())
        back = lib.window_step({k: v[1] for k, v in self.state.items()}, self.ins["spacings"][1], self.ins["T"][1], self.ins["info"][1],
                               self.ins["status"][1], self.ins["inliers"][1], None if self.start is None else self.start[1], min_inliers, chi,
                               damping, n_iter, out={k: v[1] for k, v in self.outs.items()}, workspace=self.ws[1])
        T.cuda.synchronize()
        assert lib.window_launch_count() - n0 == 1 and (lib.launch_count(), lib.graph_launch_count()) == counts, "one launch, of the fifth library"
        assert all(back[k] is self.outs[k][1] for k in lib.WINDOW_OUT_KEYS)
        for name, (whole, mid) in self.pairs():
            guarded.assert_guards(whole, _raw(T, mid), f"{what} {name}")
        if written:
            for k, (whole, mid) in self.outs.items():
                guarded.assert_written(_raw(T, mid), f"{what} {k}")
        for key, a in (("spacings", spacings), ("T", Tm), ("info", info), ("status", status), ("inliers", inliers)):
            assert np.array_equal(_bits(self.ins[key][1].cpu().numpy().reshape(np.shape(a))), _bits(np.asarray(a))), f"{what}: input {key} was written"
        return {k: v[1].cpu().numpy() for k, v in self.outs.items()}, before, self.state_np()


def _stated(t, W, S, capacity):
    """The state elements a step at counter t writes: name -> boolean mask over one window's array."""
    base = max(0, t - W + 1)
    slots, rows, frames = np.zeros(W * S, bool), np.zeros(W, bool), np.zeros(capacity, bool)
    slots[(t % W) * S:(t % W) * S + S] = True
    rows[[j % W for j in range(base, t + 1)]] = True
    frames[[j for j in range(base, t + 1) if j < capacity]] = True
    return dict(t=np.ones((), bool), ring_first=slots, ring_second=slots, ring_T=np.repeat(slots[:, None], 12, 1), ring_info=np.repeat(slots[:, None], 21, 1),
                ring_C=np.repeat(rows[:, None], 12, 1), trajectory=np.repeat(frames[:, None], 12, 1))


def run_cases(T, cases, what, with_start=None, dev=None):
    """Every step of `cases` (one shape; one window each of one launch) on the device, each step held to the restatement: the
    outputs bit for bit, the stated state elements bit for bit, every other state element untouched."""
    c0 = cases[0]
    W, S, cap = c0["window"], len(c0["spacings"]), c0["capacity"]
    with_start = c0["C_start"] is not None if with_start is None else with_start
    dev = Device(T, W, S, cap, len(cases), with_start) if dev is None else dev
    states = [ref.fresh_state(W, S, cap) for _ in cases]
    ops = wc.stacked(cases)
    start = np.stack([c["C_start"] for c in cases]) if with_start else None
    for i in range(len(c0["T"])):
        got, before, after = dev.step(c0["spacings"], ops["T"][i], ops["info"][i], ops["status"][i], ops["inliers"][i], start, c0["min_inliers"],
                                      c0["chi"], c0["damping"], c0["n_iter"], f"{what} step {i}")
        for w, c in enumerate(cases):
            want = ref.step(states[w], c["spacings"], c["T"][i], c["info"][i], c["status"][i], c["inliers"][i], c["C_start"], c["min_inliers"], c["chi"],
                            c["damping"], c["n_iter"])
            for k in ref.OUT_KEYS:
                _assert_same(got[k][w], want[k], f"{what} step {i} window {w}: {k}")
            for k, mask in _stated(i, W, S, cap).items():
                b, a, r = _bits(before[k][w]), _bits(after[k][w]), _bits(states[w][k])
                assert np.array_equal(a[mask], r[mask]), f"{what} step {i} window {w}: state {k} is not the restatement's"
                assert np.array_equal(a[~mask], b[~mask]), f"{what} step {i} window {w}: state {k} changed outside the stated elements"
    return dev, states


SHAPES = wc.shape_cases()
CONTRACT = wc.contract_cases()


@pytest.mark.parametrize("index", range(len(SHAPES)), ids=[c["name"] for c in SHAPES])
def test_shapes_equal_the_restatement(T, index):
    c = SHAPES[index]
    assert len(c["T"]) > c["window"], "the ring wraps"
    outs, _ = wc.expected(c["name"])
    assert all(o["status"] == 0 and o["iterations"] >= 1 for o in outs[1:]), "the case takes steps"
    if c["name"] == "window_4_edges_drop":
        assert outs[-1]["dropped_edges"] > 0
    if c["name"] == "window_4_spacing_past_the_window":
        assert not any(o["admitted"][2] for o in outs)
    run_cases(T, [c], c["name"])


@pytest.mark.parametrize("index", range(len(CONTRACT)), ids=[c["name"] for c in CONTRACT])
def test_contract_rows_equal_the_restatement(T, index):
    """tests/test_window_cpu.py::test_contract_rows_of_the_restatement says what each row shows; here the device gives those bits."""
    c = CONTRACT[index]
    dev, states = run_cases(T, [c], c["name"])
    if c["name"] == "short_trajectory":
        assert states[0]["trajectory"].shape == (5, 12) and int(states[0]["t"]) == 9
    if c["name"] == "start_given":                                 # the same steps with NULL: [I | 0]
        run_cases(T, [dict(c, C_start=None)], "start NULL")


@pytest.mark.parametrize("t", [-1, -2 ** 31, 2 ** 31 - 1])
def test_a_counter_out_of_range_writes_status_4_and_nothing_else(T, t):
    c = wc.case("base")
    dev = Device(T, 4, 3, 9, 2)
    dev.state["t"][1].copy_(T.tensor([t, 0], dtype=T.int32))       # the window beside it steps as ever
    got, before, after = dev.step(c["spacings"], np.stack([c["T"][0]] * 2), np.stack([c["info"][0]] * 2), np.stack([c["status"][0]] * 2),
                                  np.stack([c["inliers"][0]] * 2), None, 12, 4.0, 0.0, 2, f"counter {t}", written=False)
    sentinel32, sentinel64 = np.int32(guarded.SENTINEL), np.int64(guarded.SENTINEL64)
    for k, v in got.items():
        if k == "status":
            assert v.tolist() == [4, 3]
        else:
            poison = (v[0].view(np.int64) == sentinel64) if v.dtype == np.float64 else (v[0] == sentinel32)
            assert poison.all() and not ((v[1].view(np.int64) == sentinel64) if v.dtype == np.float64 else (v[1] == sentinel32)).any(), k
    for k in ref.STATE_KEYS:
        assert np.array_equal(_bits(before[k][0]), _bits(after[k][0])), f"state {k} of the refused window was written"
    assert after["t"].tolist() == [t, 1]


def test_five_windows_in_one_launch_are_independent(T):
    """Five seeds of one shape in one launch: every window's outputs and state are what the restatement gives it alone, so the
    offsets past window 0 are exercised - with a status-2 window (all-zero information) among them."""
    cases = [wc.window_case(f"seed {seed}", 5, (1, 2, 4), 9, seed, outliers=0.1) for seed in (31, 32, 33, 34, 35)]
    cases[2] = dict(cases[2], info=np.zeros_like(cases[2]["info"]))
    _, states = run_cases(T, cases, "five windows")
    assert len({s["ring_C"].tobytes() for s in states}) == 5


def test_every_step_is_the_pose_graph_on_the_window_local_operands(T):
    """At every step C, status, iterations, the costs and edge_chi2 equal sslg_pose_graph - the banded solver of the third library -
    run on the device on the window-local operands at band = W - 1: the dense solve gives the banded statement's bits."""
    from sslam_amd import lib
    for name in ("window_4_edges_drop", "window_21_five_spacings"):
        c = wc.case(name)
        W, S = c["window"], len(c["spacings"])
        state = ref.fresh_state(W, S, c["capacity"])
        dstate, dout = lib.alloc_window_state(W, S, c["capacity"]), lib.alloc_window_out(W, S)
        sp = T.from_numpy(c["spacings"]).cuda()
        for i in range(len(c["T"])):
            loc = ref.step(state, c["spacings"], c["T"][i], c["info"][i], c["status"][i], c["inliers"][i], None, c["min_inliers"], c["chi"],
                           c["damping"], c["n_iter"], detail=True)["local"]
            got = lib.window_step(dstate, sp, *(T.from_numpy(np.ascontiguousarray(c[k][i])).cuda() for k in ("T", "info", "status", "inliers")),
                                  None, c["min_inliers"], c["chi"], c["damping"], c["n_iter"], out=dout)
            if i == 0:
                continue
            banded = dict(zip(lib.POSE_GRAPH_KEYS, lib.pose_graph(*(T.from_numpy(np.ascontiguousarray(loc[k])).cuda() for k in ("first", "second", "T", "info", "C_in")),
                                                                  W - 1, c["chi"], c["damping"], c["n_iter"])))
            nn = len(loc["C_in"])
            assert T.equal(_raw(T, got["C_window"][0, :nn]), _raw(T, banded["C"][0])), (name, i)
            for k in ("status", "iterations", "used_edges", "failed_row", "cost_in", "cost", "edge_chi2"):
                assert T.equal(_raw(T, got[k]), _raw(T, banded[k])), (name, i, k)
            assert int(got["dropped_edges"]) == int(banded["skipped_edges"])


@pytest.mark.parametrize("mode", ["lo", "hi"])
def test_every_pointer_at_its_least_alignment(T, mode):
    """Each operand at the alignment include/sslam_window.h states and no better, just past and just before a 256-byte boundary:
    the same bits as the restatement."""
    c = wc.case("start_given")
    with guarded.placed(guarded.Placement(wt.ALIGN[ENTRY], mode)) as p:
        dev = Device(T, c["window"], len(c["spacings"]), c["capacity"], 1, True)
    assert sorted(r["name"] for r in p.made) == sorted(wt.ALIGN[ENTRY])
    for r in p.made:
        a = r["align"]
        assert r["middle"].data_ptr() % 256 == (a if mode == "lo" else 256 - a), r["name"]
    run_cases(T, [c], f"window_step {mode}", dev=dev)


@pytest.mark.parametrize("W", [4, 24])
def test_ten_steps_replayed_from_a_captured_graph_equal_ten_launches(T, W):
    """W = 24 asks for 80 040 bytes of LDS: past 60 KB the entry raises the kernel's allowance on every call, here inside the
    capture too."""
    from sslam_amd import lib
    c = wc.window_case("capture", W, (1, 2, 3), 10, 41, outliers=0.1)
    S = 3
    assert (wt.lds_bytes(W) > 60 * 1024) == (W == 24)
    want, _ = ref.run(c)
    keys = ("T", "info", "status", "inliers")
    ins = {k: T.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in keys}
    sp = T.from_numpy(c["spacings"]).cuda()
    cur = {k: T.zeros_like(ins[k][0]) for k in keys}
    state, out = lib.alloc_window_state(W, S, 10), lib.alloc_window_out(W, S)
    ws = T.empty(lib.window_workspace_bytes(1, W, S), dtype=T.uint8, device="cuda")
    call = lambda: lib.window_step(state, sp, cur["T"], cur["info"], cur["status"], cur["inliers"], None, 12, 4.0, 0.0, 2, out=out, workspace=ws)
    stream = T.cuda.Stream()
    stream.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(stream):
        call()
    T.cuda.current_stream().wait_stream(stream)
    T.cuda.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):
        call()
    for replayed in (True, False):
        for v in state.values():
            v.zero_()
        state["ring_first"].fill_(-1)
        for i in range(10):
            for k in keys:
                cur[k].copy_(ins[k][i])
            g.replay() if replayed else call()
            for k in ref.OUT_KEYS:
                _assert_same(out[k].cpu().numpy()[0], want[i][k], f"{'replay' if replayed else 'launch'} {i}: {k}")
        assert int(state["t"]) == 10


# ---------------------------------------------------------------------------------------------------------- through the layers
E2E_THRESHOLD = 12.0        # px: the selector's keypoints sit on the 16-px patch grid (tests/test_gpu_pose_refine.py's choice)
E2E_HYP, E2E_SEED, E2E_HUBER, E2E_ITER, E2E_MIN_INLIERS = 64, 5, 4.0, 5, 4
E2E_FRAMES, E2E_SPACINGS, E2E_WINDOW = 8, (1, 2, 3), 4


_SEQ = {}


def _sequence(T, subcell):
    """The synthetic frames and depth of the PoseFrameStepper tests, and the batched rows of every pair a step refines - by
    match_pairs, estimate_poses and refine_poses on the whole bank, the calls odometry(refine=True) makes for a pair list
    (tests/test_gpu_pose_refine.py::test_odometry_with_refinement_is_odometry_followed_by_refine_poses holds odometry to exactly
    these rows, so a step's rows equal odometry's through it).  subcell: a pipeline that localises its keypoints, whose geometry
    bank is the refined one.  Computed once per form, shared, not written to."""
    if subcell in _SEQ:
        return _SEQ[subcell]
    import pose_depth_cases
    import pose_eval_ref as pr
    from sslam_amd import evaluation as ev
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K, subcell=subcell), inp["selector"], inp["refiner"],
                            device="cuda")
    n = E2E_FRAMES
    toks, depth, cam, rule = T.from_numpy(inp["tokens"]).cuda()[:n], pose_depth_cases.sequence_depth()[:n], ev.Camera(), MatchRule.mnn_ratio(0.9)
    ex = pipe.extract(toks, None)
    kp = pipe.geometry_keypoints(ex)
    assert ("keypoints_subpixel" in ex) == subcell and (kp is ex["keypoints_pixel"]) == (not subcell)
    kd = ev.gather_keypoint_depth(pipe, depth, kp, n)
    first = [i - s if i >= s else -1 for i in range(n) for s in E2E_SPACINGS]
    second = [i for i in range(n) for _ in E2E_SPACINGS]
    mm = pipe.match_pairs(ex["descriptors"], ex["scores"], first=first, second=second, rule=rule)
    est = pipe.estimate_poses(kp, kd, first, second, mm, cam, E2E_THRESHOLD, E2E_HYP, E2E_SEED)
    refined = pipe.refine_poses(kp, kd, first, second, mm, cam, est, E2E_THRESHOLD, E2E_HUBER, E2E_ITER)
    S = len(E2E_SPACINGS)
    rows = lambda d: {k: v.cpu().numpy().reshape((n, S) + tuple(v.shape[1:])) for k, v in d.items()}
    _SEQ[subcell] = dict(pipe=pipe, toks=toks, depth=T.from_numpy(depth).cuda(), cam=cam, rule=rule, first=np.array(first).reshape(n, S),
                         est=rows(est), refined=rows(refined))
    return _SEQ[subcell]


@pytest.fixture(scope="module")
def seq(T):
    return _sequence(T, False)


def _stepper(seq, use_graph, window=E2E_WINDOW, **kw):
    from sslam_amd.online import WindowPoseFrameStepper
    return WindowPoseFrameStepper(seq["pipe"], 48, 64, 480, 640, camera=seq["cam"], use_graph=use_graph, tokens_in=True, spacings=E2E_SPACINGS,
                                  window=window, threshold=E2E_THRESHOLD, hypotheses=E2E_HYP, seed=E2E_SEED, huber=E2E_HUBER,
                                  iterations=E2E_ITER, min_inliers=E2E_MIN_INLIERS, capacity=6, **kw)


def _steps(T, seq, st):
    """The frames through the stepper -> per step, the numpy copies of "pose" (with "refined") and "window"."""
    image = T.zeros((48, 64, 3), dtype=T.uint8, device="cuda")
    host = lambda d: {k: (host(v) if isinstance(v, dict) else v.cpu().numpy()) for k, v in d.items()}
    got = []
    for i in range(E2E_FRAMES):
        out = st.step(image, seq["depth"][i], seq["toks"][i])
        got.append(dict(pose=host(out["pose"]), window=host(out["window"]), pair_first=out["pair_first"]))
    return got


@pytest.mark.parametrize("use_graph, subcell", [(False, False), (True, False), (True, True)])
def test_window_stepper_equals_the_batched_rows_and_the_restatement(T, use_graph, subcell):
    """subcell: the stepper's geometry bank follows pipe.geometry_keypoints - the rows are those of the refined keypoints."""
    from sslam_amd import lib
    seq = _sequence(T, subcell)
    st = _stepper(seq, use_graph)
    assert ("keypoints_subpixel" in st.bank) == subcell
    got = _steps(T, seq, st)
    S = len(E2E_SPACINGS)
    state = ref.fresh_state(E2E_WINDOW, S, 6)
    admitted = 0
    for i, g in enumerate(got):
        assert set(g["pose"]) == set(lib.POSE_RANSAC_KEYS) | {"refined"} and set(g["pose"]["refined"]) == set(lib.POSE_REFINE_KEYS)
        assert tuple(g["window"]) == lib.WINDOW_OUT_KEYS and g["pair_first"] == seq["first"][i].tolist()
        for k in range(S):
            if seq["first"][i, k] < 0:
                assert g["pose"]["refined"]["status"][k] == 3, "an absent pair is not attempted"
                continue
            for key in lib.POSE_RANSAC_KEYS:
                assert g["pose"][key][k].tobytes() == seq["est"][key][i, k].tobytes(), f"frame {i} spacing {k}: RANSAC's {key}"
            for key in lib.POSE_REFINE_KEYS:
                assert g["pose"]["refined"][key][k].tobytes() == seq["refined"][key][i, k].tobytes(), f"frame {i} spacing {k}: refined {key}"
        r = g["pose"]["refined"]
        want = ref.step(state, np.array(E2E_SPACINGS, np.int32), r["T"], r["info"], r["status"], r["inlier_count"], None, E2E_MIN_INLIERS, 4.0, 0.0, 2)
        for key in ref.OUT_KEYS:
            _assert_same(g["window"][key], want[key], f"frame {i}: window {key}")
        admitted += int(want["admitted"].sum())
    assert admitted > 0 and any(g["window"]["status"] == 0 for g in got), "the synthetic sequence has pairs the window admits and optimises"
    traj = st.trajectory()
    assert traj.shape == (6, 4, 4), "capacity 6 of 8 frames"
    import pose_graph_ref as pg
    assert traj.tobytes() == pg.trajectory(state["trajectory"]).tobytes()
    if use_graph:
        n0 = lib.launch_count(), lib.window_launch_count()
        st.step(T.zeros((48, 64, 3), dtype=T.uint8, device="cuda"), seq["depth"][0], seq["toks"][0])
        assert (lib.launch_count(), lib.window_launch_count()) == n0, "a replayed step makes no library call"
    st.reset()                                                     # the same frames again: the same bits
    again = _steps(T, seq, st)
    for i, (a, b) in enumerate(zip(got, again)):
        for key in ref.OUT_KEYS:
            _assert_same(b["window"][key], a["window"][key], f"after reset, frame {i}: window {key}")
        assert b["pose"]["refined"]["T"].tobytes() == a["pose"]["refined"]["T"].tobytes()
    assert st.trajectory().tobytes() == traj.tobytes()


def test_window_stepper_graph_and_launches_agree_and_the_pose_stepper_is_as_it_was(T, seq):
    """The graph against the launches at window 4 and at window 24, whose launch raises the kernel's LDS allowance inside the
    captured step."""
    from sslam_amd import lib
    from sslam_amd.online import PoseFrameStepper
    for window in (E2E_WINDOW, 24):
        a, b = _steps(T, seq, _stepper(seq, True, window)), _steps(T, seq, _stepper(seq, False, window))
        for i, (x, y) in enumerate(zip(a, b)):
            for key in ref.OUT_KEYS:
                _assert_same(x["window"][key], y["window"][key], f"window {window}, frame {i}: {key}, graph against launches")
    st = PoseFrameStepper(seq["pipe"], 48, 64, 480, 640, camera=seq["cam"], use_graph=False, tokens_in=True, threshold=E2E_THRESHOLD,
                          hypotheses=E2E_HYP, seed=E2E_SEED, refine=True, huber=E2E_HUBER, iterations=E2E_ITER)
    image = T.zeros((48, 64, 3), dtype=T.uint8, device="cuda")
    for i in range(4):
        out = st.step(image, seq["depth"][i], seq["toks"][i])
        if i == 0:
            assert out["pose"] is None
            continue
        assert set(out["pose"]) == set(lib.POSE_RANSAC_KEYS) | {"refined"} and "window" not in out
        for key in lib.POSE_REFINE_KEYS:
            assert out["pose"]["refined"][key].cpu().numpy().tobytes() == seq["refined"][key][i, 0].tobytes(), f"frame {i}: {key}"
