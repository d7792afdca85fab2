"""libsslam_place.so on the device, bit for bit: the place step against its restatement (tests/place_ref.py) at every step and
against ssll_frame_signatures + ssll_loop_candidates run on the device on the prefix, row t; the edge log against its restatement;
a counter out of range; every pointer at its least alignment; state, outputs and workspace in poisoned guarded buffers
(tests/guarded.py); captured graphs - and online.LoopWindowPoseFrameStepper through the layers."""
import numpy as np
import pytest

import guarded
import place_cases as pcs
import place_ref as ref
import place_table as pt

pytestmark = pytest.mark.gpu
PLACE, LOG = "sslp_place_step", "sslp_edge_log_step"


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _bits(a):
    """The bits that are compared; a computed NaN counts as a NaN, whatever its sign and payload (the nan_score case: numpy and the
    device need not hand the same NaN on) - but the poison of tests/guarded.py, a NaN's bits too, stays itself."""
    a = np.ascontiguousarray(a)
    if a.dtype not in (np.float32, np.float64):
        return a
    wide = a.dtype == np.float64
    u = a.view(np.uint64 if wide else np.uint32).copy()
    u[np.isnan(a) & (u != (guarded.SENTINEL64 if wide else guarded.SENTINEL))] = 1
    return u


def _raw(T, t):
    return t.view(T.int64) if t.dtype == T.float64 else t


def _buf(T, shape, dtype, name):
    """A poisoned guarded buffer; float64 travels as int64 bits (tests/guarded.py has no float64 sentinel) -> (whole, middle)."""
    if dtype == T.float64:
        whole, mid = guarded.guarded(T, shape, T.int64, name=name)
        return whole, mid.view(T.float64)
    return guarded.guarded(T, shape, dtype, name=name)


def _poison(T, mid):
    _raw(T, mid).fill_(guarded._int_view(T, _raw(T, mid).dtype)[1])


def _assert_same(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    bad = np.flatnonzero(_bits(g).reshape(-1) != _bits(w).reshape(-1))
    assert bad.size == 0, f"{what} differs in {bad.size} elements, the first at flat index {bad[0]}: {g.reshape(-1)[bad[0]]!r} for {w.reshape(-1)[bad[0]]!r}"


def _counts(lib):
    return lib.launch_count(), lib.ext_launch_count(), lib.graph_launch_count(), lib.loop_launch_count(), lib.window_launch_count()


# ------------------------------------------------------------------------------------------------------------- the place bank
class Bank:
    """One place bank on the device: state, the frame's inputs, outputs and workspace each in a poisoned guarded buffer, the state
    made fresh (t = 0; raw and sum stay poison: nothing of them is read before it is written)."""

    def __init__(self, T, capacity, k, d, per_frame):
        from sslam_amd import lib
        self.T, self.lib, self.cap, self.d = T, lib, capacity, d
        self.state = {key: _buf(T, shape, dt, key) for key, (shape, dt) in lib.place_state_shapes(capacity, d).items()}
        self.state["t"][1].zero_()
        self.ins = dict(desc=_buf(T, (k, d), T.float32, "desc"), scores=_buf(T, (k,), T.float32, "scores"))
        self.outs = {key: _buf(T, shape, dt, key) for key, (shape, dt) in lib.place_out_shapes(per_frame, d).items()}
        self.ws = guarded.guarded(T, lib.place_workspace_bytes(capacity), T.uint8, name="workspace")

    def pairs(self):
        return list(self.state.items()) + list(self.ins.items()) + list(self.outs.items()) + [("workspace", self.ws)]

    def state_np(self):
        return {k: v[1].cpu().numpy() for k, v in self.state.items()}

    def step(self, desc, scores, c, what):
        """One guarded step -> (outputs, state before, state after) as dicts of numpy arrays."""
        T, lib = self.T, self.lib
        self.ins["desc"][1].copy_(T.from_numpy(np.ascontiguousarray(desc)))
        self.ins["scores"][1].copy_(T.from_numpy(np.ascontiguousarray(scores)))
        for whole, mid in self.outs.values():                      # poisoned again: a step writes every element
            _poison(T, mid)
        before = self.state_np()
        n0, others = lib.place_launch_count(), _counts(lib)
        back = lib.place_step({k: v[1] for k, v in self.state.items()}, self.ins["desc"][1], self.ins["scores"][1], c["min_gap"], c["min_sim"],
                              c["per_frame"], c["suppress"], out={k: v[1] for k, v in self.outs.items()}, workspace=self.ws[1])
        T.cuda.synchronize()
        assert lib.place_launch_count() - n0 == 3 and _counts(lib) == others, "three launches, of the sixth library"
        assert all(back[k] is self.outs[k][1] for k in lib.PLACE_OUT_KEYS)
        for name, (whole, mid) in self.pairs():
            guarded.assert_guards(whole, _raw(T, mid), f"{what} {name}")
        for k, (whole, mid) in self.outs.items():
            guarded.assert_written(mid, f"{what} {k}")
        assert np.array_equal(_bits(self.ins["desc"][1].cpu().numpy()), _bits(np.asarray(desc))), f"{what}: desc was written"
        return {k: v[1].cpu().numpy() for k, v in self.outs.items()}, before, self.state_np()


def _batch_row(T, lib, desc, scores, t, c):
    """Row t of ssll_loop_candidates over ssll_frame_signatures of the frames 0 .. t, on the device."""
    sig = lib.frame_signatures(desc[:t + 1], scores[:t + 1])
    first, second, sim, count = lib.loop_candidates(sig, c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"])
    per = c["per_frame"]
    return dict(first=first[t * per:(t + 1) * per], second=second[t * per:(t + 1) * per], sim=sim[t * per:(t + 1) * per], count=count[t:t + 1], sig=sig[t])


def run_bank(T, c, what, dev=None, batch_at=None):
    from sslam_amd import lib
    n_all, k, d = c["desc"].shape
    dev = Bank(T, c["capacity"], k, d, c["per_frame"]) if dev is None else dev
    want, final = pcs.bank_expected(c["name"])
    n = min(n_all, c["capacity"])
    desc_d, scores_d = T.from_numpy(c["desc"][:n]).cuda(), T.from_numpy(c["scores"][:n]).cuda()
    batch_at = range(n) if batch_at is None else batch_at
    for i in range(n_all):
        got, before, after = dev.step(c["desc"][i], c["scores"][i], c, f"{what} step {i}")
        for key in ref.OUT_KEYS:
            _assert_same(got[key], want[i][key], f"{what} step {i}: {key} against the restatement")
        if i >= n:                                                   # the bank is full: status 4, the state's bytes untouched
            assert got["status"][0] == 4 and all(np.array_equal(_bits(before[key]), _bits(after[key])) for key in ref.STATE_KEYS)
            continue
        assert after["t"].tolist() == [i + 1]
        rows = np.zeros(c["capacity"], bool)
        rows[i] = True
        assert np.array_equal(_bits(after["raw"])[~rows], _bits(before["raw"])[~rows]), f"{what} step {i}: raw changed outside row {i}"
        if i in batch_at:
            row = _batch_row(T, lib, desc_d, scores_d, i, c)
            for key, v in row.items():
                _assert_same(got[key], v.cpu().numpy(), f"{what} step {i}: {key} against the batch entries on the prefix")
    after = dev.state_np()
    _assert_same(after["raw"][:n], final["raw"][:n], f"{what}: raw")
    _assert_same(after["sum"], final["sum"], f"{what}: sum")
    return dev


BATCH_AT = {"frames_300_copies": (255, 256, 257, 299)}


@pytest.mark.parametrize("name", pcs.BANK_NAMES)
def test_banks_equal_the_restatement_and_the_batch_entries_on_the_prefix(T, name):
    """tests/test_place_cpu.py::test_contract_rows_of_the_place_bank says what each planting shows - the twins' order, the copies as
    first picks, the NaN score, the full bank; here the device gives those bits, and row t of the batch entries on the prefix: at
    every t where the bank holds at most 70 frames, at t = 255, 256, 257, 299 of the long one."""
    c = pcs.bank(name)
    assert len(c["desc"]) <= 70 or name in BATCH_AT
    run_bank(T, c, name, batch_at=BATCH_AT.get(name))


@pytest.mark.parametrize("t", [-1, 3, 2 ** 31 - 1])
def test_a_counter_out_of_range_answers_absent_and_leaves_the_state_alone(T, t):
    c = pcs.bank("capacity_3_k_1")
    dev = Bank(T, 3, 1, 128, 1)
    dev.state["t"][1].fill_(t)
    got, before, after = dev.step(c["desc"][0], c["scores"][0], c, f"counter {t}")
    assert got["status"].tolist() == [4] and got["first"].tolist() == [-1] and got["second"].tolist() == [-1] and got["count"].tolist() == [0]
    assert _bits(got["sim"]).tolist() == [0] and not _bits(got["sig"]).any(), "+0.0 in every word"
    for key in ref.STATE_KEYS:                                      # raw and sum still hold their poison
        assert np.array_equal(_bits(before[key]), _bits(after[key])), f"state {key} was written"
    assert after["t"].tolist() == [t]


@pytest.mark.parametrize("mode", ["lo", "hi"])
def test_every_pointer_at_its_least_alignment(T, mode):
    """Each operand of both entries at the alignment include/sslam_place.h states and no better, just past and just before a
    256-byte boundary: the same bits as the restatement."""
    c = pcs.bank("frames_70_d_256")
    with guarded.placed(guarded.Placement(pt.ALIGN[PLACE], mode)) as p:
        dev = Bank(T, c["capacity"], c["desc"].shape[1], 256, c["per_frame"])
    assert sorted(r["name"] for r in p.made) == sorted(pt.ALIGN[PLACE])
    for r in p.made:
        assert r["middle"].data_ptr() % 256 == (r["align"] if mode == "lo" else 256 - r["align"]), r["name"]
    run_bank(T, c, f"place_step {mode}", dev=dev, batch_at=())
    lc = pcs.log("base")
    with guarded.placed(guarded.Placement(pt.ALIGN[LOG], mode)) as p:
        log = Log(T, lc["capacity"], 4)
    assert sorted(r["name"] for r in p.made) == sorted(pt.ALIGN[LOG])
    for r in p.made:
        assert r["middle"].data_ptr() % 256 == (r["align"] if mode == "lo" else 256 - r["align"]), r["name"]
    run_log(T, lc, f"edge_log_step {mode}", dev=log)


def _capture(T, call):
    stream = T.cuda.Stream()
    stream.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(stream):
        call()
    T.cuda.current_stream().wait_stream(stream)
    T.cuda.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):
        call()
    return g


def test_ten_steps_replayed_from_a_captured_graph_equal_ten_launches(T):
    from sslam_amd import lib
    c = pcs.bank("nan_score_at_8")                                  # 14 frames: picks from frame 3 on, ten steps hold several
    want, _ = pcs.bank_expected(c["name"])
    desc, scores = T.from_numpy(c["desc"]).cuda(), T.from_numpy(c["scores"]).cuda()
    cur_d, cur_s = T.zeros_like(desc[0]), T.zeros_like(scores[0])
    state, out = lib.alloc_place_state(c["capacity"], 128), lib.alloc_place_out(c["per_frame"], 128)
    ws = T.empty(lib.place_workspace_bytes(c["capacity"]), dtype=T.uint8, device="cuda")
    call = lambda: lib.place_step(state, cur_d, cur_s, c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"], out=out, workspace=ws)
    g = _capture(T, call)
    states = []
    for replayed in (True, False):
        state["t"].zero_()
        state["raw"].fill_(7.0), state["sum"].fill_(-3.0)           # a fresh state is t = 0 and nothing else
        for i in range(10):
            cur_d.copy_(desc[i]), cur_s.copy_(scores[i])
            g.replay() if replayed else call()
            for k in ref.OUT_KEYS:
                _assert_same(out[k].cpu().numpy(), want[i][k], f"{'replay' if replayed else 'launch'} {i}: {k}")
        assert int(state["t"]) == 10
        states.append({k: v.cpu().numpy()[:10] for k, v in state.items()})
    for k in ref.STATE_KEYS:
        _assert_same(states[0][k], states[1][k], f"state {k}, replay against launches")


# --------------------------------------------------------------------------------------------------------------- the edge log
IN_KEYS = (("slot_first", "slot_first"), ("T", "new_T"), ("info", "new_info"), ("status", "new_status"), ("inliers", "new_inliers"))


class Log:
    def __init__(self, T, capacity, n_slots):
        from sslam_amd import lib
        self.T, self.lib, self.cap, self.E = T, lib, capacity, n_slots
        self.state = {key: _buf(T, shape, dt, key) for key, (shape, dt) in lib.edge_log_shapes(capacity, n_slots).items()}
        self.state["t"][1].zero_()
        E, f64, i32 = n_slots, T.float64, T.int32
        self.ins = dict(slot_first=_buf(T, (E,), i32, "slot_first"), T=_buf(T, (E, 12), f64, "new_T"), info=_buf(T, (E, 21), f64, "new_info"),
                        status=_buf(T, (E,), i32, "new_status"), inliers=_buf(T, (E,), i32, "new_inliers"))
        self.outs = {key: _buf(T, shape, dt, key) for key, (shape, dt) in lib.edge_log_out_shapes(n_slots).items()}

    def state_np(self):
        return {k: v[1].cpu().numpy() for k, v in self.state.items()}

    def step(self, c, i, what):
        T, lib = self.T, self.lib
        for key, _ in IN_KEYS:
            self.ins[key][1].copy_(T.from_numpy(np.ascontiguousarray(c[key][i])))
        for whole, mid in self.outs.values():
            _poison(T, mid)
        before = self.state_np()
        n0, others = lib.place_launch_count(), _counts(lib)
        back = lib.edge_log_step({k: v[1] for k, v in self.state.items()}, *(self.ins[key][1] for key, _ in IN_KEYS), c["n_odometry"], c["min_inliers"],
                                 c["loop_min_inliers"], out={k: v[1] for k, v in self.outs.items()})
        T.cuda.synchronize()
        assert lib.place_launch_count() - n0 == 1 and _counts(lib) == others, "one launch, of the sixth library"
        assert all(back[k] is self.outs[k][1] for k in lib.EDGE_LOG_OUT_KEYS)
        for name, (whole, mid) in list(self.state.items()) + list(self.ins.items()) + list(self.outs.items()):
            guarded.assert_guards(whole, _raw(T, mid), f"{what} {name}")
        for k, (whole, mid) in self.outs.items():
            guarded.assert_written(mid, f"{what} {k}")
        for key, _ in IN_KEYS:
            assert np.array_equal(_bits(self.ins[key][1].cpu().numpy()), _bits(np.asarray(c[key][i]))), f"{what}: input {key} was written"
        return {k: v[1].cpu().numpy() for k, v in self.outs.items()}, before, self.state_np()


def run_log(T, c, what, dev=None):
    """Every step of a log case on the device: the outputs and the step's E rows are the restatement's, every other state element -
    the poison of the rows not yet logged among them - is untouched."""
    E = c["slot_first"].shape[1]
    dev = Log(T, c["capacity"], E) if dev is None else dev
    want, final = pcs.log_expected(c["name"])
    state = ref.fresh_log(c["capacity"], E)
    for i in range(len(c["T"])):
        got, before, after = dev.step(c, i, f"{what} step {i}")
        r = ref.log_step(state, c["slot_first"][i], c["T"][i], c["info"][i], c["status"][i], c["inliers"][i], c["n_odometry"], c["min_inliers"],
                         c["loop_min_inliers"])
        for key in ref.LOG_OUT_KEYS:
            _assert_same(got[key], want[i][key], f"{what} step {i}: {key}")
            _assert_same(got[key], r[key], f"{what} step {i}: {key}")
        rows = np.zeros(c["capacity"] * E, bool)
        if i < c["capacity"]:
            rows[i * E:(i + 1) * E] = True
        else:
            assert got["status"][0] == 4 and not got["logged"].any()
        assert after["t"].tolist() == [min(i + 1, c["capacity"])]
        for key in ("log_first", "log_second", "log_T", "log_info"):
            a, b = _bits(after[key]), _bits(before[key])
            assert np.array_equal(a[rows], _bits(state[key])[rows]), f"{what} step {i}: {key} is not the restatement's"
            assert np.array_equal(a[~rows], b[~rows]), f"{what} step {i}: {key} changed outside the step's rows"
    return dev


@pytest.mark.parametrize("name", pcs.LOG_NAMES)
def test_edge_log_cases_equal_the_restatement(T, name):
    """The contract's rows (tests/test_place_cpu.py::test_contract_rows_of_the_edge_log says what each shows), one and sixteen slots,
    two windows' worth of steps, a full log."""
    run_log(T, pcs.log(name), name)


@pytest.mark.parametrize("t", [-1, 10, 2 ** 31 - 1])
def test_a_log_counter_out_of_range_writes_status_4_and_logs_nothing(T, t):
    c = pcs.log("base")
    dev = Log(T, 10, 4)
    dev.state["t"][1].fill_(t)
    got, before, after = dev.step(c, 9, f"log counter {t}")
    assert got["status"].tolist() == [4] and got["logged"].tolist() == [0, 0, 0, 0]
    assert all(np.array_equal(_bits(before[k]), _bits(after[k])) for k in ref.LOG_STATE_KEYS) and after["t"].tolist() == [t]


def test_ten_log_steps_replayed_from_a_captured_graph_equal_ten_launches(T):
    from sslam_amd import lib
    c = pcs.log("base")
    want, final = pcs.log_expected("base")
    ins = {key: T.from_numpy(np.ascontiguousarray(c[key])).cuda() for key, _ in IN_KEYS}
    cur = {key: T.zeros_like(ins[key][0]) for key, _ in IN_KEYS}
    state = lib.alloc_edge_log(10, 4)
    out = {k: T.zeros(shape, dtype=dt, device="cuda") for k, (shape, dt) in lib.edge_log_out_shapes(4).items()}
    call = lambda: lib.edge_log_step(state, *(cur[key] for key, _ in IN_KEYS), c["n_odometry"], c["min_inliers"], c["loop_min_inliers"], out=out)
    g = _capture(T, call)
    for replayed in (True, False):
        state["t"].zero_()
        state["log_T"].fill_(5.0), state["log_first"].fill_(77)
        for i in range(10):
            for key, _ in IN_KEYS:
                cur[key].copy_(ins[key][i])
            g.replay() if replayed else call()
            for k in ref.LOG_OUT_KEYS:
                _assert_same(out[k].cpu().numpy(), want[i][k], f"{'replay' if replayed else 'launch'} {i}: {k}")
        for k in ref.LOG_STATE_KEYS:
            _assert_same(state[k].cpu().numpy().reshape(final[k].shape), final[k], f"{'replay' if replayed else 'launches'}: state {k}")


# ---------------------------------------------------------------------------------------------------------- through the layers
E2E_THRESHOLD = 12.0        # px: the selector's keypoints sit on the 16-px patch grid (tests/test_gpu_window.py's choices throughout)
E2E_HYP, E2E_SEED, E2E_HUBER, E2E_ITER, E2E_MIN_INLIERS = 64, 5, 4.0, 5, 4
E2E_SPACINGS, E2E_WINDOW, E2E_CAPACITY = (1, 2, 3), 4, 50
E2E_DISTINCT, E2E_REPEATED = 32, 16                                 # 48 frames: the last third shows the first third again
E2E_FRAMES = E2E_DISTINCT + E2E_REPEATED
E2E_LOOPS = dict(min_gap=20, min_sim=0.3, per_frame=2, suppress=2, min_inliers=4)      # a repeat lies 32 frames back: eligible


_SEQ = {}


def _sequence(T, subcell):
    """48 synthetic frames and their depth: 32 distinct ones (tests/synth.py, tests/pose_depth_cases.py), then the first 16 again,
    images and depth alike.  Computed once per form, shared, not written to."""
    if subcell in _SEQ:
        return _SEQ[subcell]
    import pose_depth_cases
    import pose_eval_ref as pr
    import synth
    from sslam_amd import evaluation as ev
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K, subcell=subcell), inp["selector"], inp["refiner"],
                            device="cuda")
    order = list(range(E2E_DISTINCT)) + list(range(E2E_REPEATED))
    toks = T.from_numpy(synth.token_sequence(E2E_DISTINCT, pr.SEQ_GRID)[order]).cuda()
    depth = T.from_numpy(pose_depth_cases.sequence_depth(E2E_DISTINCT)[order]).cuda()
    _SEQ[subcell] = dict(pipe=pipe, toks=toks, depth=depth, cam=ev.Camera(), rule=MatchRule.mnn_ratio(0.9))
    return _SEQ[subcell]


def _stepper(seq, use_graph, loops=True):
    from sslam_amd.online import LoopWindowPoseFrameStepper, WindowPoseFrameStepper
    kw = dict(camera=seq["cam"], use_graph=use_graph, tokens_in=True, spacings=E2E_SPACINGS, window=E2E_WINDOW, threshold=E2E_THRESHOLD,
              hypotheses=E2E_HYP, seed=E2E_SEED, huber=E2E_HUBER, iterations=E2E_ITER, min_inliers=E2E_MIN_INLIERS, capacity=E2E_CAPACITY)
    if loops:
        return LoopWindowPoseFrameStepper(seq["pipe"], 48, 64, 480, 640, loops=E2E_LOOPS, **kw)
    return WindowPoseFrameStepper(seq["pipe"], 48, 64, 480, 640, **kw)


def _host(d):
    return {k: (_host(v) if isinstance(v, dict) else v.cpu().numpy()) for k, v in d.items() if v is not None and not isinstance(v, list)}


def _steps(T, seq, st, close_at=None):
    """The frames through the stepper -> per step, numpy copies of everything step() returns."""
    image = T.zeros((48, 64, 3), dtype=T.uint8, device="cuda")
    got, closed = [], None
    for i in range(E2E_FRAMES):
        if i == close_at:
            closed = st.close_loops()
        got.append(_host(st.step(image, seq["depth"][i], seq["toks"][i])))
    return got, closed


@pytest.mark.parametrize("use_graph, subcell", [(False, False), (True, False), (True, True)])
def test_loop_stepper_through_the_layers(T, use_graph, subcell):
    """One sequence, every promise of LoopWindowPoseFrameStepper: the window and the spacing rows are WindowPoseFrameStepper's bytes;
    the candidate rows are find_loop_candidates on the prefix; their matches and refined poses are the batched calls' on the same
    frame pairs; logged is the restatement fed with the device's rows, and loop slots ARE logged; close_loops is
    lib.pose_graph_sparse on the read-back log and loop_ref.optimize, bit for bit; and stepping on after close_loops gives the
    bytes it gives without the call."""
    import loop_ref
    from sslam_amd import evaluation as ev, lib
    seq = _sequence(T, subcell)
    pipe, S, L, n = seq["pipe"], len(E2E_SPACINGS), E2E_LOOPS["per_frame"], E2E_FRAMES
    E = S + L
    st = _stepper(seq, use_graph)
    got, closed_mid = _steps(T, seq, st, close_at=40)
    plain, _ = _steps(T, seq, _stepper(seq, use_graph, loops=False))
    for i, (g, w) in enumerate(zip(got, plain)):
        for key in lib.WINDOW_OUT_KEYS:
            _assert_same(g["window"][key], w["window"][key], f"frame {i}: window {key} against WindowPoseFrameStepper")
        for key in ("matches", "match_count", "value"):
            _assert_same(g[key][:S], w[key], f"frame {i}: {key} of the spacing rows")
        for key in lib.POSE_RANSAC_KEYS:
            _assert_same(g["pose"][key][:S], w["pose"][key], f"frame {i}: RANSAC's {key} of the spacing rows")
        for key in lib.POSE_REFINE_KEYS:
            _assert_same(g["pose"]["refined"][key][:S], w["pose"]["refined"][key], f"frame {i}: refined {key} of the spacing rows")
            _assert_same(g["loops"]["refined"][key], g["pose"]["refined"][key][S:], f"frame {i}: the loop rows' view of {key}")
    # the bank as the steps extracted it, and the candidates of every prefix
    ex = {k: T.from_numpy(np.stack([g[k] for g in got])).cuda() for k in st.bank_keys}
    first = np.stack([g["loops"]["first"] for g in got])
    for i, g in enumerate(got):
        cand = pipe.find_loop_candidates(ex["descriptors"][:i + 1], ex["scores"][:i + 1], E2E_LOOPS["min_gap"], E2E_LOOPS["min_sim"], L, E2E_LOOPS["suppress"])
        for key in ("first", "second", "sim"):
            _assert_same(g["loops"][key], cand[key][i * L:(i + 1) * L].cpu().numpy(), f"frame {i}: candidate {key} against find_loop_candidates")
        _assert_same(g["loops"]["count"], cand["count"][i:i + 1].cpu().numpy(), f"frame {i}: count")
        _assert_same(g["loops"]["sig"], cand["signatures"][i].cpu().numpy(), f"frame {i}: signature")
        assert g["loops"]["status"].tolist() == [0]
    for i in range(E2E_DISTINCT, n):
        assert first[i, 0] == i - E2E_DISTINCT, f"frame {i} shows frame {i - E2E_DISTINCT} again: its first candidate"
    # the loop rows against the batched calls on the same frame pairs
    kp = pipe.geometry_keypoints(ex)
    kd = ev.gather_keypoint_depth(pipe, seq["depth"].cpu().numpy(), kp, n)
    lf, ls = first.reshape(-1).astype(np.int32), np.where(first >= 0, np.arange(n)[:, None], -1).reshape(-1).astype(np.int32)
    lf_d, ls_d = T.from_numpy(lf).cuda(), T.from_numpy(ls).cuda()
    mm = pipe.match_pairs(ex["descriptors"], ex["scores"], first=lf_d, second=ls_d, rule=seq["rule"])
    est = pipe.estimate_poses(kp, kd, lf_d, ls_d, mm, seq["cam"], E2E_THRESHOLD, E2E_HYP, E2E_SEED)
    refined = pipe.refine_poses(kp, kd, lf_d, ls_d, mm, seq["cam"], est, E2E_THRESHOLD, E2E_HUBER, E2E_ITER)
    rows = lambda d: {k: v.cpu().numpy().reshape((n, L) + tuple(v.shape[1:])) for k, v in d.items()}
    mm, est, refined = rows({k: mm[k] for k in ("matches", "match_count", "value")}), rows(est), rows(refined)
    for i, g in enumerate(got):
        for key in mm:
            _assert_same(g[key][S:], mm[key][i], f"frame {i}: {key} of the loop rows against match_pairs")
        for key in lib.POSE_RANSAC_KEYS:
            _assert_same(g["pose"][key][S:], est[key][i], f"frame {i}: RANSAC's {key} of the loop rows")
        for key in lib.POSE_REFINE_KEYS:
            _assert_same(g["loops"]["refined"][key], refined[key][i], f"frame {i}: refined {key} of the loop rows")
    # the log: the restatement fed with the device's own rows
    log = ref.fresh_log(E2E_CAPACITY, E)
    loops_logged = 0
    for i, g in enumerate(got):
        r = g["pose"]["refined"]
        slot_first = np.array([i - s if i >= s else -1 for s in E2E_SPACINGS] + first[i].tolist(), np.int32)
        want = ref.log_step(log, slot_first, r["T"], r["info"], r["status"], r["inlier_count"], S, E2E_MIN_INLIERS, E2E_LOOPS["min_inliers"])
        _assert_same(g["loops"]["logged"], want["logged"], f"frame {i}: logged")
        assert g["loops"]["log_status"].tolist() == [0] and want["logged"][:S].tolist() == g["window"]["admitted"].tolist()
        loops_logged += int(want["logged"][S:].sum())
    assert loops_logged >= 1, "the repeated frames give loop slots that are logged: the restatement fed with the device's rows logs them"
    dlog = {k: v.cpu().numpy() for k, v in st.log["state"].items()}
    for key in ("log_first", "log_second", "log_T", "log_info"):
        _assert_same(dlog[key][:n * E], log[key][:n * E], f"the device's log: {key}")
    # close_loops: the sparse solver on the read-back log, and its restatement
    closed = st.close_loops()
    traj = st.win["state"]["trajectory"][0, :n].contiguous()
    dev = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    direct = dict(zip(lib.POSE_GRAPH_SPARSE_KEYS, lib.pose_graph_sparse(dev(log["log_first"][:n * E]), dev(log["log_second"][:n * E]), dev(log["log_T"][:n * E]),
                                                                        dev(log["log_info"][:n * E]), traj)))
    want = loop_ref.optimize(log["log_first"][:n * E], log["log_second"][:n * E], log["log_T"][:n * E], log["log_info"][:n * E], traj.cpu().numpy())
    _assert_same(closed["C"], direct["C"][0].cpu().numpy(), "close_loops: C against lib.pose_graph_sparse")
    _assert_same(closed["C"], want["C"], "close_loops: C against loop_ref.optimize")
    _assert_same(closed["edge_chi2"], want["edge_chi2"], "close_loops: edge_chi2")
    _assert_same(closed["cg_steps"], want["cg_steps"].astype(np.int64), "close_loops: cg_steps")
    for key in ("status", "iterations", "used_edges", "skipped_edges", "failed_row"):
        assert closed[key] == int(want[key]) == int(direct[key][0]), key
    assert np.float64(closed["cost"]).tobytes() == np.float64(want["cost"]).tobytes() and np.float64(closed["cost_in"]).tobytes() == np.float64(want["cost_in"]).tobytes()
    frames, slots = np.nonzero(log["log_first"][:n * E].reshape(n, E)[:, S:] >= 0)
    assert closed["loop_edges"].tolist() == [[int(first[f, s]), int(f)] for f, s in zip(frames, slots)] and len(closed["loop_edges"]) == loops_logged
    assert closed["trajectory"].shape == (n, 4, 4) and closed_mid["trajectory"].shape == (40, 4, 4) and st.trajectory().shape == (n, 4, 4)
    # the same frames again after reset(), this time without close_loops between the steps: the same bytes
    if use_graph:
        n0 = _counts(lib), lib.place_launch_count()
        st.step(T.zeros((48, 64, 3), dtype=T.uint8, device="cuda"), seq["depth"][0], seq["toks"][0])
        assert (_counts(lib), lib.place_launch_count()) == n0, "a replayed step makes no library call"
    st.reset()
    again, _ = _steps(T, seq, st)
    for i, (a, b) in enumerate(zip(got, again)):
        for key in lib.WINDOW_OUT_KEYS:
            _assert_same(b["window"][key], a["window"][key], f"without close_loops, frame {i}: window {key}")
        for key in ("first", "second", "sim", "count", "status", "sig", "logged", "log_status"):
            _assert_same(b["loops"][key], a["loops"][key], f"without close_loops, frame {i}: loops {key}")
        _assert_same(b["pose"]["refined"]["T"], a["pose"]["refined"]["T"], f"without close_loops, frame {i}: refined T")
    for key, v in st.log["state"].items():
        _assert_same(v.cpu().numpy()[:n * E] if key != "t" else v.cpu().numpy(), dlog[key][:n * E] if key != "t" else dlog[key], f"the log after the second run: {key}")


def test_past_capacity_the_window_carries_on_and_the_new_entries_answer_4(T):
    """capacity 6 of 10 frames: from frame 6 on the place step and the log answer 4, the candidate rows read absent, and the window's
    outputs stay WindowPoseFrameStepper's."""
    from sslam_amd import lib
    from sslam_amd.online import LoopWindowPoseFrameStepper, WindowPoseFrameStepper
    seq = _sequence(T, False)
    kw = dict(camera=seq["cam"], use_graph=False, tokens_in=True, spacings=E2E_SPACINGS, window=E2E_WINDOW, threshold=E2E_THRESHOLD, hypotheses=E2E_HYP,
              seed=E2E_SEED, huber=E2E_HUBER, iterations=E2E_ITER, min_inliers=E2E_MIN_INLIERS, capacity=6)
    a = LoopWindowPoseFrameStepper(seq["pipe"], 48, 64, 480, 640, loops=dict(E2E_LOOPS, min_gap=2), **kw)
    b = WindowPoseFrameStepper(seq["pipe"], 48, 64, 480, 640, **kw)
    image = T.zeros((48, 64, 3), dtype=T.uint8, device="cuda")
    S = len(E2E_SPACINGS)
    for i in range(10):
        x, y = _host(a.step(image, seq["depth"][i], seq["toks"][i])), _host(b.step(image, seq["depth"][i], seq["toks"][i]))
        for key in lib.WINDOW_OUT_KEYS:
            _assert_same(x["window"][key], y["window"][key], f"frame {i}: window {key}")
        full = i >= 6
        assert x["loops"]["status"].tolist() == [4 if full else 0] and x["loops"]["log_status"].tolist() == [4 if full else 0]
        if full:
            assert (x["loops"]["first"] == -1).all() and not x["loops"]["logged"].any() and (x["pose"]["refined"]["status"][S:] == 3).all()
    assert a.close_loops()["trajectory"].shape == (6, 4, 4) and int(a.log["state"]["t"]) == 6 and int(a.place["state"]["t"]) == 6
