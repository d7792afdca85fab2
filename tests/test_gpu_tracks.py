"""libsslam_track.so on the device, bit for bit against tests/track_ref.py: links, ids, landmarks and the online step, outputs and
state, each entry into poisoned guarded buffers (tests/guarded.py) with its launches counted; every pointer at its least alignment;
the two invariants of the landmarks; the step against the batch entries run on the device on every prefix, past capacity, from a
captured graph; every refusal launching and writing nothing; and the layers: SequencePipeline, odometry_graph(tracks=) and
online.TrackWindowPoseFrameStepper."""
import ctypes

import numpy as np
import pytest

import guarded
import track_cases as tc
import track_ref as ref
import track_table as tt

pytestmark = pytest.mark.gpu
LINK, IDS, LAND, STEP = "sslt_link_pairs", "sslt_track_ids", "sslt_landmarks", "sslt_track_step"


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _assert_same(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    bad = np.flatnonzero(_bits(g).reshape(-1) != _bits(w).reshape(-1))
    assert bad.size == 0, f"{what} differs in {bad.size} elements, the first at flat index {bad[0]}: {g.reshape(-1)[bad[0]]!r} for {w.reshape(-1)[bad[0]]!r}"


def _raw(T, t):
    return t.view(T.int64) if t.dtype == T.float64 else t


def _out(T, shape, dtype, name):
    """A poisoned guarded output; float64 travels as int64 bits (tests/guarded.py has no float64 sentinel) -> (whole, middle)."""
    if dtype == T.float64:
        whole, mid = guarded.guarded(T, shape, T.int64, name=name)
        return whole, mid.view(T.float64)
    return guarded.guarded(T, shape, dtype, name=name)


def _in(T, array, name):
    """A guarded input (None stays None) -> (whole, middle)."""
    if array is None:
        return None, None
    a = np.ascontiguousarray(array)
    if a.dtype == np.float64:
        whole, mid = guarded.guarded_input(T, a.view(np.int64), name=name)
        return whole, mid.view(T.float64)
    return guarded.guarded_input(T, a, name=name)


def _poison(T, mid):
    _raw(T, mid).fill_(guarded._int_view(T, _raw(T, mid).dtype)[1])


def _others(lib):
    return (lib.launch_count(), lib.ext_launch_count(), lib.graph_launch_count(), lib.loop_launch_count(), lib.window_launch_count(),
            lib.place_launch_count(), lib.conf_launch_count(), lib.weight_launch_count())


class Call:
    """One guarded call of an entry: inputs between NaN bands, outputs poisoned, launches counted, bands and inputs checked after."""

    def __init__(self, T, entry, ins: dict, shapes: dict, keys, workspace=None, fill=0xA5):
        self.T, self.entry, self.keys = T, entry, keys
        self.host = {k: v for k, v in ins.items()}
        self.ins = {k: _in(T, v, k) for k, v in ins.items()}
        rename = (lambda k: "out_" + k if k in ("track_id", "age") else k) if entry == STEP else (lambda k: k)
        self.outs = {k: _out(T, shapes[k][0], shapes[k][1], rename(k)) for k in keys}
        self.ws = None if workspace is None else guarded.dirty(T, workspace, fill)

    def i(self, key):
        return self.ins[key][1]

    def o(self):
        return {k: v[1] for k, v in self.outs.items()}

    def run(self, fn, launches, what):
        from sslam_amd import lib
        T = self.T
        n0, others = lib.track_launch_count(), _others(lib)
        back = fn()
        T.cuda.synchronize()
        assert lib.track_launch_count() - n0 == launches and _others(lib) == others, f"{what}: {launches} launches, of the ninth library"
        assert all(back[k] is self.outs[k][1] for k in self.keys)
        for k, (whole, mid) in self.outs.items():
            guarded.assert_guards(whole, _raw(T, mid), f"{what} {k}")
            guarded.assert_written(_raw(T, mid), f"{what} {k}")
        for k, (whole, mid) in self.ins.items():
            if mid is not None:
                guarded.assert_guards(whole, _raw(T, mid), f"{what} input {k}")
                _assert_same(mid.cpu().numpy(), np.ascontiguousarray(self.host[k]), f"{what}: input {k} was written")
        return {k: v[1].cpu().numpy() for k, v in self.outs.items()}


def dev_links(T, c, masked=True, what="links"):
    from sslam_amd import lib
    call = Call(T, LINK, dict(pair_first=c["first"], pair_second=c["second"], matches=c["matches"], count=c["count"],
                              mask=c["mask"] if masked else None), lib.link_shapes(c["n_bank"], c["K"]), lib.LINK_KEYS)
    return call.run(lambda: lib.link_pairs(call.i("pair_first"), call.i("pair_second"), call.i("matches"), call.i("count"), c["n_bank"], c["K"],
                                           mask=call.i("mask"), out=call.o()), tt.launches(LINK), what)


def dev_ids(T, links, what="ids", fill=0xA5):
    from sslam_amd import lib
    n_bank, k = links["prev"].shape
    call = Call(T, IDS, dict(prev=links["prev"], prev_frame=links["prev_frame"]), lib.track_id_shapes(n_bank, k), lib.TRACK_ID_KEYS,
                workspace=lib.track_workspace_bytes(n_bank, k), fill=fill)
    return call.run(lambda: lib.track_ids(call.i("prev"), call.i("prev_frame"), out=call.o(), workspace=call.ws), tt.launches(IDS, n_bank), what)


def dev_landmarks(T, s, tr, weight, threshold=3.0, min_obs=2, what="landmarks"):
    from sslam_amd import lib
    n_bank, k = s["depth"].shape
    call = Call(T, LAND, dict(kp_bank=s["kp"], kp_depth_bank=s["depth"], C=s["C"], next=tr["next"], next_frame=tr["next_frame"],
                              root_frame=tr["root_frame"], root_slot=tr["root_slot"], n_tracks=tr["n_tracks"], weight=weight),
                lib.landmark_shapes(n_bank, k), lib.LANDMARK_KEYS)
    return call.run(lambda: lib.landmarks(call.i("kp_bank"), call.i("kp_depth_bank"), call.i("C"), tc.CAMERA, call.i("next"), call.i("next_frame"),
                                          call.i("root_frame"), call.i("root_slot"), call.i("n_tracks"), call.i("weight"), 1.0, 1.0, threshold,
                                          min_obs, out=call.o()), tt.launches(LAND), what)


def _ref_tracks(c, masked=True):
    links = ref.link_pairs(c["first"], c["second"], c["matches"], c["count"], c["mask"] if masked and "mask" in c else None, c["n_bank"], c["K"])
    return links, ref.track_ids(links["prev"], links["prev_frame"])


def _ref_landmarks(s, tr, weight, threshold=3.0, min_obs=2):
    return ref.landmarks(s["kp"], s["depth"], s["C"], tc.CAMERA, tr["next"], tr["next_frame"], tr["root_frame"], tr["root_slot"], tr["n_tracks"],
                         weight, threshold, min_obs)


# ------------------------------------------------------------------------------------------------------------ links and tracks
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", tc.LINK_NAMES + (tc.ONE_TRACK,))
def test_links_and_ids_equal_the_restatement(T, name, masked):
    """tests/test_tracks_cpu.py says what each case plants - 0 to 8 pointer-jumping rounds, K past a wave and past a workgroup, the
    numbering scan at and just past one tile, duplicate and invalid rows, a bridged gap, non-mutual slots, masks, counts and indices
    out of range, one track through 33 frames; here the device gives those bits."""
    c = tc.links(name)
    want_links, want_ids = _ref_tracks(c, masked)
    got = dev_links(T, c, masked, f"{name} links")
    for key in ref.LINK_KEYS:
        _assert_same(got[key], want_links[key], f"{name}: {key}")
    ids = dev_ids(T, got, f"{name} ids")
    for key in ref.TRACK_KEYS:
        _assert_same(ids[key], want_ids[key], f"{name}: {key}")
    if name == "scan_past_1025":                                    # scratch is written before it is read: another fill, the same bits
        again = dev_ids(T, got, f"{name} ids, workspace 0x00", fill=0x00)
        for key in ref.TRACK_KEYS:
            _assert_same(again[key], ids[key], f"{name}: {key} under another workspace fill")


# ------------------------------------------------------------------------------------------------------------------ landmarks
@pytest.fixture(scope="module")
def scene():
    s = tc.scene()
    links, ids = _ref_tracks(s, False)
    return s, {**links, **ids}


@pytest.mark.parametrize("min_obs", [2, 3])
def test_landmarks_equal_the_restatement_on_every_planted_fate(T, scene, min_obs):
    """Zero and -1 depth, a non-finite C row, zero / NaN / infinite / negative / subnormal weights, tracks with 0, 1, min_obs - 1 and
    min_obs kept observations, an outlier the refit drops (tests/test_tracks_cpu.py asserts each fate on the restatement)."""
    s, tr = scene
    got, want = dev_landmarks(T, s, tr, s["weight"], 3.0, min_obs), _ref_landmarks(s, tr, s["weight"], 3.0, min_obs)
    for key in ref.LANDMARK_KEYS:
        _assert_same(got[key], want[key], f"min_obs {min_obs}: {key}")


def test_landmarks_behind_a_camera_the_exact_scene_and_both_invariants(T, scene):
    b = tc.behind_scene()
    tr = {**_ref_tracks(b, False)[0], **_ref_tracks(b, False)[1]}
    got, want = dev_landmarks(T, b, tr, b["weight"], what="behind"), _ref_landmarks(b, tr, b["weight"])
    assert np.isposinf(want["residual"][1, 0]) and want["kept"][1, 0] == 0
    for key in ref.LANDMARK_KEYS:
        _assert_same(got[key], want[key], f"behind: {key}")
    e = tc.exact_scene()
    tr = {**_ref_tracks(e, False)[0], **_ref_tracks(e, False)[1]}
    got, want = dev_landmarks(T, e, tr, None, what="exact"), _ref_landmarks(e, tr, None)
    for key in ref.LANDMARK_KEYS:
        _assert_same(got[key], want[key], f"exact: {key}")
    ids = tr["track_id"][0, e["perm"][0]]
    assert np.abs(got["xyz"][ids] - e["Pw"]).max() < 1e-15
    # weight = NULL against a bank of exactly 1.0f: byte-identical
    s, tr = scene
    null, ones = dev_landmarks(T, s, tr, None, what="NULL"), dev_landmarks(T, s, tr, np.ones_like(s["weight"]), what="ones")
    for key in ref.LANDMARK_KEYS:
        _assert_same(null[key], ones[key], f"NULL against 1.0f: {key}")
        _assert_same(null[key], _ref_landmarks(s, tr, None)[key], f"NULL against the restatement: {key}")
    # every weight scaled by a power of two: weight_sum scaled exactly, every other output's bytes (the subnormal weight is left out
    # of the scaling - it would underflow - and so is its track of the comparison)
    base = dev_landmarks(T, s, tr, s["weight"], what="base")
    small = np.abs(s["weight"]) < 1e-30
    sub = int(tr["track_id"][0, s["perm"][0, s["planted"]["weights"]]])
    rows = np.arange(len(base["weight_sum"])) != sub
    members = tr["track_id"] != sub
    for scale in (2.0 ** -20, 2.0 ** 30):
        w = (s["weight"] * np.float32(scale)).astype(np.float32)
        w[small] = s["weight"][small]
        scaled = dev_landmarks(T, s, tr, w, what=f"scaled {scale}")
        _assert_same(scaled["weight_sum"][rows], base["weight_sum"][rows] * scale, f"weight_sum scaled by {scale}")
        for key in ("xyz", "n_obs", "n_kept", "status", "rms"):
            _assert_same(scaled[key][rows], base[key][rows], f"{key} under weights scaled by {scale}")
        for key in ("residual", "kept"):
            _assert_same(scaled[key][members], base[key][members], f"{key} under weights scaled by {scale}")


# ---------------------------------------------------------------------------------------------------------------------- online
class Bank:
    """One track bank on the device: state, the step's inputs and outputs each in a poisoned guarded buffer, the state made fresh
    (the counters 0; everything else stays poison: nothing of it is read before it is written)."""

    def __init__(self, T, capacity, k, n1, masked=True):
        from sslam_amd import lib
        self.T, self.lib, self.cap, self.k, self.masked = T, lib, capacity, k, masked
        self.state = {key: _out(T, shape, dt, key) for key, (shape, dt) in lib.track_state_shapes(capacity, k).items()}
        self.state["t"][1].zero_(), self.state["next_id"][1].zero_()
        self.ins = dict(matches=_out(T, (1, n1, 2), T.int64, "matches"), count=_out(T, (1,), T.int32, "count"),
                        first=_out(T, (1,), T.int32, "first"))
        if masked:
            self.ins["mask"] = _out(T, (1, n1), T.int32, "mask")
        self.outs = {key: _out(T, shape, dt, "out_" + key if key in ("track_id", "age") else key) for key, (shape, dt) in lib.track_out_shapes(k).items()}

    def pairs(self):
        return list(self.state.items()) + list(self.ins.items()) + list(self.outs.items())

    def state_np(self):
        return {k: v[1].cpu().numpy() for k, v in self.state.items()}

    def load(self, matches, count, mask, first):
        T = self.T
        self.ins["matches"][1].copy_(T.from_numpy(np.ascontiguousarray(matches))[None])
        self.ins["count"][1].fill_(int(count)), self.ins["first"][1].fill_(int(first))
        if self.masked:
            self.ins["mask"][1].copy_(T.from_numpy(np.ascontiguousarray(mask))[None])

    def call(self):
        return self.lib.track_step({k: v[1] for k, v in self.state.items()}, self.ins["matches"][1], self.ins["count"][1], self.ins["first"][1],
                                   mask=self.ins["mask"][1] if self.masked else None, out={k: v[1] for k, v in self.outs.items()})

    def step(self, matches, count, mask, first, what, call=None):
        """One guarded step -> (outputs, state before, state after) as dicts of numpy arrays."""
        T, lib = self.T, self.lib
        self.load(matches, count, mask, first)
        for whole, mid in self.outs.values():
            _poison(T, mid)
        before = self.state_np()
        n0, others = lib.track_launch_count(), _others(lib)
        (call or self.call)()
        T.cuda.synchronize()
        assert lib.track_launch_count() - n0 == (1 if call is None else 0) and _others(lib) == others, "one launch, of the ninth library"
        for name, (whole, mid) in self.pairs():
            guarded.assert_guards(whole, _raw(T, mid), f"{what} {name}")
        for k, (whole, mid) in self.outs.items():
            guarded.assert_written(mid, f"{what} {k}")
        return {k: v[1].cpu().numpy() for k, v in self.outs.items()}, before, self.state_np()


def _prefix_on_device(T, lib, c, rows):
    """sslt_link_pairs + sslt_track_ids on the device over the rows (first, second, case row) stepped so far."""
    first, second = (T.tensor([r[i] for r in rows], dtype=T.int32, device="cuda") for i in (0, 1))
    idx = [r[2] for r in rows]
    dev = lambda a: T.from_numpy(np.ascontiguousarray(a[idx])).cuda()
    links = lib.link_pairs(first, second, dev(c["matches"]), dev(c["count"]), len(rows), c["K"], mask=dev(c["mask"]))
    return {k: v.cpu().numpy() for k, v in {**links, **lib.track_ids(links["prev"], links["prev_frame"])}.items()}


def run_bank(T, c, steps, what, dev=None, device_prefix=True, call_of=None):
    from sslam_amd import lib
    cap, k = len(steps), c["K"]
    dev = Bank(T, cap, k, c["matches"].shape[1]) if dev is None else dev
    host = ref.TrackBank(cap, k)
    call = None if call_of is None else call_of(dev)
    rows = []
    for t, (a, p) in enumerate(steps + [(0, 0), (1, 0)]):          # and two steps past capacity
        p_ = 0 if p is None else p
        got, before, after = dev.step(c["matches"][p_], c["count"][p_], c["mask"][p_], a, f"{what} step {t}", call)
        want = host.step(c["matches"][p_], c["count"][p_], c["mask"][p_], a)
        for key in ref.BANK_OUT_KEYS:
            _assert_same(got[key], want[key], f"{what} step {t}: {key} against the restatement")
        if t >= cap:                                                # the bank is full: status 4, the state's bytes untouched
            assert got["status"].tolist() == [4] and (got["track_id"] == -1).all() and got["n_new"].tolist() == [0]
            for key in ref.BANK_STATE_KEYS:
                _assert_same(after[key], before[key], f"{what} step {t}: state {key} past capacity")
            continue
        rows.append((a, t, p_))
        n = t + 1
        assert after["t"].tolist() == [n] and after["next_id"].tolist() == host.state["next_id"].tolist()
        for key in ref.LINK_KEYS + ("track_id", "age"):
            _assert_same(after[key][:n], host.state[key][:n], f"{what} step {t}: state {key} against the restatement")
            later = np.ones(cap, bool)
            later[:n] = False
            _assert_same(after[key][later], before[key][later], f"{what} step {t}: state {key} past row {t}")
        if device_prefix:
            batch = _prefix_on_device(T, lib, c, rows)
            for key in ref.LINK_KEYS + ("track_id", "age"):
                _assert_same(after[key][:n], batch[key], f"{what} step {t}: state {key} against the batch entries on the prefix")
            assert batch["n_tracks"].tolist() == after["next_id"].tolist()
            st = {key: dev.state[key][1][:n] for key in ("prev", "prev_frame")}      # the stored links reproduce the stored ids
            again = lib.track_ids(st["prev"], st["prev_frame"])
            _assert_same(again["track_id"].cpu().numpy(), after["track_id"][:n], f"{what} step {t}: track_ids over the stored prev bank")
    return dev


def _steps_12(c):
    """The 12-frame scene's rows (t - 1, t), but frame 6 is dropped: step 6 names no frame and step 7 bridges it from frame 5."""
    steps = [(-1, None)] + [(t - 1, t - 1) for t in range(1, 12)]
    steps[6], steps[7] = (-1, None), (5, 6)
    return steps


@pytest.fixture(scope="module")
def scene12():
    s = tc.scene(3, 12, 70, dirty=False)
    mask = np.ones(s["matches"].shape[:2], np.int32)
    mask[:, ::7], mask[:, 3::11] = 0, -1
    return dict(s, mask=mask)


def test_track_step_over_12_frames_equals_the_batch_entries_on_every_prefix(T, scene12):
    run_bank(T, scene12, _steps_12(scene12), "12 frames")


def test_track_step_on_the_row_and_slot_rules(T):
    c = tc.links("row_rules")
    steps = tc.steps_of("row_rules")
    steps[5] = (3, 3)                                               # frames 4 and 5 both name frame 3 first: only the earlier step links
    run_bank(T, c, steps, "row rules")
    c = tc.links("n9_k257")                                         # K past a workgroup: the new ids' scan carries over two chunks
    run_bank(T, c, tc.steps_of("n9_k257"), "K 257", device_prefix=False)


@pytest.mark.parametrize("t", [-1, 12, 2 ** 31 - 1])
def test_a_counter_out_of_range_answers_4_and_leaves_the_state_alone(T, scene12, t):
    dev = Bank(T, 12, 70, 70)
    dev.state["t"][1].fill_(t)
    got, before, after = dev.step(scene12["matches"][0], scene12["count"][0], scene12["mask"][0], 0, f"counter {t}")
    assert got["status"].tolist() == [4] and (got["track_id"] == -1).all() and (got["age"] == -1).all() and got["n_new"].tolist() == [0]
    for key in ref.BANK_STATE_KEYS:                                 # everything but the counters still holds its poison
        _assert_same(after[key], before[key], f"state {key}")
    assert after["t"].tolist() == [t]


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


def test_track_step_replayed_from_a_captured_graph(T, scene12):
    """No host value enters the step: one captured launch, replayed for every frame, gives the restatement's bits."""
    def call_of(dev):
        dev.load(scene12["matches"][0], 0, scene12["mask"][0], -1)
        g = _capture(T, dev.call)
        dev.state["t"][1].zero_(), dev.state["next_id"][1].zero_()  # the warm-up and the capture's launch stepped the bank
        return g.replay
    run_bank(T, scene12, _steps_12(scene12), "captured", device_prefix=False, call_of=call_of)


# ------------------------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("mode", ["lo", "hi"])
def test_every_pointer_at_its_least_alignment(T, scene, scene12, mode):
    """Each operand of the four entries at the alignment include/sslam_track.h states and no better, just past and just before a
    256-byte boundary: the same bits as the restatement."""
    def placed(entry, make):
        with guarded.placed(guarded.Placement(tt.ALIGN[entry], mode)) as p:
            got = make()
        assert sorted(r["name"] for r in p.made) == sorted(tt.ALIGN[entry]), entry
        for r in p.made:
            assert r["middle"].data_ptr() % 256 == (r["align"] if mode == "lo" else 256 - r["align"]), (entry, r["name"])
        return got
    c = tc.links("n5_k70")
    want_links, want_ids = _ref_tracks(c)
    links = placed(LINK, lambda: dev_links(T, c, True, f"links {mode}"))
    ids = placed(IDS, lambda: dev_ids(T, links, f"ids {mode}"))
    for key in ref.LINK_KEYS:
        _assert_same(links[key], want_links[key], f"{mode}: {key}")
    for key in ref.TRACK_KEYS:
        _assert_same(ids[key], want_ids[key], f"{mode}: {key}")
    s, tr = scene
    lm, want = placed(LAND, lambda: dev_landmarks(T, s, tr, s["weight"], what=f"landmarks {mode}")), _ref_landmarks(s, tr, s["weight"])
    for key in ref.LANDMARK_KEYS:
        _assert_same(lm[key], want[key], f"{mode}: {key}")
    bank = placed(STEP, lambda: Bank(T, 12, 70, 70))
    run_bank(T, scene12, _steps_12(scene12), f"step {mode}", dev=bank, device_prefix=False)


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_launches_nothing_and_writes_nothing(T, scene):
    """Each entry with real poisoned outputs: one past each size limit, a size of zero, a pointer one word off its alignment and a
    NULL pointer - the code, no launch, every output still poison.  The limits are run by refusal alone: no large allocation."""
    from sslam_amd import lib
    L = lib.track()
    s, tr = scene
    n_bank, k = s["depth"].shape
    stream = ctypes.c_void_p(T.cuda.current_stream().cuda_stream)
    d = lambda t: ctypes.c_void_p(t.data_ptr())
    dd = ctypes.c_double

    def refused(entry, outs, args_of, cases):
        for what, over, code in cases:
            n0 = lib.track_launch_count()
            assert getattr(L, entry)(*args_of(**over), stream) == code, (entry, what)
            T.cuda.synchronize()
            assert lib.track_launch_count() == n0, (entry, what, "launched")
            for key, (whole, mid) in outs.items():
                raw = _raw(T, mid)
                assert bool((raw == guarded._int_view(T, raw.dtype)[1]).all()), (entry, what, key, "written")

    ins = {key: T.from_numpy(np.ascontiguousarray(v)).cuda() for key, v in dict(
        first=s["first"], second=s["second"], matches=s["matches"], count=s["count"], kp=s["kp"], depth=s["depth"], C=s["C"], next=tr["next"],
        next_frame=tr["next_frame"], root_frame=tr["root_frame"], root_slot=tr["root_slot"], n_tracks=tr["n_tracks"], prev=tr["prev"],
        prev_frame=tr["prev_frame"]).items()}
    P, n1 = s["matches"].shape[:2]
    limits = [("one past the node limit", dict(n_bank=2 ** 28, K=8), -2), ("far past it", dict(n_bank=2 ** 31 - 1, K=2), -2), ("n_bank 0", dict(n_bank=0), -1),
              ("K 0", dict(K=0), -1)]
    # links
    outs = {key: _out(T, shape, dt, key) for key, (shape, dt) in lib.link_shapes(n_bank, k).items()}
    def link_args(n_bank=n_bank, K=k, n_pairs=P, off=0, null=False):
        o = [d(outs[key][1]) for key in lib.LINK_KEYS]
        o[0] = ctypes.c_void_p(0 if null else o[0].value + off)
        return [d(ins["first"]), d(ins["second"]), n_pairs, d(ins["matches"]), d(ins["count"]), None, n1, n_bank, K] + o
    refused(LINK, outs, link_args, limits + [("K past SSLT_MAX_K", dict(K=tt.MAX_K + 1, n_bank=1), -2), ("no pairs", dict(n_pairs=0), -1),
                                             ("prev misaligned", dict(off=2), -1), ("prev NULL", dict(null=True), -1)])
    # ids
    outs = {key: _out(T, shape, dt, key) for key, (shape, dt) in lib.track_id_shapes(n_bank, k).items()}
    ws = guarded.guarded(T, lib.track_workspace_bytes(n_bank, k), T.uint8)
    outs["workspace"] = ws
    def ids_args(n_bank=n_bank, K=k, off=0, null=False):
        o = [d(outs[key][1]) for key in lib.TRACK_ID_KEYS]
        return [d(ins["prev"]), d(ins["prev_frame"]), n_bank, K, ctypes.c_void_p(0 if null else ws[1].data_ptr() + off)] + o
    refused(IDS, outs, ids_args, limits + [("workspace at 4 bytes", dict(off=4), -1), ("workspace NULL", dict(null=True), -1)])
    # landmarks
    outs = {key: _out(T, shape, dt, key) for key, (shape, dt) in lib.landmark_shapes(n_bank, k).items()}
    def land_args(n_bank=n_bank, K=k, off=0, null=False, min_obs=2, threshold=3.0, fx=525.0):
        o = [d(outs[key][1]) for key in lib.LANDMARK_KEYS]
        o[0] = ctypes.c_void_p(0 if null else o[0].value + off)
        cam = [dd(fx), dd(525.0), dd(319.5), dd(239.5), dd(5000.0), dd(1.0), dd(1.0), dd(640.0), dd(480.0), dd(threshold)]
        return [d(ins["kp"]), d(ins["depth"]), d(ins["C"]), n_bank, K] + cam + [d(ins[key]) for key in ("next", "next_frame", "root_frame", "root_slot", "n_tracks")] + \
            [None, min_obs] + o
    refused(LAND, outs, land_args, limits + [("min_obs 1", dict(min_obs=1), -1), ("threshold NaN", dict(threshold=float("nan")), -1),
                                             ("fx 0", dict(fx=0.0), -1), ("xyz at 4 bytes", dict(off=4), -1), ("xyz NULL", dict(null=True), -1)])
    # the step: the state is an output too
    bank = Bank(T, 4, k, n1, masked=False)
    bank.load(s["matches"][0], s["count"][0], None, -1)
    for key in ("t", "next_id"):
        _poison(T, bank.state[key][1])
    outs = dict(list(bank.state.items()) + list(bank.outs.items()))
    def step_args(n_bank=4, K=k, off=0, null=False):
        st = [d(bank.state[key][1]) for key in lib.TRACK_STATE_KEYS]
        st[0] = ctypes.c_void_p(0 if null else st[0].value + off)
        return st + [d(bank.ins["matches"][1]), d(bank.ins["count"][1]), None, d(bank.ins["first"][1]), n1, K, n_bank] + \
            [d(bank.outs[key][1]) for key in lib.TRACK_OUT_KEYS]
    refused(STEP, outs, step_args, limits + [("K past SSLT_MAX_K", dict(K=tt.MAX_K + 1, n_bank=1), -2), ("t misaligned", dict(off=2), -1),
                                             ("t NULL", dict(null=True), -1)])


# ---------------------------------------------------------------------------------------------------------------------- layers
E2E_THRESHOLD, E2E_HYP, E2E_SEED, E2E_HUBER, E2E_ITER, E2E_MIN_INLIERS = 12.0, 64, 5, 4.0, 5, 4      # tests/test_gpu_window.py's choices
E2E_FRAMES, E2E_SPACINGS, E2E_WINDOW = 8, (1, 2, 3), 4


@pytest.fixture(scope="module")
def seq(T):
    import pose_depth_cases
    import pose_eval_ref as pr
    from sslam_amd import evaluation as ev
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K), inp["selector"], inp["refiner"], device="cuda")
    n = E2E_FRAMES
    return dict(pipe=pipe, toks=T.from_numpy(inp["tokens"]).cuda()[:n], depth_np=pose_depth_cases.sequence_depth()[:n],
                depth=T.from_numpy(pose_depth_cases.sequence_depth()[:n]).cuda(), cam=ev.Camera(), K=pr.SEQ_K)


def test_the_pipeline_methods_equal_the_restatement(T, seq, scene12):
    from sslam_amd import lib
    pipe, c = seq["pipe"], scene12
    dev = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    mm = dict(matches=dev(c["matches"]), match_count=dev(c["count"]))
    links = pipe.link_matches(c["first"].tolist(), c["second"].tolist(), mm, mask=dict(inlier_of_slot=dev(c["mask"])), n_frames=12, k=70)
    tr = pipe.track_ids(links)
    want = {**_ref_tracks(c)[0], **_ref_tracks(c)[1]}
    assert set(tr) == set(lib.LINK_KEYS) | set(lib.TRACK_ID_KEYS)
    for key in want:
        _assert_same(tr[key].cpu().numpy(), want[key], f"pipeline: {key}")
    cam = tc.CAMERA                                                 # the pipeline's depth scales: camera pixels per keypoint unit
    sx, sy = pipe.depth_scales(cam)
    lm = pipe.landmarks(dev(c["kp"]), dev(c["depth"]), dev(c["C"]), tr, cam, threshold=2.0, min_obs=3, weights=dev(c["weight"]))
    wl = ref.landmarks(c["kp"], c["depth"], c["C"], cam, want["next"], want["next_frame"], want["root_frame"], want["root_slot"], want["n_tracks"],
                       c["weight"], 2.0, 3, sx, sy)
    for key in ref.LANDMARK_KEYS:
        _assert_same(lm[key].cpu().numpy(), wl[key], f"pipeline: {key}")
    bank = pipe.alloc_track_bank(12, 70)
    first = T.full((1,), -1, dtype=T.int32, device="cuda")
    for t in range(12):
        first.fill_(t - 1)
        out = pipe.track_step(bank, mm, first, mask=dev(c["mask"]), row=max(t - 1, 0))
        assert out["track_id"] is bank["out"]["track_id"]
        _assert_same(out["track_id"].cpu().numpy(), want["track_id"][t], f"pipeline step {t}: track_id")
    _assert_same(bank["state"]["age"].cpu().numpy(), want["age"], "pipeline: the bank's ages")
    with pytest.raises(ValueError, match="n_frames"):
        pipe.link_matches(c["first"].tolist(), c["second"].tolist(), mm)


@pytest.fixture(scope="module")
def seq_conf(T, seq):
    """The same frames on a pipeline that extracts the keypoint confidence: what weights= and the weighted map need."""
    import confidence_cases
    import pose_eval_ref as pr
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K, confidence=True), inp["selector"], inp["refiner"],
                            device="cuda", confidence_state=confidence_cases.head_state("x4"))
    return dict(seq, pipe=pipe)


def _same_nested(a, b, at):
    assert type(a) is type(b), at
    if isinstance(a, dict):
        assert set(a) == set(b), at
        for key in a:
            _same_nested(a[key], b[key], f"{at}.{key}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), at
    else:
        assert a == b or (a != a and b != b), at


def _separate_calls(s, weights, threshold, min_obs, graph_iterations, weighted_map=True):
    """What odometry_graph(tracks=...) does, call by call: the refined rows, the graph's C ON THE DEVICE (odometry._graph_device, the
    function odometry_graph itself runs: the same bits, no inverse of an inverse), links, ids, landmarks -> host arrays."""
    from sslam_amd import evaluation as ev
    from sslam_amd import odometry
    from sslam_amd.pipeline import MatchRule
    pipe, n, K = s["pipe"], E2E_FRAMES, s["K"]
    ex = pipe.extract(s["toks"], None)
    kp = pipe.geometry_keypoints(ex)
    kd = ev.gather_keypoint_depth(pipe, s["depth_np"], kp, n)
    lists = {sp: [(i, i + sp) for i in range(n - sp)] for sp in E2E_SPACINGS}
    pairs = [pr for sp in lists for pr in lists[sp]]
    first, second = [a for a, _ in pairs], [b for _, b in pairs]
    mm = pipe.match_pairs(ex["descriptors"], ex["scores"], first=first, second=second, rule=MatchRule.mnn_ratio(0.9))
    w = None if weights is None else pipe.match_weights(ex["confidence"], first, second, mm, weights)
    est = pipe.estimate_poses(kp, kd, first, second, mm, s["cam"], E2E_THRESHOLD, E2E_HYP, E2E_SEED)
    refined = pipe.refine_poses(kp, kd, first, second, mm, s["cam"], est, E2E_THRESHOLD, E2E_HUBER, E2E_ITER, weights=w)
    g = odometry._graph_device(pipe, refined, pairs, lists, n, None, max(E2E_SPACINGS), 4.0, 0.0, graph_iterations)
    rows = slice(0, n - 1)                                          # the spacing-1 rows stand first
    links = pipe.link_matches(first[rows], second[rows], {k: mm[k][rows] for k in ("matches", "match_count")}, mask=refined["inlier_of_slot"][rows],
                              n_frames=n, k=K)
    tr = pipe.track_ids(links)
    lm = pipe.landmarks(kp, kd, g["C"].reshape(n, 12), tr, s["cam"], threshold, min_obs,
                        weights=ex["confidence"] if weights is not None and weighted_map else None)
    host = {k: v.cpu().numpy() for k, v in {**tr, **lm}.items()}
    host["mask_links"] = int((refined["inlier_of_slot"][rows] == 1).sum().cpu())
    return host


def test_odometry_graph_with_tracks_equals_the_separate_calls(T, seq_conf):
    """'tracks' of odometry_graph against link_matches + track_ids + landmarks under the graph's own C, byte for byte - every column of
    the read-back: n_tracks, track_id, the length statistics, landmarks, status, n_kept, rms - for tracks=True, for a dictionary, and
    with weights=, where the keypoint confidences weight the map; the other keys equal odometry_graph()'s bytes."""
    from sslam_amd import lib, odometry
    from sslam_amd import track_numpy as tn
    from sslam_amd.pipeline import PoseWeights
    s = seq_conf
    pipe, n, K = s["pipe"], E2E_FRAMES, s["K"]
    kw = dict(depth=s["depth_np"], camera=s["cam"], spacings=E2E_SPACINGS, threshold=E2E_THRESHOLD, hypotheses=E2E_HYP, seed=E2E_SEED,
              tokens=s["toks"], huber=E2E_HUBER, iterations=E2E_ITER, graph_iterations=4)
    pw = PoseWeights.expected_error(0.5)
    assert odometry.check_tracks(None) is None and odometry.check_tracks(True) == odometry.TRACK_DEFAULTS == dict(threshold=3.0, min_obs=2)
    assert odometry.check_tracks(dict(min_obs=3)) == dict(threshold=3.0, min_obs=3)
    each = tt.launches(LINK) + tt.launches(IDS, n) + tt.launches(LAND)
    kept_any = False
    for what, weights, tracks, threshold, min_obs in (("tracks=True", None, True, 3.0, 2),
                                                      ("a dictionary", None, dict(threshold=E2E_THRESHOLD, min_obs=3), E2E_THRESHOLD, 3),
                                                      ("weights= and tracks=", pw, dict(threshold=E2E_THRESHOLD), E2E_THRESHOLD, 2)):
        wkw = {} if weights is None else dict(weights=weights)
        n0 = lib.track_launch_count()
        plain = odometry.odometry_graph(pipe, **kw, **wkw)
        assert lib.track_launch_count() == n0 and "tracks" not in plain, "tracks=None launches nothing from the ninth library"
        full = odometry.odometry_graph(pipe, tracks=tracks, **kw, **wkw)
        assert lib.track_launch_count() - n0 == each, what
        _same_nested({k: v for k, v in full.items() if k != "tracks"}, plain, f"{what}: odometry_graph")
        want = _separate_calls(s, weights, threshold, min_obs, 4)
        tk, nt = full["tracks"], int(want["n_tracks"][0])
        assert set(tk) == {"n_tracks", "length", "landmarks", "status", "n_kept", "rms", "track_id"} and tk["n_tracks"] == nt, what
        stats = tn.length_statistics(want["length"], [nt])
        del stats["n_tracks"]
        _same_nested(tk["length"], stats, f"{what}: length")
        for key, col in (("track_id", want["track_id"]), ("landmarks", want["xyz"][:nt]), ("status", want["status"][:nt]),
                         ("n_kept", want["n_kept"][:nt]), ("rms", want["rms"][:nt])):
            _assert_same(tk[key], col, f"{what}: {key}")
        assert want["mask_links"] > 0 and tk["length"]["max"] >= 2, "the synthetic sequence has refined inliers to link"
        kept_any = kept_any or bool((tk["status"] == 0).any())
        if weights is not None:                                     # the confidences reached the map: the same tracks under weight 1 differ
            uniform = _separate_calls(s, weights, threshold, min_obs, 4, weighted_map=False)
            assert uniform["track_id"].tobytes() == want["track_id"].tobytes() and (uniform["xyz"][:nt] != tk["landmarks"]).any()
    assert kept_any, "the synthetic sequence has tracks whose observations agree at the pose stage's threshold"
    with pytest.raises(ValueError, match="tracks must be"):
        odometry.odometry_graph(pipe, tracks=dict(window=3), **kw)
    with pytest.raises(ValueError, match="tracks must be"):
        odometry.odometry_graph(pipe, tracks=False, **kw)
    with pytest.raises(ValueError, match="min_obs"):
        odometry.odometry_graph(pipe, tracks=dict(min_obs=1), **kw)


def test_track_window_stepper_shares_the_window_steppers_bytes_and_equals_the_batch_entries(T, seq):
    from sslam_amd import lib
    from sslam_amd.online import TrackWindowPoseFrameStepper, WindowPoseFrameStepper
    kw = dict(camera=seq["cam"], tokens_in=True, spacings=E2E_SPACINGS, window=E2E_WINDOW, threshold=E2E_THRESHOLD, hypotheses=E2E_HYP,
              seed=E2E_SEED, huber=E2E_HUBER, iterations=E2E_ITER, min_inliers=E2E_MIN_INLIERS, capacity=6)
    image = T.zeros((48, 64, 3), dtype=T.uint8, device="cuda")
    host = lambda d: {k: (host(v) if isinstance(v, dict) else (v.cpu().numpy().copy() if isinstance(v, T.Tensor) else v)) for k, v in d.items()}
    runs = {}
    for name, cls, use_graph in (("window", WindowPoseFrameStepper, True), ("track", TrackWindowPoseFrameStepper, True),
                                 ("track_launches", TrackWindowPoseFrameStepper, False)):
        st = cls(seq["pipe"], 48, 64, 480, 640, use_graph=use_graph, **kw)
        runs[name] = [host(st.step(image, seq["depth"][i], seq["toks"][i])) for i in range(E2E_FRAMES)], st
    new = {"track_id", "track_age", "n_new", "track_status"}

    def same(a, b, at):
        if isinstance(a, dict):
            assert set(a) == set(b), at
            for key in a:
                same(a[key], b[key], f"{at}.{key}")
        elif isinstance(a, np.ndarray):
            assert a.tobytes() == b.tobytes(), at
        else:
            assert a == b, at
    for i in range(E2E_FRAMES):
        got = runs["track"][0][i]
        assert set(got) - set(runs["window"][0][i]) == new
        same({k: v for k, v in got.items() if k not in new}, runs["window"][0][i], f"frame {i}: the shared outputs")
        same(got, runs["track_launches"][0][i], f"frame {i}: graph against launches")
    # the bank against the batch entries over the same rows: the step's own spacing-1 match lists and refined masks
    st = runs["track"][1]
    cap, K = 6, seq["K"]
    state = {k: v.cpu().numpy() for k, v in st.tracks["state"].items()}
    assert state["t"].tolist() == [cap], "two of the eight frames were stepped past the bank"
    m = np.stack([runs["track"][0][i]["matches"][0] for i in range(1, cap)])
    cnt = np.array([runs["track"][0][i]["match_count"][0] for i in range(1, cap)], np.int32)
    mask = np.stack([runs["track"][0][i]["pose"]["refined"]["inlier_of_slot"][0] for i in range(1, cap)])
    want_links = ref.link_pairs(np.arange(cap - 1, dtype=np.int32), np.arange(1, cap, dtype=np.int32), m, cnt, mask, cap, K)
    want_ids = ref.track_ids(want_links["prev"], want_links["prev_frame"])
    for key in ref.LINK_KEYS:
        _assert_same(state[key], want_links[key], f"stepper: state {key}")
    for key in ("track_id", "age"):
        _assert_same(state[key], want_ids[key], f"stepper: state {key}")
    for i in range(E2E_FRAMES):
        got = runs["track"][0][i]
        if i < cap:
            _assert_same(got["track_id"], want_ids["track_id"][i], f"frame {i}: track_id")
            _assert_same(got["track_age"], want_ids["age"][i], f"frame {i}: track_age")
            assert got["track_status"].tolist() == [0] and got["n_new"][0] == (want_ids["age"][i] == 0).sum()
        else:
            assert got["track_status"].tolist() == [4] and (got["track_id"] == -1).all()
    assert (want_ids["age"] > 0).any(), "the synthetic sequence has refined inliers to link"
    # landmarks(): outside the captured step, one read-back, no state changed
    before = {k: v.clone() for k, v in st.tracks["state"].items()}
    n0 = lib.track_launch_count()
    lm = st.landmarks(threshold=E2E_THRESHOLD)
    assert lib.track_launch_count() - n0 == tt.launches(IDS, cap) + tt.launches(LAND)
    assert all(T.equal(before[k], v) for k, v in st.tracks["state"].items())
    nt = int(want_ids["n_tracks"][0])
    assert lm["n_tracks"] == nt and lm["track_id"].tobytes() == want_ids["track_id"].tobytes() and lm["age"].tobytes() == want_ids["age"].tobytes()
    assert lm["length"].tobytes() == want_ids["length"][:nt].tobytes()
    C = st.win["state"]["trajectory"][0, :cap].cpu().numpy()
    kp, kd = st.track_kp[:cap].cpu().numpy(), st.track_depth[:cap].cpu().numpy()
    sx, sy = seq["pipe"].depth_scales(seq["cam"])
    wl = ref.landmarks(kp, kd, C, seq["cam"], want_links["next"], want_links["next_frame"], want_ids["root_frame"], want_ids["root_slot"],
                       want_ids["n_tracks"], None, E2E_THRESHOLD, 2, sx, sy)
    _assert_same(lm["landmarks"], wl["xyz"][:nt], "stepper: landmarks")
    _assert_same(lm["status"], wl["status"][:nt], "stepper: status")
    _assert_same(lm["n_kept"], wl["n_kept"][:nt], "stepper: n_kept")
    _assert_same(lm["rms"], wl["rms"][:nt], "stepper: rms")
    st.reset()
    again = host(st.step(image, seq["depth"][0], seq["toks"][0]))
    same(again, runs["track"][0][0], "after reset, frame 0")
    with pytest.raises(ValueError, match="spacings must hold 1"):
        TrackWindowPoseFrameStepper(seq["pipe"], 48, 64, 480, 640, **dict(kw, spacings=(2, 3)))
