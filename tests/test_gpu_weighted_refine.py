"""GPU tests of confidence-weighted pose refinement: sslu_match_weights and sslu_pose_refine_weighted_pairs through sslam_amd.lib,
SequencePipeline.match_weights / refine_poses(weights=), sslam_amd.odometry(weights=), odometry_graph(weights=),
online.PoseFrameStepper(weights=) (the drop-ins need no GPU: tests/test_weighted_refine_cpu.py).

Reference: the float64 restatement of tests/weighted_refine_ref.py on the seeded cases of tests/weighted_refine_cases.py, which
tests/test_weighted_refine_cpu.py holds to their margins, to an independent implementation and to the header's two invariants.
EVERY output is compared bit for bit, as bytes.  Every launch goes into poisoned outputs between guard bands (tests/guarded.py)
with the inputs between NaN bands; inputs are compared with their host copies after the call; launches are counted."""
import ctypes as C

import numpy as np
import pytest

import guarded
import pose_refine_cases as pc
import weight_table as wt
import weighted_refine_cases as cases
import weighted_refine_ref as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev(T, a):
    return None if a is None else T.from_numpy(np.ascontiguousarray(a)).cuda()


def _outputs(T, n_pairs, n1):
    """Poisoned outputs between guard bands: {key: (whole, middle, tensor handed to the entry)}; float64 lies in an int64 layout."""
    from sslam_amd import lib
    shapes, out = lib.pose_refine_weighted_shapes(n_pairs, n1), {}
    for key in lib.POSE_REFINE_WEIGHTED_KEYS:
        shape, dt = shapes[key]
        whole, mid = guarded.guarded(T, shape, T.int64 if dt == T.float64 else dt, name=key)
        out[key] = (whole, mid, mid.view(T.float64) if dt == T.float64 else mid)
    return out


INPUTS = ("bank", "depth_bank", "first", "second", "matches", "count")
ARG = dict(bank="kp_bank", depth_bank="kp_depth_bank", first="pair_first", second="pair_second", matches="matches", count="count")


def run_case(T, c, weight, **override):
    """sslu_pose_refine_weighted_pairs on a case, one launch into poisoned, guarded outputs -> dict of numpy arrays."""
    from sslam_amd import lib
    a = dict(threshold=c["threshold"], huber=c["huber"], n_iter=c["n_iter"], T_in=c["T_in"])
    a.update(override)
    ins = {key: guarded.guarded_input(T, c[key], name=ARG[key]) for key in INPUTS}
    ins["T_in"] = guarded.guarded_input(T, np.ascontiguousarray(a["T_in"]).view(np.int64), name="T_in")      # float64 bits, NaN among them
    ins["weight"] = guarded.guarded_input(T, np.ascontiguousarray(weight).view(np.int32), name="weight")      # fp32 bits, NaN among them
    out = _outputs(T, len(c["first"]), c["n1"])
    n0, m0 = lib.weight_launch_count(), lib.launch_count()
    lib.pose_refine_weighted(*(ins[key][1] for key in INPUTS), c["cam"], ins["T_in"][1].view(T.float64), ins["weight"][1].view(T.float32),
                             c["scale_x"], c["scale_y"], a["threshold"], a["huber"], a["n_iter"],
                             out=tuple(out[key][2] for key in lib.POSE_REFINE_WEIGHTED_KEYS))
    assert lib.weight_launch_count() - n0 == 1 and lib.launch_count() == m0, "one launch, of this library"
    got = {}
    for key, (whole, mid, t) in out.items():
        guarded.assert_guards(whole, mid, f"pose_refine_weighted {key}")
        guarded.assert_written(mid, f"pose_refine_weighted {key}")
        got[key] = t.cpu().numpy()
    for key, (whole, mid) in ins.items():
        guarded.assert_guards(whole, mid, f"input {key}")
        want = np.ascontiguousarray(a["T_in"]).view(np.int64) if key == "T_in" else np.ascontiguousarray(weight).view(np.int32) if key == "weight" else c[key]
        assert np.array_equal(mid.cpu().numpy(), want), f"input {key} was written"
    return got


def run_weights(T, s, mode, sigma0):
    """sslu_match_weights on a weight_case, one launch into a poisoned, guarded output -> (P, n1) fp32 numpy."""
    from sslam_amd import lib
    names = dict(conf="conf_bank", first="pair_first", second="pair_second", matches="matches", count="count")
    ins = {key: guarded.guarded_input(T, s[key].view(np.int32) if key == "conf" else s[key], name=names[key]) for key in names}
    whole, mid = guarded.guarded(T, s["matches"].shape[:2], T.float32, name="weight")
    n0 = lib.weight_launch_count()
    lib.match_weights(ins["conf"][1].view(T.float32), ins["first"][1], ins["second"][1], ins["matches"][1], ins["count"][1], mode, sigma0, out=mid)
    assert lib.weight_launch_count() - n0 == 1, "one launch"
    guarded.assert_guards(whole, mid, "match_weights weight")
    guarded.assert_written(mid, "match_weights weight")
    for key, (w, m) in ins.items():
        guarded.assert_guards(w, m, f"input {key}")
        assert np.array_equal(m.cpu().numpy(), s[key].view(np.int32) if key == "conf" else s[key]), f"input {key} was written"
    return mid.cpu().numpy()


def same_bits(got, want, where, keys=wr.KEYS):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (where, key)
        if got[key].tobytes() != want[key].tobytes():
            bad = np.argwhere((got[key].view(np.int64) if got[key].dtype == np.float64 else got[key]) !=
                              (want[key].view(np.int64) if want[key].dtype == np.float64 else want[key]))
            at = tuple(bad[0])
            raise AssertionError(f"{where} {key}: {len(bad)} elements differ; the first at {at}: device {got[key][at]!r}, restatement {want[key][at]!r}")


@pytest.fixture(scope="module")
def device_runs(T):
    """(name, kind) -> the device's outputs of the base run, launched once per process and shared by the tests that compare runs."""
    done = {}

    def get(name, kind):
        if (name, kind) not in done:
            done[(name, kind)] = run_case(T, pc.case(name), cases.weights(name, kind))
        return done[(name, kind)]
    return get


# ------------------------------------------------------------------------------------------------- 1. the restatement, bit for bit
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_output_equals_the_restatement_bit_for_bit(device_runs, name, kind):
    got, want = device_runs(name, kind), cases.expected(name, kind)
    print(f"{name} / {kind}: status {np.bincount(got['status'], minlength=4)} / {np.bincount(want['status'], minlength=4)}, selected "
          f"{int(got['selected_count'].sum())} of {int(got['inlier_count_in'].sum())} geometrically in, usable up to {int(got['usable_count'].max())}")
    same_bits(got, want, f"{name} / {kind}")


@pytest.mark.parametrize("name,override", cases.VARIATIONS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in o.items())}" for n, o in cases.VARIATIONS])
def test_iteration_counts_and_huber_deltas_under_random_weights(T, name, override):
    got = run_case(T, pc.case(name), cases.weights(name, "random"), **override)
    want = cases.expected(name, "random", tuple(override.items()))
    print(f"{name} {override}: status {np.bincount(want['status'], minlength=4)}, accepted steps {np.bincount(want['iterations'])}")
    same_bits(got, want, f"{name} {override}")


# ------------------------------------------------------------------------------------------------------ 2. the two invariants
def test_all_ones_equals_the_unweighted_entry_byte_for_byte(T, device_runs):
    """On the same operands, in one test: every shared output of the weighted entry under weights of exactly 1.0f is
    sslam_pose_refine_pairs' bytes, and weight_sum is the number of selected rows."""
    from sslam_amd import lib
    for name in cases.NAMES:
        c = pc.case(name)
        w = device_runs(name, "ones")
        ins = {key: _dev(T, c[key]) for key in INPUTS}
        u = lib.pose_refine_pairs(*(ins[key] for key in INPUTS), c["cam"], _dev(T, c["T_in"]), c["scale_x"], c["scale_y"], c["threshold"], c["huber"],
                                  c["n_iter"])
        u = {key: v.cpu().numpy() for key, v in zip(lib.POSE_REFINE_KEYS, u)}
        same_bits(w, u, f"{name}: all ones against the unweighted entry", keys=lib.POSE_REFINE_KEYS)
        assert np.array_equal(w["weight_sum"], w["selected_count"].astype(np.float64)), name
        assert np.array_equal(w["selected_count"], w["inlier_count_in"]), name


def test_power_of_two_scaling_is_exact(device_runs):
    for name in cases.NAMES:
        base = device_runs(name, "random")
        for kind, f in (("quarter", 0.25), ("eight", 8.0)):
            e = device_runs(name, kind)
            for key in wr.KEYS:
                if key in wr.SCALED:
                    assert (e[key] == base[key] * f).all(), (name, kind, key)
                else:
                    assert e[key].tobytes() == base[key].tobytes(), (name, kind, key)
    assert any((device_runs(name, "random")["status"] == 0).any() for name in cases.NAMES)


def test_a_pair_s_row_does_not_depend_on_its_place_in_the_list(T, device_runs):
    name = "k64_p70"
    c, w = pc.case(name), cases.weights(name, "bad")
    P = len(c["first"])
    perm = np.random.default_rng(3).permutation(P)
    moved = dict(c, first=c["first"][perm].copy(), second=c["second"][perm].copy(), matches=c["matches"][perm].copy(), count=c["count"][perm].copy(),
                 T_in=c["T_in"][perm].copy())
    got, base = run_case(T, moved, w[perm].copy()), device_runs(name, "bad")
    for key in wr.KEYS:
        assert got[key].tobytes() == base[key][perm].tobytes(), f"{key}: a pair's row depends on its place in the list"
    assert len(set(base["status"].tolist())) >= 2


# ------------------------------------------------------------------------------------------------------ 3. sslu_match_weights
@pytest.mark.parametrize("mode", [wr.PRODUCT, wr.EXPECTED_ERROR])
@pytest.mark.parametrize("shape", ["k1", "k300_n257", "k4096"])
def test_match_weights_equal_the_restatement_bit_for_bit(T, shape, mode):
    """K = n1 = 1; n1 = 257 < K = 300; K = n1 = 4096; count 0, negative and above n1; indices -1 and K; absent pairs."""
    s = cases.weight_case(shape)
    for sigma0 in ((1.0,) if mode == wr.PRODUCT else (0.3, 7.5)):
        got = run_weights(T, s, mode, sigma0)
        want = wr.match_weights(s["conf"], s["first"], s["second"], s["matches"], s["count"], mode, sigma0)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), f"{shape} mode {mode} sigma0 {sigma0}: {int((got.view(np.int32) != want.view(np.int32)).sum())} slots differ"
    if shape != "k1":
        assert (want == 0).any() and (want > 0).any() and ((s["count"] <= 0).any() and (s["count"] > s["n1"]).any())


def test_match_weights_ignore_sigma0_in_the_product_mode(T):
    from sslam_amd import lib
    s = cases.weight_case("k300_n257")
    ins = {key: _dev(T, s[key]) for key in ("conf", "first", "second", "matches", "count")}
    out = T.empty(s["matches"].shape[:2], dtype=T.float32, device="cuda")
    want = wr.match_weights(s["conf"], s["first"], s["second"], s["matches"], s["count"], wr.PRODUCT)
    for v in (0.0, -1.0, float("nan"), float("inf")):
        with T.cuda.device(0):
            rc = lib.weight().sslu_match_weights(ins["conf"].data_ptr(), s["n_bank"], s["K"], ins["first"].data_ptr(), ins["second"].data_ptr(),
                                                 len(s["first"]), ins["matches"].data_ptr(), ins["count"].data_ptr(), s["n1"], wr.PRODUCT, v,
                                                 out.data_ptr(), C.c_void_p(T.cuda.current_stream().cuda_stream))
        assert rc == lib.OK and out.cpu().numpy().tobytes() == want.tobytes(), v


# ---------------------------------------------------------------------------------------------------------- 4. least alignment
@pytest.mark.parametrize("mode", ["lo", "hi"])
@pytest.mark.parametrize("entry", list(wt.ALIGN))
def test_every_pointer_at_its_least_alignment(T, entry, mode):
    """Each operand at the alignment include/sslam_weight.h states and no better, just past and just before a 256-byte boundary:
    the restatement's bits all the same."""
    with guarded.placed(guarded.Placement(wt.ALIGN[entry], mode)) as p:
        if entry == "sslu_match_weights":
            s = cases.weight_case("k300_n257")
            got = dict(weight=run_weights(T, s, wr.EXPECTED_ERROR, 0.5))
            want = dict(weight=wr.match_weights(s["conf"], s["first"], s["second"], s["matches"], s["count"], wr.EXPECTED_ERROR, 0.5))
        else:
            got, want = run_case(T, pc.case("k1025"), cases.weights("k1025", "bad")), cases.expected("k1025", "bad")
    assert sorted(r["name"] for r in p.made) == sorted(wt.ALIGN[entry])
    for r in p.made:
        a = r["align"]
        assert r["middle"].data_ptr() % 256 == (a if mode == "lo" else 256 - a), r["name"]
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), f"{entry} placed {mode}: {key}"


# ------------------------------------------------------------------------------------------------------------- 5. refusals
def test_every_refusal_returns_its_code_and_writes_nothing(T):
    from sslam_amd import lib
    c = pc.case("k5_dup")
    P, n1, k = len(c["first"]), c["n1"], c["bank"].shape[1]
    ins = {key: _dev(T, c[key]) for key in INPUTS}
    t_in = _dev(T, c["T_in"])
    weight = _dev(T, np.append(cases.weights("k5_dup", "random").reshape(-1), np.float32(1.0)))      # one float more: the call 4 bytes on reads it
    conf = _dev(T, cases.confidence_bank(c, 1))
    out = _outputs(T, P, n1)
    w_whole, w_mid = guarded.guarded(T, (P, n1), T.float32)
    cam = c["cam"]
    base = dict(kp_bank=ins["bank"].data_ptr(), kp_depth_bank=ins["depth_bank"].data_ptr(), n_bank=len(c["bank"]), K=k,
                pair_first=ins["first"].data_ptr(), pair_second=ins["second"].data_ptr(), n_pairs=P, matches=ins["matches"].data_ptr(),
                count=ins["count"].data_ptr(), n1=n1, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, depth_scale=cam.depth_scale,
                scale_x=c["scale_x"], scale_y=c["scale_y"], view_w=float(cam.width), view_h=float(cam.height), threshold=3.0,
                T_in=t_in.data_ptr(), huber=1.0, n_iter=5, weight=weight.data_ptr())
    base.update({key: out[key][2].data_ptr() for key in lib.POSE_REFINE_WEIGHTED_KEYS})
    pointers = ("kp_bank", "kp_depth_bank", "pair_first", "pair_second", "matches", "count", "T_in", "weight") + lib.POSE_REFINE_WEIGHTED_KEYS
    doubles = ("fx", "fy", "cx", "cy", "depth_scale", "scale_x", "scale_y", "view_w", "view_h", "threshold", "huber")
    stream = lambda: C.c_void_p(T.cuda.current_stream().cuda_stream)       # noqa: E731

    def call(**change):
        a = dict(base, **change)
        conv = lambda key: C.c_void_p(a[key]) if key in pointers else C.c_double(a[key]) if key in doubles else int(a[key])      # noqa: E731
        with T.cuda.device(0):
            return lib.weight().sslu_pose_refine_weighted_pairs(*(conv(key) for key in base), stream())

    wbase = dict(conf_bank=conf.data_ptr(), n_bank=len(c["bank"]), K=k, pair_first=ins["first"].data_ptr(), pair_second=ins["second"].data_ptr(),
                 n_pairs=P, matches=ins["matches"].data_ptr(), count=ins["count"].data_ptr(), n1=n1, mode=wr.EXPECTED_ERROR, sigma0=1.0,
                 weight=w_mid.data_ptr())
    wpointers = ("conf_bank", "pair_first", "pair_second", "matches", "count", "weight")

    def wcall(**change):
        a = dict(wbase, **change)
        conv = lambda key: C.c_void_p(a[key]) if key in wpointers else C.c_double(a[key]) if key == "sigma0" else int(a[key])      # noqa: E731
        with T.cuda.device(0):
            return lib.weight().sslu_match_weights(*(conv(key) for key in wbase), stream())

    refused = [({key: None}, lib.E_INVALID) for key in pointers]                                       # NULL, weight and weight_sum among them
    refused += [({key: base[key] + 2}, lib.E_INVALID) for key in pointers]                             # misaligned (2 bytes off)
    refused += [({key: base[key] + 4}, lib.E_INVALID) for key in pointers if wt.ALIGN["sslu_pose_refine_weighted_pairs"][key] == 8]
    refused += [({key: v}, lib.E_INVALID) for key in ("n_bank", "K", "n_pairs", "n1") for v in (0, -1)]
    refused += [(dict(n1=k + 1), lib.E_INVALID), (dict(n_iter=-1), lib.E_INVALID), (dict(n_iter=lib.REFINE_MAX_ITER + 1), lib.E_INVALID)]
    refused += [(dict(threshold=v), lib.E_INVALID) for v in (-1.0, float("nan"), float("inf"))]
    refused += [({key: v}, lib.E_INVALID) for key in ("fx", "fy", "depth_scale", "scale_x", "scale_y", "view_w", "view_h", "huber")
                for v in (0.0, -1.0, float("nan"), float("inf"))]
    refused += [(dict(K=lib.EVAL_MAX_K + 1), lib.E_UNSUPPORTED), (dict(K=lib.EVAL_MAX_K + 1, n1=lib.EVAL_MAX_K + 2), lib.E_INVALID)]
    wrefused = [({key: None}, lib.E_INVALID) for key in wpointers] + [({key: wbase[key] + 2}, lib.E_INVALID) for key in wpointers]
    wrefused += [(dict(matches=wbase["matches"] + 4), lib.E_INVALID)]
    wrefused += [({key: v}, lib.E_INVALID) for key in ("n_bank", "K", "n_pairs", "n1") for v in (0, -1)]
    wrefused += [(dict(mode=v), lib.E_INVALID) for v in (2, -1, 255)]
    wrefused += [(dict(sigma0=v), lib.E_INVALID) for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf"))]
    wrefused += [(dict(n_pairs=1 << 20, n1=1 << 12), lib.E_UNSUPPORTED)]
    n0 = lib.weight_launch_count()
    for change, code in refused:
        assert call(**change) == code, (change, code)
    for change, code in wrefused:
        assert wcall(**change) == code, (change, code)
    T.cuda.synchronize()
    assert lib.weight_launch_count() == n0, "a refused call launched something"
    for key, (whole, mid, _) in out.items():
        guarded.assert_guards(whole, mid, f"refused {key}")
        assert bool((mid == (guarded.SENTINEL64 if mid.dtype == T.int64 else guarded.SENTINEL)).all()), f"a refused call wrote {key}"
    guarded.assert_guards(w_whole, w_mid, "refused weight")
    assert bool((w_mid.view(T.int32) == guarded.SENTINEL).all()), "a refused call wrote weight"
    assert call() == lib.OK and wcall() == lib.OK and lib.weight_launch_count() == n0 + 2, "the unchanged arguments are accepted"
    assert call(weight=base["weight"] + 4) == lib.OK, "4-byte alignment is all the weights need"
    T.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. the layers above the entries
E2E_THRESHOLD = 12.0        # px: the selector's keypoints sit on the 16-px patch grid (tests/test_gpu_pose_refine.py's choice)
E2E_HYP, E2E_SEED, E2E_HUBER, E2E_ITER = 64, 5, 4.0, 5


@pytest.fixture(scope="module")
def seq(T):
    import confidence_cases
    import pose_depth_cases
    import pose_eval_ref as pr
    from sslam_amd import evaluation as ev
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, PoseWeights, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K, confidence=True), inp["selector"], inp["refiner"],
                            device="cuda", confidence_state=confidence_cases.head_state("x4"))
    toks = T.from_numpy(inp["tokens"]).cuda()
    return dict(pipe=pipe, toks=toks, poses=inp["poses"], depth=pose_depth_cases.sequence_depth(), cam=ev.Camera(),
                rule=MatchRule.mnn_ratio(0.9), k=pr.SEQ_K, weights=PoseWeights.expected_error(0.5))


def _counts(lib):
    return np.array([lib.launch_count(), lib.conf_launch_count(), lib.weight_launch_count()])


def _by_hand(T, s, pairs, weights):
    """extract -> match_pairs -> match_weights -> estimate_poses -> weighted refine_poses over `pairs`."""
    from sslam_amd import evaluation as ev
    pipe = s["pipe"]
    ex = pipe.extract(s["toks"], None)
    kd = ev.gather_keypoint_depth(pipe, s["depth"], ex["keypoints_pixel"], len(s["depth"]))
    f, sec = [a for a, _ in pairs], [b for _, b in pairs]
    mm = pipe.match_pairs(ex["descriptors"], ex["scores"], first=f, second=sec, rule=s["rule"])
    w = None if weights is None else pipe.match_weights(ex["confidence"], f, sec, mm, weights)
    est = pipe.estimate_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], E2E_THRESHOLD, E2E_HYP, E2E_SEED)
    ref = pipe.refine_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], est, E2E_THRESHOLD, E2E_HUBER, E2E_ITER, weights=w)
    return dict(ex=ex, kd=kd, mm=mm, w=w, est=est, ref=ref, f=f, sec=sec)


def test_refine_poses_with_weights_equals_the_lib_call(T, seq):
    from sslam_amd import lib
    s = seq
    pipe = s["pipe"]
    pairs = [(0, 1), (1, 2), (2, 3), (-1, 4), (3, 8), (7, 2), (0, 1)]
    h = _by_hand(T, s, pairs, s["weights"])
    ex, kd, mm, w = h["ex"], h["kd"], h["mm"], h["w"]
    first, second = _dev(T, np.array(h["f"], np.int32)), _dev(T, np.array(h["sec"], np.int32))
    assert w.shape == mm["matches"].shape[:2] and w.dtype == T.float32
    direct_w = lib.match_weights(ex["confidence"], first, second, mm["matches"], mm["match_count"], lib.WEIGHT_EXPECTED_ERROR, 0.5)
    assert direct_w.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()
    want_w = wr.match_weights(ex["confidence"].cpu().numpy(), h["f"], h["sec"], mm["matches"].cpu().numpy(), mm["match_count"].cpu().numpy(),
                              wr.EXPECTED_ERROR, 0.5)
    assert w.cpu().numpy().tobytes() == want_w.tobytes() and (want_w[3] == 0).all() and (want_w > 0).any()
    sx, sy = pipe.depth_scales(s["cam"])
    direct = lib.pose_refine_weighted(ex["keypoints_pixel"], kd, first, second, mm["matches"], mm["match_count"], s["cam"], h["est"]["T"], w, sx, sy,
                                      E2E_THRESHOLD, E2E_HUBER, E2E_ITER)
    assert list(h["ref"]) == list(lib.POSE_REFINE_WEIGHTED_KEYS)
    for key, v in zip(lib.POSE_REFINE_WEIGHTED_KEYS, direct):
        assert h["ref"][key].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), key
    ref = {key: v.cpu().numpy() for key, v in h["ref"].items()}
    assert ref["status"][3] == 3 and (ref["status"][[0, 1, 2]] != 3).all() and ref["T"][0].tobytes() == ref["T"][6].tobytes()
    assert (ref["weight_sum"][ref["status"] != 3] > 0).all() and (ref["weight_sum"][ref["status"] == 3] == 0).all()
    out = pipe.alloc_pose_refine(len(pairs), s["k"], weighted=True)
    assert list(out) == list(lib.POSE_REFINE_WEIGHTED_KEYS) and list(pipe.alloc_pose_refine(2, s["k"])) == list(lib.POSE_REFINE_KEYS)
    again = pipe.refine_poses(ex["keypoints_pixel"], kd, h["f"], h["sec"], mm, s["cam"], h["est"], E2E_THRESHOLD, E2E_HUBER, E2E_ITER, out=out, weights=w)
    assert again["weight_sum"] is out["weight_sum"] and out["T"].cpu().numpy().tobytes() == ref["T"].tobytes()
    # the weights change the answer, and weights of one do not
    plain = {key: v.cpu().numpy() for key, v in _by_hand(T, s, pairs, None)["ref"].items()}
    assert "weight_sum" not in plain and plain["info"].tobytes() != ref["info"].tobytes()
    ones = pipe.refine_poses(ex["keypoints_pixel"], kd, h["f"], h["sec"], mm, s["cam"], h["est"], E2E_THRESHOLD, E2E_HUBER, E2E_ITER, weights=T.ones_like(w))
    for key in lib.POSE_REFINE_KEYS:
        assert ones[key].cpu().numpy().tobytes() == plain[key].tobytes(), key
    with pytest.raises(ValueError, match="weights"):
        pipe.refine_poses(ex["keypoints_pixel"], kd, h["f"], h["sec"], mm, s["cam"], h["est"], E2E_THRESHOLD, E2E_HUBER, E2E_ITER, weights=w[:, :-1])
    with pytest.raises(ValueError, match="weight_sum"):
        pipe.refine_poses(ex["keypoints_pixel"], kd, h["f"], h["sec"], mm, s["cam"], h["est"], E2E_THRESHOLD, E2E_HUBER, E2E_ITER,
                          out=pipe.alloc_pose_refine(len(pairs), s["k"]), weights=w)


def test_odometry_with_weights_is_the_chain_done_by_hand(T, seq):
    from sslam_amd import lib
    from sslam_amd import odometry as od
    s = seq
    pipe = s["pipe"]
    kw = dict(camera=s["cam"], poses=s["poses"], threshold=E2E_THRESHOLD, hypotheses=E2E_HYP, seed=E2E_SEED, rule=s["rule"], refine=True, huber=E2E_HUBER,
              iterations=E2E_ITER)
    od.odometry(pipe, tokens=s["toks"], depth=s["depth"], **kw)              # warm: every lazy allocation made
    n0 = _counts(lib)
    plain = od.odometry(pipe, tokens=s["toks"], depth=s["depth"], **kw)
    n1 = _counts(lib)
    got = od.odometry(pipe, tokens=s["toks"], depth=s["depth"], weights=s["weights"], **kw)
    n2 = _counts(lib)
    assert "weight_sum" not in plain["refine"] and (n1 - n0)[2] == 0, "without weights: no weight_sum, nothing of the eighth library launched"
    assert list(plain["refine"]) == ["status", "iterations", "selected_count", "cost_in", "cost", "info"]
    d = (n2 - n1) - (n1 - n0)
    assert d.tolist() == [-1, 0, 2], f"weighted: match_weights and the weighted refinement in the unweighted refinement's place, got {d}"
    h = _by_hand(T, s, plain["pairs"], s["weights"])
    ref = {key: v.cpu().numpy() for key, v in h["ref"].items()}
    assert got["T"][:, :3].tobytes() == ref["T"].reshape(-1, 3, 4).tobytes()
    for key in ("inlier_count", "rms"):
        assert np.array_equal(got[key], ref[key]), key
    for key in ("status", "iterations", "selected_count", "cost_in", "cost", "weight_sum"):
        assert np.array_equal(got["refine"][key], ref[key]), key
    assert list(got["refine"]) == ["status", "iterations", "selected_count", "cost_in", "cost", "info", "weight_sum"]
    assert got["refine"]["info"].tobytes() == od.info_matrix(ref["info"]).tobytes() != plain["refine"]["info"].tobytes()
    for key in got["ransac"]:
        assert repr(got["ransac"][key]) == repr(plain["ransac"][key]), ("ransac", key)
    assert (got["refine"]["status"] == 0).any() and (got["refine"]["weight_sum"] > 0).any()


def test_odometry_graph_reads_the_weighted_information(T, seq):
    from sslam_amd import odometry as od
    s = seq
    pipe = s["pipe"]
    kw = dict(camera=s["cam"], poses=s["poses"], spacings=(1, 3), threshold=E2E_THRESHOLD, hypotheses=E2E_HYP, seed=E2E_SEED, rule=s["rule"],
              huber=E2E_HUBER, iterations=E2E_ITER)
    plain = od.odometry_graph(pipe, tokens=s["toks"], depth=s["depth"], **kw)
    got = od.odometry_graph(pipe, tokens=s["toks"], depth=s["depth"], weights=s["weights"], **kw)
    pairs = got["graph"]["pairs"]
    assert pairs == plain["graph"]["pairs"] and len(pairs) == len(got[1]["pairs"]) + len(got[3]["pairs"])
    h = _by_hand(T, s, pairs, s["weights"])
    ref = {key: v.cpu().numpy() for key, v in h["ref"].items()}
    at = 0
    for sp in (1, 3):
        n = len(got[sp]["pairs"])
        assert "weight_sum" not in plain[sp]["refine"]
        assert np.array_equal(got[sp]["refine"]["weight_sum"], ref["weight_sum"][at:at + n])
        assert got[sp]["refine"]["info"].tobytes() == od.info_matrix(ref["info"][at:at + n]).tobytes()
        assert got[sp]["T"][:, :3].tobytes() == ref["T"][at:at + n].reshape(-1, 3, 4).tobytes()
        at += n
    lists = {sp: got[sp]["pairs"] for sp in (1, 3)}
    n_nodes = len(got["graph"]["trajectory"])
    g = od._graph_device(pipe, h["ref"], pairs, lists, n_nodes, s["poses"], 3, 4.0, 0.0, 8)
    assert got["graph"]["edge_chi2"].tobytes() == g["edge_chi2"].cpu().numpy().tobytes(), "the graph ran on the weighted information matrices"
    assert got["graph"]["cost"] == float(g["cost"].cpu()) and got["graph"]["status"] == int(g["status"].cpu())
    assert got["graph"]["edge_chi2"].tobytes() != plain["graph"]["edge_chi2"].tobytes()


@pytest.mark.parametrize("use_graph", [False, True])
def test_pose_frame_stepper_with_weights_equals_the_batched_rows(T, seq, use_graph):
    from sslam_amd import lib
    from sslam_amd.online import PoseFrameStepper
    s = seq
    pipe, n = s["pipe"], 4
    sub = dict(s, toks=s["toks"][:n], depth=s["depth"][:n])
    h = _by_hand(T, sub, [(i, i + 1) for i in range(n - 1)], s["weights"])
    want = {key: v.cpu().numpy() for key, v in h["ref"].items()}
    want_est = {key: v.cpu().numpy() for key, v in h["est"].items()}
    mk = lambda graph, **more: PoseFrameStepper(pipe, 48, 64, 480, 640, camera=s["cam"], use_graph=graph, tokens_in=True, threshold=E2E_THRESHOLD,      # noqa: E731
                                                hypotheses=E2E_HYP, seed=E2E_SEED, refine=True, huber=E2E_HUBER, iterations=E2E_ITER, **more)
    st = mk(use_graph, weights=s["weights"])
    image = T.zeros((48, 64, 3), dtype=T.uint8, device="cuda")
    depth = T.from_numpy(s["depth"]).cuda()
    for i in range(n):
        n0 = _counts(lib)
        out = st.step(image, depth[i], s["toks"][i])
        if use_graph and i:
            assert (_counts(lib) == n0).all(), "a replayed step makes no library call"
        if i == 0:
            assert out["pose"] is None
            continue
        assert set(out["pose"]["refined"]) == set(lib.POSE_REFINE_WEIGHTED_KEYS)
        for key in lib.POSE_RANSAC_KEYS:
            assert out["pose"][key].cpu().numpy().tobytes() == want_est[key][i - 1].tobytes(), f"frame {i}: RANSAC's {key} is untouched"
        for key in lib.POSE_REFINE_WEIGHTED_KEYS:
            assert out["pose"]["refined"][key].cpu().numpy().tobytes() == want[key][i - 1].tobytes(), f"frame {i}: refined {key}"
    assert (want["status"] == 0).any() and (want["weight_sum"] > 0).any()
    plain = mk(False)
    assert plain.weight is None and plain.weights is None and set(plain.refined) == set(lib.POSE_REFINE_KEYS)
    if not use_graph:
        steps = []
        for stepper in (plain, st):
            stepper.reset()
            stepper.step(image, depth[0], s["toks"][0])
            n0 = _counts(lib)
            res = stepper.step(image, depth[1], s["toks"][1])
            steps.append(_counts(lib) - n0)
        assert "weight_sum" not in plain.step(image, depth[2], s["toks"][2])["pose"]["refined"]
        assert int(steps[1].sum()) == int(steps[0].sum()) + 1 and steps[0][2] == 0 and steps[1][2] == 2, (steps, "exactly one launch more per step")
        assert res["pose"]["refined"]["weight_sum"].cpu().numpy().tobytes() == want["weight_sum"][0].tobytes()
