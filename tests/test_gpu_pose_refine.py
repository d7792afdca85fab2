"""GPU tests of the pose refinement: sslam_pose_refine_pairs through sslam_amd.lib, SequencePipeline.refine_poses,
sslam_amd.odometry(refine=True), online.PoseFrameStepper(refine=True), run_directory(evaluate={"refine": True}) and the drop-in
refine_relative_pose.

Reference: the float64 restatement of tests/pose_refine_ref.py on the seeded cases of tests/pose_refine_cases.py, which
tests/test_pose_refine_cpu.py holds to their margins, to an independent implementation and to the planted motions.  EVERY output
is compared bit for bit, as bytes - T, cost_in, cost, rms and info included (pose_ransac_ref's docstring says why no tolerance is
needed).  Every launch goes into poisoned outputs between guard bands (tests/guarded.py) with the inputs between NaN bands; inputs
are compared with their host copies after the call; launches are counted."""
import ctypes as C

import numpy as np
import pytest

import guarded
import pose_ransac_ref as rr
import pose_refine_cases as cases
import pose_refine_ref as fr

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
    shapes, out = lib.pose_refine_shapes(n_pairs, n1), {}
    for key in lib.POSE_REFINE_KEYS:
        shape, dt = shapes[key]
        whole, mid = guarded.guarded(T, shape, T.int64 if dt == T.float64 else dt, name=key)
        out[key] = (whole, mid, mid.view(T.float64) if dt == T.float64 else mid)
    return out


INPUTS = ("bank", "depth_bank", "first", "second", "matches", "count")
ARG = dict(bank="kp_bank", depth_bank="kp_depth_bank", first="pair_first", second="pair_second", matches="matches", count="count")      # include/sslam_hip.h


def run_case(T, c, **override):
    """sslam_pose_refine_pairs on a case, one launch into poisoned, guarded outputs -> dict of numpy arrays."""
    from sslam_amd import lib
    a = dict(threshold=c["threshold"], huber=c["huber"], n_iter=c["n_iter"], T_in=c["T_in"])
    a.update(override)
    ins = {key: guarded.guarded_input(T, c[key], name=ARG[key]) for key in INPUTS}
    ins["T_in"] = guarded.guarded_input(T, np.ascontiguousarray(a["T_in"]).view(np.int64), name="T_in")      # float64 bits, NaN among them
    out = _outputs(T, len(c["first"]), c["n1"])
    n0 = lib.launch_count()
    lib.pose_refine_pairs(*(ins[key][1] for key in INPUTS), c["cam"], ins["T_in"][1].view(T.float64), c["scale_x"], c["scale_y"], a["threshold"],
                          a["huber"], a["n_iter"], out=tuple(out[key][2] for key in lib.POSE_REFINE_KEYS))
    assert lib.launch_count() - n0 == 1, "one launch"
    got = {}
    for key, (whole, mid, t) in out.items():
        guarded.assert_guards(whole, mid, f"pose_refine_pairs {key}")
        guarded.assert_written(mid, f"pose_refine_pairs {key}")
        got[key] = t.cpu().numpy()
    for key, (whole, mid) in ins.items():
        guarded.assert_guards(whole, mid, f"input {key}")
        want = np.ascontiguousarray(a["T_in"]).view(np.int64) if key == "T_in" else c[key]
        assert np.array_equal(mid.cpu().numpy(), want), f"input {key} was written"
    return got


def same_bits(got, want, where, keys=fr.KEYS):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (where, key)
        if got[key].tobytes() != want[key].tobytes():
            bad = np.argwhere((got[key].view(np.int64) if got[key].dtype == np.float64 else got[key]) !=
                              (want[key].view(np.int64) if want[key].dtype == np.float64 else want[key]))
            at = tuple(bad[0])
            raise AssertionError(f"{where} {key}: {len(bad)} elements differ; the first at {at}: device {got[key][at]!r}, restatement {want[key][at]!r}")


# ------------------------------------------------------------------------------------------------- 1. the restatement, bit for bit
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_output_equals_the_restatement_bit_for_bit(T, name):
    c = cases.case(name)
    got = run_case(T, c)
    want = cases.expected(name)
    print(f"{name}: status {np.bincount(got['status'], minlength=4)} / {np.bincount(want['status'], minlength=4)}, accepted steps "
          f"{np.bincount(got['iterations'])}, usable {sorted(set(got['usable_count'].tolist()))[-4:]}, "
          f"max |T - T'| {np.abs(np.where(np.isfinite(want['T']), got['T'], 0.0) - np.where(np.isfinite(want['T']), want['T'], 0.0)).max():.3e}, "
          f"max |cost - cost'| {np.abs(got['cost'] - want['cost']).max():.3e}")
    same_bits(got, want, name)
    again = run_case(T, c)
    for key in fr.KEYS:
        assert got[key].tobytes() == again[key].tobytes(), f"{name} {key}: the same call twice gave other bits"


@pytest.mark.parametrize("name,override", cases.VARIATIONS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in o.items())}" for n, o in cases.VARIATIONS])
def test_iteration_counts_and_huber_deltas(T, name, override):
    """n_iter 0, 5 and 16 (the base runs take 1 and 2), huber below every residual and above every residual."""
    c = cases.case(name)
    got = run_case(T, c, **override)
    want = cases.expected(name, tuple(override.items()))
    print(f"{name} {override}: status {np.bincount(want['status'], minlength=4)}, accepted steps {np.bincount(want['iterations'])}")
    same_bits(got, want, f"{name} {override}")


def test_chain_ransac_then_refine_and_a_second_refinement(T):
    """The device chain RANSAC -> refine equals the restatement's chain; refining the entry's own output gives cost no higher."""
    from sslam_amd import lib
    for name in ("k64_p70", "k1025"):
        c = cases.case(name)
        ins = {key: _dev(T, c[key]) for key in INPUTS}
        est = lib.pose_ransac_pairs(*(ins[key] for key in INPUTS), c["cam"], c["scale_x"], c["scale_y"], 3.0, c["n_hyp"], cases.SEED)
        assert est[0].cpu().numpy().tobytes() == c["ransac"]["T"].tobytes(), "the RANSAC launch gives the restatement's poses"
        ref = lib.pose_refine_pairs(*(ins[key] for key in INPUTS), c["cam"], est[0], c["scale_x"], c["scale_y"], 3.0, 1.0, 5)
        got = {key: v.cpu().numpy() for key, v in zip(lib.POSE_REFINE_KEYS, ref)}
        want = fr.stacked(cases.run(c, threshold=3.0, huber=1.0, n_iter=5, T_in=c["ransac"]["T"]))
        same_bits(got, want, f"{name}: RANSAC -> refine")
        twice = lib.pose_refine_pairs(*(ins[key] for key in INPUTS), c["cam"], ref[0], c["scale_x"], c["scale_y"], 3.0, 1.0, 5)
        got2 = {key: v.cpu().numpy() for key, v in zip(lib.POSE_REFINE_KEYS, twice)}
        same_bits(got2, fr.stacked(cases.run(c, threshold=3.0, huber=1.0, n_iter=5, T_in=want["T"])), f"{name}: refine -> refine")
        # the second call selects again, so its cost is over its own rows; where the selection did not change it cannot be higher
        kept = got2["selected_count"] == got["selected_count"]
        assert kept.any() and (got2["cost"][kept] <= got["cost"][kept]).all() and (got2["cost"] <= got2["cost_in"]).all()
        assert (got["cost"] <= got["cost_in"]).all()


# ------------------------------------------------------------------------------------------------------------- 2. refusals
def test_every_refusal_returns_its_code_and_writes_nothing(T):
    from sslam_amd import lib
    c = cases.case("k5_dup")
    P, n1, k = len(c["first"]), c["n1"], c["bank"].shape[1]
    ins = {key: _dev(T, c[key]) for key in INPUTS}
    t_in = _dev(T, c["T_in"])
    out = _outputs(T, P, n1)
    cam = c["cam"]
    base = dict(kp_bank=ins["bank"].data_ptr(), kp_depth_bank=ins["depth_bank"].data_ptr(), n_bank=len(c["bank"]), K=k,
                pair_first=ins["first"].data_ptr(), pair_second=ins["second"].data_ptr(), n_pairs=P, matches=ins["matches"].data_ptr(),
                count=ins["count"].data_ptr(), n1=n1, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, depth_scale=cam.depth_scale,
                scale_x=c["scale_x"], scale_y=c["scale_y"], view_w=float(cam.width), view_h=float(cam.height), threshold=3.0,
                T_in=t_in.data_ptr(), huber=1.0, n_iter=5)
    base.update({key: out[key][2].data_ptr() for key in lib.POSE_REFINE_KEYS})
    pointers = ("kp_bank", "kp_depth_bank", "pair_first", "pair_second", "matches", "count", "T_in") + lib.POSE_REFINE_KEYS
    doubles = ("fx", "fy", "cx", "cy", "depth_scale", "scale_x", "scale_y", "view_w", "view_h", "threshold", "huber")

    def call(**change):
        a = dict(base, **change)
        conv = lambda key: C.c_void_p(a[key]) if key in pointers else C.c_double(a[key]) if key in doubles else int(a[key])
        with T.cuda.device(0):
            return lib.lib().sslam_pose_refine_pairs(*(conv(key) for key in base), C.c_void_p(T.cuda.current_stream().cuda_stream))

    refused = [({key: None}, lib.E_INVALID) for key in pointers]                                       # NULL
    refused += [({key: base[key] + 2}, lib.E_INVALID) for key in pointers]                             # misaligned (2 bytes off)
    refused += [({key: v}, lib.E_INVALID) for key in ("n_bank", "K", "n_pairs", "n1") for v in (0, -1)]
    refused += [(dict(n1=k + 1), lib.E_INVALID), (dict(n_iter=-1), lib.E_INVALID), (dict(n_iter=lib.REFINE_MAX_ITER + 1), lib.E_INVALID)]
    refused += [(dict(threshold=v), lib.E_INVALID) for v in (-1.0, float("nan"), float("inf"))]
    refused += [({key: v}, lib.E_INVALID) for key in ("fx", "fy", "depth_scale", "scale_x", "scale_y", "view_w", "view_h", "huber")
                for v in (0.0, -1.0, float("nan"), float("inf"))]
    refused += [({key: v}, lib.E_INVALID) for key in ("cx", "cy") for v in (float("nan"), float("-inf"))]
    refused += [(dict(K=lib.EVAL_MAX_K + 1), lib.E_UNSUPPORTED)]
    n0 = lib.launch_count()
    for change, code in refused:
        assert call(**change) == code, (change, code)
    T.cuda.synchronize()
    assert lib.launch_count() == n0, "a refused call launched something"
    for key, (whole, mid, _) in out.items():
        guarded.assert_guards(whole, mid, f"refused {key}")
        idt = mid.dtype
        assert bool((mid == (guarded.SENTINEL64 if idt == T.int64 else guarded.SENTINEL)).all()), f"a refused call wrote {key}"
    assert call() == lib.OK and lib.launch_count() == n0 + 1, "the unchanged arguments are accepted"
    assert call(n_iter=0) == lib.OK and call(n_iter=lib.REFINE_MAX_ITER) == lib.OK, "both ends of the range"
    T.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the layers above the entry
E2E_THRESHOLD = 12.0        # px: the selector's keypoints sit on the 16-px patch grid (tests/test_gpu_pose_ransac.py's choice)
E2E_HYP, E2E_SEED, E2E_HUBER, E2E_ITER = 64, 5, 4.0, 5


@pytest.fixture(scope="module")
def seq(T):
    import pose_depth_cases
    import pose_eval_ref as pr
    from sslam_amd import evaluation as ev
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K), inp["selector"], inp["refiner"], device="cuda")
    toks = T.from_numpy(inp["tokens"]).cuda()
    return dict(pipe=pipe, toks=toks, poses=inp["poses"], depth=pose_depth_cases.sequence_depth(), cam=ev.Camera(),
                rule=MatchRule.mnn_ratio(0.9), k=pr.SEQ_K)


def test_refine_poses_on_a_permuted_pair_list_gives_the_permuted_rows(T, seq):
    from sslam_amd import evaluation as ev
    from sslam_amd import lib
    s = seq
    pipe = s["pipe"]
    ex = pipe.extract(s["toks"], None)
    kd = ev.gather_keypoint_depth(pipe, s["depth"], ex["keypoints_pixel"], len(s["depth"]))
    first, second = [0, 1, 2, -1, 3, 7, 0], [1, 2, 3, 4, 8, 2, 1]
    perm = [4, 0, 6, 2, 5, 1, 3]

    def run(f, sec):
        mm = pipe.match_pairs(ex["descriptors"], ex["scores"], first=f, second=sec, rule=s["rule"])
        est = pipe.estimate_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], E2E_THRESHOLD, E2E_HYP, E2E_SEED)
        n0 = lib.launch_count()
        out = pipe.refine_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], est, E2E_THRESHOLD, E2E_HUBER, E2E_ITER)
        assert lib.launch_count() - n0 == 1, "one launch, nothing else"
        same = pipe.refine_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], est["T"], E2E_THRESHOLD, E2E_HUBER, E2E_ITER)
        assert all(T.equal(out[key].view(T.int64) if out[key].dtype == T.float64 else out[key],
                           same[key].view(T.int64) if same[key].dtype == T.float64 else same[key]) for key in out), "the dictionary or its T"
        return {key: v.cpu().numpy() for key, v in out.items()}, est, mm
    (a, est, mm), (b, _, _) = run(first, second), run([first[i] for i in perm], [second[i] for i in perm])
    for key in lib.POSE_REFINE_KEYS:
        assert a[key][perm].tobytes() == b[key].tobytes(), f"{key}: a pair's row depends on its place in the list"
    assert a["T"][0].tobytes() == a["T"][6].tobytes() and a["status"][3] == 3 and (a["cost"] <= a["cost_in"]).all()
    assert (a["status"][[0, 1, 2]] != 3).all(), "the sequence has poses to refine"
    assert np.array_equal(a["inlier_count_in"], est["inlier_count"].cpu().numpy()), "T_in's inliers are RANSAC's own count"
    third = pipe.refine_poses(ex["keypoints_pixel"], kd, first, second, mm, s["cam"], est, E2E_THRESHOLD, None, E2E_ITER)      # huber=None
    fourth = pipe.refine_poses(ex["keypoints_pixel"], kd, first, second, mm, s["cam"], est, E2E_THRESHOLD, E2E_THRESHOLD / 3.0, E2E_ITER)
    assert third["T"].cpu().numpy().tobytes() == fourth["T"].cpu().numpy().tobytes() and T.equal(third["iterations"], fourth["iterations"])
    out = pipe.alloc_pose_refine(7, s["k"])
    assert pipe.refine_poses(ex["keypoints_pixel"], kd, first, second, mm, s["cam"], est, E2E_THRESHOLD, E2E_HUBER, E2E_ITER, out=out)["T"] is out["T"]
    assert out["T"].cpu().numpy().tobytes() == a["T"].tobytes()


def _same_value(a, b, what):
    if isinstance(a, dict):
        assert list(a) == list(b), what
        for key in a:
            _same_value(a[key], b[key], (what, key))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    else:
        assert repr(a) == repr(b), what


def test_odometry_with_refinement_is_odometry_followed_by_refine_poses(T, seq):
    from sslam_amd import evaluation as ev
    from sslam_amd import lib
    from sslam_amd import odometry as od
    from sslam_amd.harness import StreamingSequence
    s = seq
    pipe = s["pipe"]
    kw = dict(camera=s["cam"], poses=s["poses"], threshold=E2E_THRESHOLD, hypotheses=E2E_HYP, seed=E2E_SEED)
    base = od.odometry(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], **kw)
    off = od.odometry(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], refine=False, huber=123.0, iterations=3, **kw)
    _same_value(base, off, "refine=False")
    assert list(base) == ["pairs", "T", "inlier_count", "usable_count", "best_hypothesis", "refit_kept", "match_count", "rms", "inlier_ratio",
                          "trajectory", "rpe", "ate"], "what odometry() returned before there was a refinement"
    got = od.odometry(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], refine=True, huber=E2E_HUBER, iterations=E2E_ITER, **kw)
    # the same by hand
    ex = pipe.extract(s["toks"], None)
    kd = ev.gather_keypoint_depth(pipe, s["depth"], ex["keypoints_pixel"], len(s["depth"]))
    pairs = base["pairs"]
    f, sec = [a for a, _ in pairs], [b for _, b in pairs]
    mm = pipe.match_pairs(ex["descriptors"], ex["scores"], first=f, second=sec, rule=s["rule"])
    est = pipe.estimate_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], E2E_THRESHOLD, E2E_HYP, E2E_SEED)
    ref = {key: v.cpu().numpy() for key, v in pipe.refine_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], est, E2E_THRESHOLD, E2E_HUBER, E2E_ITER).items()}
    assert got["T"][:, :3].tobytes() == ref["T"].reshape(-1, 3, 4).tobytes() and np.array_equal(got["T"][:, 3], np.tile([0, 0, 0, 1.0], (len(pairs), 1)))
    for key in ("inlier_count", "rms"):
        assert np.array_equal(got[key], ref[key]), key
    for key in ("status", "iterations", "selected_count", "cost_in", "cost"):
        assert np.array_equal(got["refine"][key], ref[key]), key
    assert got["refine"]["info"].tobytes() == od.info_matrix(ref["info"]).tobytes()
    for key in ("usable_count", "best_hypothesis", "refit_kept", "match_count", "pairs"):
        _same_value(got[key], base[key], key)
    assert list(got["ransac"]) == ["T", "inlier_count", "rms", "inlier_ratio", "trajectory", "rpe", "ate"]
    for key in got["ransac"]:
        _same_value(got["ransac"][key], base[key], ("ransac", key))
    assert np.abs(got["trajectory"] - od.chain(got["T"], s["poses"][0])).max() == 0.0
    _same_value(got["rpe"], od.rpe_summary(od.relative_pose_errors(got["T"], s["poses"], pairs)), "rpe of the refined poses")
    _same_value(got["ate"], od.ate_summary(got["trajectory"], s["poses"][:len(pairs) + 1]), "ate of the refined trajectory")
    assert (got["refine"]["status"] == 0).any() and (got["refine"]["cost"] <= got["refine"]["cost_in"]).all()
    print(f"refined {int((got['refine']['status'] == 0).sum())} of {len(pairs)} pairs; rpe {base['rpe']} -> {got['rpe']} (synthetic frames: no accuracy claim)")
    # one read-back: the library is entered for launches only, and the result of odometry_result is the same dictionary
    result = StreamingSequence(pipe, (1, 5), rule=s["rule"]).run(s["toks"])
    for spacing, num_pairs in ((1, None), (5, 4)):
        a = od.odometry(pipe, tokens=s["toks"], depth=s["depth"], spacing=spacing, num_pairs=num_pairs, rule=s["rule"], refine=True, **kw)
        b = od.odometry_result(pipe, result, depth=T.from_numpy(s["depth"]).cuda(), spacing=spacing, num_pairs=num_pairs, refine=True, **kw)
        _same_value(a, b, f"spacing {spacing}")
        assert ("trajectory" in a) == (spacing == 1) == ("trajectory" in a["ransac"]) and (a["ate"] is None) == (spacing != 1)


@pytest.mark.parametrize("use_graph", [False, True])
def test_pose_frame_stepper_with_refinement_equals_the_batched_rows(T, seq, use_graph):
    from sslam_amd import evaluation as ev
    from sslam_amd import lib
    from sslam_amd.online import PoseFrameStepper
    s = seq
    pipe, n = s["pipe"], 4
    ex = pipe.extract(s["toks"][:n], None)
    kd = ev.gather_keypoint_depth(pipe, s["depth"][:n], ex["keypoints_pixel"], n)
    f, sec = list(range(n - 1)), list(range(1, n))
    mm = pipe.match_pairs(ex["descriptors"], ex["scores"], first=f, second=sec, rule=s["rule"])
    est = pipe.estimate_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], E2E_THRESHOLD, E2E_HYP, E2E_SEED)
    want = {key: v.cpu().numpy() for key, v in pipe.refine_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], est, E2E_THRESHOLD, E2E_HUBER, E2E_ITER).items()}
    want_est = {key: v.cpu().numpy() for key, v in est.items()}
    st = PoseFrameStepper(pipe, 48, 64, 480, 640, camera=s["cam"], use_graph=use_graph, tokens_in=True, threshold=E2E_THRESHOLD,
                          hypotheses=E2E_HYP, seed=E2E_SEED, refine=True, huber=E2E_HUBER, iterations=E2E_ITER)
    image = T.zeros((48, 64, 3), dtype=T.uint8, device="cuda")
    depth = T.from_numpy(s["depth"]).cuda()
    for i in range(n):
        n0 = lib.launch_count()
        out = st.step(image, depth[i], s["toks"][i])
        if use_graph and i:
            assert lib.launch_count() == n0, "a replayed step makes no library call"
        if i == 0:
            assert out["pose"] is None
            continue
        assert set(out["pose"]) == set(lib.POSE_RANSAC_KEYS) | {"refined"} and set(out["pose"]["refined"]) == set(lib.POSE_REFINE_KEYS)
        for key in lib.POSE_RANSAC_KEYS:
            assert out["pose"][key].cpu().numpy().tobytes() == want_est[key][i - 1].tobytes(), f"frame {i}: RANSAC's {key} is untouched"
        for key in lib.POSE_REFINE_KEYS:
            assert out["pose"]["refined"][key].cpu().numpy().tobytes() == want[key][i - 1].tobytes(), f"frame {i}: refined {key}"
    assert (want["status"] == 0).any()
    plain = PoseFrameStepper(pipe, 48, 64, 480, 640, camera=s["cam"], use_graph=False, tokens_in=True, threshold=E2E_THRESHOLD,
                             hypotheses=E2E_HYP, seed=E2E_SEED)
    assert plain.refined is None and plain.refine is False
    plain.step(image, depth[0], s["toks"][0])
    n0 = lib.launch_count()
    st_plain = plain.step(image, depth[1], s["toks"][1])
    launches_plain = lib.launch_count() - n0
    assert "refined" not in st_plain["pose"]
    if not use_graph:
        st.reset()
        st.step(image, depth[0], s["toks"][0])
        n0 = lib.launch_count()
        st.step(image, depth[1], s["toks"][1])
        assert lib.launch_count() - n0 == launches_plain + 1, "the refinement is one launch more, and only when asked for"


def test_run_directory_adds_the_refined_odometry_and_only_when_asked(T, tmp_path):
    import synth
    from sslam_amd import evaluation as ev
    from sslam_amd import odometry as od
    from sslam_amd.harness import run_directory
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    from sslam_amd.tum import TUMSequence
    name, g, k = "rgbd_dataset_freiburg1_desk", 5, 12
    synth.write_tum_sequence(str(tmp_path / name))
    tum = TUMSequence(str(tmp_path), name)
    n = len(tum)
    depth = tum.load_depth_raw(range(n))
    cam = ev.Camera(fx=517.3 / 20, fy=516.5 / 20, cx=318.6 / 20, cy=255.3 / 20, width=32, height=24)      # the fixture's frames are 32 x 24
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    toks = T.from_numpy(synth.token_sequence(n, g)).cuda()
    kw = dict(pipe=pipe, tokens_fn=lambda a, b: toks[a:b], chunk=4, decode_workers=2)
    base = dict(num_pairs=4, threshold=20.0, depth=True, camera=cam, odometry=True)
    old = run_directory(str(tmp_path), name, (1, 3), evaluate=base, **kw)
    off = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(base, refine=False), **kw)
    got = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(base, refine=True), **kw)
    assert set(got) == set(old) and repr(got["evaluation"]) == repr(old["evaluation"]), "the scoring is what it was"
    for sp in (1, 3):
        _same_value(off["odometry"][sp], old["odometry"][sp], f"spacing {sp}: refine False")
        assert "refine" not in old["odometry"][sp] and "ransac" not in old["odometry"][sp]
        direct = od.odometry_result(pipe, got, depth=depth, camera=cam, poses=tum.poses, spacing=sp, num_pairs=4, threshold=20.0, refine=True)
        _same_value(got["odometry"][sp], direct, f"spacing {sp}")
        for key in got["odometry"][sp]["ransac"]:
            _same_value(got["odometry"][sp]["ransac"][key], old["odometry"][sp][key], ("ransac", key))
        assert set(got["odometry"][sp]) == set(old["odometry"][sp]) | {"ransac", "refine"}


def test_drop_in_refine_relative_pose_equals_the_restatement(T):
    import evaluation as dropin
    import pose_ransac_cases as rc
    c = rc.case("k300_n257")
    cam, p = c["cam"], 2
    a, b = c["first"][p], c["second"][p]
    # depth images that hold every keypoint's depth under it (scale 1: the keypoints are in depth pixels), as tests/test_gpu_pose_ransac.py builds them
    imgs = np.zeros((2, cam.height, cam.width), np.uint16)
    px = np.floor(c["bank"][[a, b]].astype(np.float64) + 0.5).astype(np.int64)
    inside = (px[..., 0] >= 0) & (px[..., 0] < cam.width) & (px[..., 1] >= 0) & (px[..., 1] < cam.height)
    kd = np.where(inside & (c["depth_bank"][[a, b]] > 0), c["depth_bank"][[a, b]], 0)
    for f in range(2):
        order = np.arange(px.shape[1])[::-1]              # the lowest index wins a shared pixel
        imgs[f, px[f, order, 1].clip(0, cam.height - 1), px[f, order, 0].clip(0, cam.width - 1)] = np.where(inside[f, order], kd[f, order], 0)
    seen = np.stack([np.where(inside[f], imgs[f, px[f, :, 1].clip(0, cam.height - 1), px[f, :, 0].clip(0, cam.width - 1)].astype(np.int32), -1)
                     for f in range(2)])      # what sslam_keypoint_depth reads: -1 outside the image
    cnt = int(np.clip(c["count"][p], 0, c["n1"]))
    start = rr.ransac(c["bank"][a], c["bank"][b], seen[0], seen[1], c["matches"][p][:cnt], cnt, cam, 3.0, 128, 9)["T"]
    for T_in, thr, huber, its in ((start, 3.0, None, 5), (cases._initial("prior", dict(first=[0], planted=c["planted"][p:p + 1]), None)[0], 60.0, 20.0, 16)):
        want = fr.refine(c["bank"][a], c["bank"][b], seen[0], seen[1], c["matches"][p][:cnt], cnt, cam, thr, thr / 3 if huber is None else huber, its, T_in)
        T4 = np.eye(4)
        T4[:3] = T_in.reshape(3, 4)
        Tm, mask, info = dropin.refine_relative_pose(c["bank"][a], c["bank"][b], imgs[0], imgs[1], c["matches"][p][:cnt], T4, cam, thr, huber, its)
        assert Tm.shape == (4, 4) and Tm[:3].tobytes() == want["T"].reshape(3, 4).tobytes() and np.array_equal(Tm[3], [0, 0, 0, 1.0])
        assert mask.dtype == bool and mask.shape == (cnt,) and np.array_equal(mask, want["inlier_of_slot"] == 1) and mask.sum() >= 50
        assert info.shape == (6, 6) and info.tobytes() == fr.full_info(want["info"]).tobytes() and want["status"] == 0
        Tm34, _, _ = dropin.refine_relative_pose(c["bank"][a], c["bank"][b], imgs[0], imgs[1], c["matches"][p][:cnt], T4[:3], cam, thr, huber, its)
        assert Tm34.tobytes() == Tm.tobytes(), "(3, 4) is taken as well"
