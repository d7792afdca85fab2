"""GPU tests of the relative pose from matches and depth: sslam_pose_ransac_pairs through sslam_amd.lib,
SequencePipeline.estimate_poses, sslam_amd.odometry, online.PoseFrameStepper, run_directory(evaluate={"odometry": True}) and the
drop-in estimate_relative_pose.

Reference: the float64 restatement of tests/pose_ransac_ref.py on the seeded cases of tests/pose_ransac_cases.py, which
tests/test_pose_ransac_cpu.py holds to their margins and to the planted motions.  EVERY output is compared bit for bit, T and rms
included (pose_ransac_ref's docstring says why no tolerance is needed).  Every launch goes into poisoned outputs between guard
bands (tests/guarded.py) with the inputs between NaN bands; inputs are compared with their host copies after the call; launches
are counted."""
import ctypes as C

import numpy as np
import pytest

import guarded
import pose_ransac_cases as cases
import pose_ransac_ref as rr

pytestmark = pytest.mark.gpu

CASE_SEEDS = [(name, seed) for name in cases.NAMES for seed in cases.seeds_of(name)]


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
    shapes, out = lib.pose_ransac_shapes(n_pairs, n1), {}
    for key in lib.POSE_RANSAC_KEYS:
        shape, dt = shapes[key]
        whole, mid = guarded.guarded(T, shape, T.int64 if dt == T.float64 else dt, name=key)
        out[key] = (whole, mid, mid.view(T.float64) if dt == T.float64 else mid)
    return out


INPUTS = ("bank", "depth_bank", "first", "second", "matches", "count")
ARG = dict(bank="kp_bank", depth_bank="kp_depth_bank", first="pair_first", second="pair_second", matches="matches", count="count")      # include/sslam_hip.h


def _inputs(T, c):
    """The case's inputs between NaN-bit bands: {key: (whole, middle)}."""
    return {key: guarded.guarded_input(T, c[key], name=ARG[key]) for key in INPUTS}


def run_case(T, c, seed, n_hyp=None, threshold=None):
    """sslam_pose_ransac_pairs on a case, one launch into poisoned, guarded outputs -> dict of numpy arrays."""
    from sslam_amd import lib
    ins = _inputs(T, c)
    out = _outputs(T, len(c["first"]), c["n1"])
    n0 = lib.launch_count()
    lib.pose_ransac_pairs(*(ins[key][1] for key in INPUTS), c["cam"], c["scale_x"], c["scale_y"], c["threshold"] if threshold is None else threshold,
                          c["n_hyp"] if n_hyp is None else n_hyp, seed, out=tuple(out[key][2] for key in lib.POSE_RANSAC_KEYS))
    assert lib.launch_count() - n0 == 1, "one launch"
    got = {}
    for key, (whole, mid, t) in out.items():
        guarded.assert_guards(whole, mid, f"pose_ransac_pairs {key}")
        guarded.assert_written(mid, f"pose_ransac_pairs {key}")
        got[key] = t.cpu().numpy()
    for key, (whole, mid) in ins.items():
        guarded.assert_guards(whole, mid, f"input {key}")
        assert np.array_equal(mid.cpu().numpy(), c[key]), f"input {key} was written"
    return got


def same_bits(got, want, where):
    for key in rr.KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (where, key)
        if got[key].tobytes() != want[key].tobytes():
            bad = np.argwhere((got[key].view(np.int64) if got[key].dtype == np.float64 else got[key]) !=
                              (want[key].view(np.int64) if want[key].dtype == np.float64 else want[key]))
            at = tuple(bad[0])
            raise AssertionError(f"{where} {key}: {len(bad)} elements differ; the first at {at}: device {got[key][at]!r}, restatement {want[key][at]!r}")


# ------------------------------------------------------------------------------------------------- 1. the restatement, bit for bit
@pytest.mark.parametrize("name,seed", CASE_SEEDS)
def test_every_output_equals_the_restatement_bit_for_bit(T, name, seed):
    c = cases.case(name)
    got = run_case(T, c, seed)
    want = cases.expected(name, seed)
    for p in range(len(c["first"])):
        print(f"{name} seed {seed:#x} pair {p}: inliers {got['inlier_count'][p]} / {want['inlier_count'][p]} of {got['usable_count'][p]} usable, "
              f"h {got['best_hypothesis'][p]} / {want['best_hypothesis'][p]}, refit {got['refit_kept'][p]}, rms {got['rms'][p]!r} / {want['rms'][p]!r}, "
              f"max |T - T'| {np.abs(got['T'][p] - want['T'][p]).max():.3e}")
    same_bits(got, want, f"{name} seed {seed:#x}")
    again = run_case(T, c, seed)
    for key in rr.KEYS:
        assert got[key].tobytes() == again[key].tobytes(), f"{name} {key}: the same call twice gave other bits"


def test_other_hypothesis_counts_on_one_case(T):
    """The 70-pair case under every hypothesis count of the list (its own is 64): the partly filled round, the second round."""
    c = cases.case("k64_p70")
    for n_hyp in (1, 63, 65, 256, 1024):
        got = run_case(T, c, cases.SEEDS[1], n_hyp=n_hyp)
        want = rr.stacked(rr.ransac_pairs(c["bank"], c["depth_bank"], c["first"], c["second"], c["matches"], c["count"], c["cam"], c["threshold"],
                                          n_hyp, cases.SEEDS[1]))
        same_bits(got, want, f"k64_p70 with {n_hyp} hypotheses")


# ------------------------------------------------------------------------------------------------------------- 2. refusals
def test_every_refusal_returns_its_code_and_writes_nothing(T):
    from sslam_amd import lib
    c = cases.case("k5_dup")
    P, n1, k = len(c["first"]), c["n1"], c["bank"].shape[1]
    ins = {key: _dev(T, c[key]) for key in INPUTS}
    out = _outputs(T, P, n1)
    cam = c["cam"]
    base = dict(kp_bank=ins["bank"].data_ptr(), kp_depth_bank=ins["depth_bank"].data_ptr(), n_bank=len(c["bank"]), K=k,
                pair_first=ins["first"].data_ptr(), pair_second=ins["second"].data_ptr(), n_pairs=P, matches=ins["matches"].data_ptr(),
                count=ins["count"].data_ptr(), n1=n1, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, depth_scale=cam.depth_scale,
                scale_x=c["scale_x"], scale_y=c["scale_y"], view_w=float(cam.width), view_h=float(cam.height), threshold=3.0, n_hyp=16, seed=1)
    base.update({key: out[key][2].data_ptr() for key in lib.POSE_RANSAC_KEYS})
    pointers = ("kp_bank", "kp_depth_bank", "pair_first", "pair_second", "matches", "count") + lib.POSE_RANSAC_KEYS
    doubles = ("fx", "fy", "cx", "cy", "depth_scale", "scale_x", "scale_y", "view_w", "view_h", "threshold")

    def call(**change):
        a = dict(base, **change)
        conv = lambda key: C.c_void_p(a[key]) if key in pointers else C.c_double(a[key]) if key in doubles else \
            C.c_uint64(a[key]) if key == "seed" else int(a[key])
        with T.cuda.device(0):
            return lib.lib().sslam_pose_ransac_pairs(*(conv(key) for key in base), C.c_void_p(T.cuda.current_stream().cuda_stream))

    refused = [({key: None}, lib.E_INVALID) for key in pointers]                                       # NULL
    refused += [({key: base[key] + 2}, lib.E_INVALID) for key in pointers]                             # misaligned (2 bytes off)
    refused += [({key: v}, lib.E_INVALID) for key in ("n_bank", "K", "n_pairs", "n1") for v in (0, -1)]
    refused += [(dict(n1=k + 1), lib.E_INVALID), (dict(n_hyp=0), lib.E_INVALID), (dict(n_hyp=-3), lib.E_INVALID),
                (dict(n_hyp=lib.POSE_MAX_HYP + 1), lib.E_INVALID)]
    refused += [(dict(threshold=v), lib.E_INVALID) for v in (-1.0, float("nan"), float("inf"))]
    refused += [({key: v}, lib.E_INVALID) for key in ("fx", "fy", "depth_scale", "scale_x", "scale_y", "view_w", "view_h")
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
    T.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the layers above the entry
E2E_THRESHOLD = 12.0        # px: the selector's keypoints sit on the 16-px patch grid; what suits real data nobody has measured
E2E_HYP, E2E_SEED = 64, 5


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


def _same_odometry(a, b, what):
    assert list(a) == list(b), what
    for key in a:
        if key == "pairs":
            assert a[key] == b[key], (what, key)
        elif isinstance(a[key], dict) or a[key] is None:
            assert repr(a[key]) == repr(b[key]), (what, key)
        else:
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (what, key)


def test_estimate_poses_on_a_permuted_pair_list_gives_the_permuted_rows(T, seq):
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
        n0 = lib.launch_count()
        out = pipe.estimate_poses(ex["keypoints_pixel"], kd, f, sec, mm, s["cam"], E2E_THRESHOLD, E2E_HYP, E2E_SEED)
        assert lib.launch_count() - n0 == 1, "one launch, nothing else"
        return {key: v.cpu().numpy() for key, v in out.items()}
    a, b = run(first, second), run([first[i] for i in perm], [second[i] for i in perm])
    for key in lib.POSE_RANSAC_KEYS:
        assert a[key][perm].tobytes() == b[key].tobytes(), f"{key}: a pair's row depends on its place in the list"
    assert a["T"][0].tobytes() == a["T"][6].tobytes() and a["best_hypothesis"][3] == -1
    assert (a["inlier_count"][[0, 1, 2]] >= 3).all(), "the sequence has poses to estimate"
    ranked = pipe.rank_matches(pipe.match_pairs(ex["descriptors"], ex["scores"], first=first, second=second, rule=s["rule"]), 100, rule=s["rule"])
    r = pipe.estimate_poses(ex["keypoints_pixel"], kd, first, second, ranked, s["cam"], E2E_THRESHOLD, E2E_HYP, E2E_SEED)
    assert tuple(r["inlier_of_slot"].shape) == (7, 100) and int(r["usable_count"].max()) <= 100, "rank_matches' output is a match list too"


def test_odometry_and_odometry_result_agree(T, seq):
    from sslam_amd import odometry as od
    from sslam_amd.harness import StreamingSequence
    s = seq
    kw = dict(camera=s["cam"], poses=s["poses"], threshold=E2E_THRESHOLD, hypotheses=E2E_HYP, seed=E2E_SEED)
    result = StreamingSequence(s["pipe"], (1, 5), rule=s["rule"]).run(s["toks"])
    for spacing, num_pairs in ((1, None), (5, 4)):
        a = od.odometry(s["pipe"], tokens=s["toks"], depth=s["depth"], spacing=spacing, num_pairs=num_pairs, rule=s["rule"], **kw)
        b = od.odometry_result(s["pipe"], result, depth=T.from_numpy(s["depth"]).cuda(), spacing=spacing, num_pairs=num_pairs, **kw)
        _same_odometry(a, b, f"spacing {spacing}")
        p = len(a["pairs"])
        assert a["T"].shape == (p, 4, 4) and a["inlier_ratio"].shape == (p,) and ("trajectory" in a) == (spacing == 1)
        assert np.array_equal(a["inlier_ratio"], a["inlier_count"] / a["match_count"]) and (a["inlier_count"] <= a["usable_count"]).all()
        assert list(a["rpe"]) == ["translation", "rotation"] and (a["ate"] is None) == (spacing != 1)
        print(f"spacing {spacing}: inlier ratio {np.round(a['inlier_ratio'], 3)}, rpe {a['rpe']}, ate {a['ate']} (synthetic frames: no accuracy claim)")
    one = od.odometry(s["pipe"], tokens=s["toks"], depth=s["depth"], **dict(kw, poses=None))
    assert "rpe" not in one and "ate" not in one and np.array_equal(one["trajectory"][0], np.eye(4))
    assert np.abs(one["trajectory"] - od.chain(one["T"])).max() == 0.0


@pytest.mark.parametrize("use_graph", [False, True])
def test_pose_frame_stepper_equals_the_batched_odometry(T, seq, use_graph):
    from sslam_amd import lib
    from sslam_amd import odometry as od
    from sslam_amd.online import PoseFrameStepper
    s = seq
    n = 4
    want = od.odometry(s["pipe"], tokens=s["toks"][:n], depth=s["depth"][:n], camera=s["cam"], threshold=E2E_THRESHOLD, hypotheses=E2E_HYP,
                       seed=E2E_SEED)
    st = PoseFrameStepper(s["pipe"], 48, 64, 480, 640, camera=s["cam"], use_graph=use_graph, tokens_in=True, threshold=E2E_THRESHOLD,
                          hypotheses=E2E_HYP, seed=E2E_SEED)
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
        got = {key: v.cpu().numpy() for key, v in out["pose"].items()}
        assert got["T"].tobytes() == want["T"][i - 1][:3].tobytes(), f"frame {i}: T"
        for key in ("inlier_count", "usable_count", "best_hypothesis", "refit_kept"):
            assert int(got[key]) == want[key][i - 1], (i, key)
        assert got["rms"].tobytes() == want["rms"][i - 1].tobytes() and int(out["match_count"]) == want["match_count"][i - 1]
        assert got["inlier_of_slot"].shape == (s["k"],) and (got["inlier_of_slot"] == 1).sum() == want["inlier_count"][i - 1]
    assert (want["inlier_count"] >= 3).all()
    st.reset()
    assert st.step(image, depth[0], s["toks"][0])["pose"] is None
    with pytest.raises(ValueError, match="depth_u16"):
        st.step(image, depth[0, :100], s["toks"][0])


def test_run_directory_adds_the_odometry_and_only_when_asked(T, tmp_path):
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
    base = dict(num_pairs=4, threshold=20.0, depth=True, camera=cam)
    old = run_directory(str(tmp_path), name, (1, 3), evaluate=base, **kw)
    got = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(base, odometry=True), **kw)
    assert "odometry" not in old and set(got) == set(old) | {"odometry"} and set(got["odometry"]) == {1, 3}
    assert repr(got["evaluation"]) == repr(old["evaluation"]), "the scoring is what it was"
    alone = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(num_pairs=4, threshold=20.0, odometry=True, camera=cam), **kw)
    plain = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(num_pairs=4, threshold=20.0), **kw)
    assert repr(alone["evaluation"]) == repr(plain["evaluation"]) and "odometry" not in plain
    for sp in (1, 3):
        direct = od.odometry_result(pipe, got, depth=depth, camera=cam, poses=tum.poses, spacing=sp, num_pairs=4, threshold=20.0)
        _same_odometry(got["odometry"][sp], direct, f"spacing {sp}")
        _same_odometry(alone["odometry"][sp], direct, f"spacing {sp}, odometry alone")
        assert len(direct["pairs"]) == 4 and ("trajectory" in direct) == (sp == 1)


def test_drop_in_estimate_relative_pose_equals_the_restatement(T):
    import evaluation as dropin
    c = cases.case("k300_n257")
    cam, p = c["cam"], 2
    a, b = c["first"][p], c["second"][p]
    # depth images that hold every keypoint's depth under it (scale 1: the keypoints are in depth pixels)
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
    assert seen.dtype == np.int32 and (seen == -1).any()
    want = rr.ransac(c["bank"][a], c["bank"][b], seen[0], seen[1], c["matches"][p][:cnt], cnt, cam, 3.0, 128, 9)
    Tm, mask = dropin.estimate_relative_pose(c["bank"][a], c["bank"][b], imgs[0], imgs[1], c["matches"][p][:cnt], cam, 3.0, 128, 9)
    assert Tm.shape == (4, 4) and Tm[:3].tobytes() == want["T"].reshape(3, 4).tobytes() and np.array_equal(Tm[3], [0, 0, 0, 1.0])
    assert mask.dtype == bool and mask.shape == (cnt,) and np.array_equal(mask, want["inlier_of_slot"] == 1) and mask.sum() >= 50
