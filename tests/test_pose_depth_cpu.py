"""The depth ground truth of the scoring stage (sslam_keypoint_depth, sslam_pose_depth_nn_pairs, sslam_match_score_known_pairs;
csrc/evaluate.hip) as far as a machine without a GPU can see it: the margins every seeded case of tests/pose_depth_cases.py
keeps from each decision, the restatement of tests/pose_depth_ref.py against closed forms, and the Python layer - the header, the
refusals of the three C entries (which come before any launch), the bindings' argument checks, relative_transform, camera_for,
load_depth_raw, the summaries' arithmetic and evaluate(depth=)'s argument errors.

Tolerances: the docstring of tests/pose_depth_ref.py.  Closed forms are held to 1e-9 px: a projected coordinate below 4096 px
carries about ten roundings of 2^-53 relative, 5e-12 px, on either side of the comparison.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pose_depth_cases as cases
import pose_depth_ref as dr
import pose_eval_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
P = [0x10000 * (i + 1) for i in range(16)]       # never dereferenced: every call below is refused before the launch
CLOSED = 1e-9


# ------------------------------------------------------------------------------------------------------------ the case lists
def test_gather_cases_keep_their_margin_and_cover_what_they_must():
    cs = cases.gather_cases()
    assert {(c["depth"].shape[1:], c["kp"].shape[1], c["depth"].shape[0]) for c in cs} >= {((6, 8), 5, 1), ((6, 8), 70, 3), ((480, 640), 5, 3),
                                                                                         ((480, 640), 70, 1)}
    assert {(c["scale_x"], c["scale_y"]) for c in cs} >= {(1.0, 1.0), (640 / 448, 480 / 448)}
    for c in cs:
        assert dr.gather_margin(c["kp"][~c["exact"]], c["scale_x"], c["scale_y"]) >= cases.MARGIN, c["name"]
        got = dr.keypoint_depth(c["depth"], c["kp"], c["scale_x"], c["scale_y"])
        assert got.dtype == np.int32 and got.shape == c["kp"].shape[:2]
        assert (got == -1).any() and (got >= 0).any(), c["name"]
        if c["scale_x"] == 1.0:
            h, w = c["depth"].shape[1:]
            assert got[0, 0] == 65535 == c["depth"][0, 2, 3], "x = 2.5 rounds to column 3, y = 1.5 to row 2"
            assert got[0, 1] == -1 and got[0, 2] == -1 and got[0, 3] == -1, "left of the image, column w, NaN"
            assert got[0, 4] == 0 == c["depth"][0, 0, 0], "a raw 0 stays 0"
            if c["kp"].shape[1] >= 12:
                assert list(got[0, 5:12]) == [-1, -1, -1, -1, c["depth"][0, 1, 0], 65535, c["depth"][0, 1, 1]]


@pytest.mark.parametrize("index", range(len(cases.WARP_SIZES)))
def test_warp_cases_keep_their_margins(index):
    c = cases.warp_case(index)
    m = cases.check_margins(c)
    print(c["name"], m)
    assert cases.margins_ok(m), (c["name"], m)
    want = dr.pose_depth_nn_pairs(c["bank"], c["depth_bank"], c["first"], c["second"], c["T"], c["cam"], c["threshold"], c["scale_x"],
                                  c["scale_y"], c["n1"], c["n2"])
    if c["bank"].shape[1] >= 64:
        assert 0 < want[0]["gt_count"] < want[0]["valid_count"] < c["n1"], "kept rows, rows beyond the threshold and invalid rows"
        rows = want[0]["gt_of_row"]
        assert rows[1] == -2 and rows[2] == -2 and rows[3] == -2, "depth 0, depth -1, out of view"
    if len(c["first"]) == 8:
        k = c["n1"]
        assert want[1]["valid_count"] == 0 and (want[1]["gt_of_row"] == -1).all(), "an absent pair"
        assert want[6]["valid_count"] == 0 and (want[6]["gt_of_row"] == -1).all(), "a second frame outside the bank"
        assert want[5]["valid_count"] == 0 and (want[5]["gt_of_row"] == -2).all() and want[5]["dist_median"] == 0.0, "the 180 degree turn"
        assert all(np.array_equal(want[0][key], want[3][key]) for key in ("gt_matches", "gt_of_row")), "a pair listed twice"
        same = want[2]                                                    # a frame against itself under the identity
        for i in np.where(same["valid"][:c["n2"]])[0]:                    # the rows that are among the candidates
            j = same["gt_of_row"][i]
            assert j <= i and np.array_equal(c["bank"][0, j], c["bank"][0, i]), "itself or its lowest-index duplicate"
        if k >= 6 and k == c["bank"].shape[1] == c["n2"]:
            assert same["gt_of_row"][k - 1] == 1, "row k - 1 duplicates row 1 and has a depth of its own: the lowest index, though row 1 has no depth"
            assert same["gt_of_row"][1] == -2 and same["gt_of_row"][k - 2] == 0, "row k - 2 duplicates row 0, which has a depth"


def test_homography_cases_hold_what_the_comparison_rests_on():
    for c in cases.homography_cases():
        cond = cases.homography_conditions(c)
        print(c["name"], cond)
        assert cond["inside"] and cond["ratio"] >= 0.5 and cond["hom"] >= cases.MARGIN and cases.margins_ok(cond["depth"])
        worst = 0.0
        for p in range(len(c["first"])):                                  # the two evaluation orders of one quantity
            a = dr.project(c["bank"][0], c["depth_bank"][0], c["T"][p], c["cam"], c["scale_x"], c["scale_y"])["warped"]
            b = pr.warp(c["bank"][0], c["H"][p])
            worst = max(worst, float(np.abs(a - b).max()))
        print(f"{c['name']}: depth warp against homography, worst {worst:.3e} px")
        assert worst <= CLOSED


def test_translation_case_is_what_it_claims():
    c = cases.translation_case()
    assert cases.margins_ok(cases.check_margins(c))
    w = dr.pose_depth_nn(c["bank"][0], c["bank"][1], c["depth_bank"][0], c["T"][0], c["cam"], 1e-2)
    assert 0.5 * cases.TRANSLATION_K < w["valid_count"] < cases.TRANSLATION_K and w["gt_count"] == w["valid_count"]
    assert np.array_equal(w["gt_of_row"][w["valid"]], np.where(w["valid"])[0])
    h = pr.pose_nn(c["bank"][0], c["bank"][1], c["H"][0], 3.0)
    print(f"translation case: depth ground truth {w['gt_count']} of {w['valid_count']} valid rows at 0.01 px; homography {h['gt_count']} at 3 px")
    assert h["gt_count"] < w["gt_count"]


# ------------------------------------------------------------------------------------------- the restatement, closed forms
def test_restatement_equals_closed_forms():
    cam = dr.Cam()
    kp = np.array([[319.5, 239.5], [100.25, 50.75], [600.0, 400.0], [10.0, 470.0]], np.float32)
    d = np.array([5000, 10000, 2500, 20000], np.int32)                    # 1, 2, 0.5, 4 m
    z = d / 5000.0
    # the identity returns the keypoint
    pj = dr.project(kp, d, dr.rigid(np.eye(3), [0, 0, 0]), cam)
    assert pj["valid"].all() and np.abs(pj["warped"] - kp).max() <= CLOSED and np.array_equal(pj["Z2"], z)
    # a sideways translation t moves u by fx t / z and leaves v
    pj = dr.project(kp, d, dr.rigid(np.eye(3), [0.1, 0, 0]), cam)
    assert np.abs(pj["u2"] - (kp[:, 0] + 525.0 * 0.1 / z)).max() <= CLOSED and np.abs(pj["v2"] - kp[:, 1]).max() <= CLOSED
    assert list(pj["valid"]) == [True, True, False, True], "600 + 105 leaves the 640-pixel view"
    # a forward translation scales about the principal point by z / (z + t)
    pj = dr.project(kp, d, dr.rigid(np.eye(3), [0, 0, 0.5]), cam)
    assert np.abs(pj["u2"] - (319.5 + (kp[:, 0] - 319.5) * z / (z + 0.5))).max() <= CLOSED
    # a turn by theta about y takes the principal ray to cx + fx tan(theta), whatever the depth
    th = np.deg2rad(10.0)
    pj = dr.project(kp[:1], d[:1], dr.rigid(dr.rotation([0, 1, 0], th), [0, 0, 0]), cam)
    assert abs(pj["u2"][0] - (319.5 + 525.0 * np.tan(th))) <= CLOSED and abs(pj["v2"][0] - 239.5) <= CLOSED
    # keypoint units: a 448-pixel pipeline's keypoint (224, 224) is the depth pixel (320, 240)
    sx, sy = cases.SCALE_448
    pj = dr.project(np.array([[224.0, 224.0]], np.float32), d[:1], dr.rigid(np.eye(3), [0, 0, 0]), cam, sx, sy)
    assert np.abs(pj["warped"] - 224.0).max() <= CLOSED and abs(pj["u2"][0] - 320.0) <= CLOSED and abs(pj["v2"][0] - 240.0) <= CLOSED
    # the rows without ground truth
    turn = dr.rigid(dr.rotation([0, 1, 0], np.pi), [0, 0, 0])
    assert not dr.project(kp, d, turn, cam)["valid"].any(), "Z' = -z"
    assert list(dr.project(kp[:3], np.array([0, -1, 1], np.int32), dr.rigid(np.eye(3), [0, 0, 0]), cam)["valid"]) == [False, False, True]
    edge = np.array([[-0.4375, 0.0], [639.4375, 479.4375], [639.5625, 10.0], [10.0, 479.5625], [-0.5625, 10.0]], np.float32)
    assert list(dr.project(edge, np.full(5, 5000, np.int32), dr.rigid(np.eye(3), [0, 0, 0]), cam)["valid"]) == [True, True, False, False, False]
    nanT = dr.rigid(np.eye(3), [0, 0, np.nan])
    assert not dr.project(kp, d, nanT, cam)["valid"].any(), "a NaN Z' is not > 0"


def test_restated_search_counts_and_median():
    cam = dr.Cam()
    kp1 = np.array([[100, 100], [200, 100], [300, 100], [400, 100], [500, 100], [100, 100]], np.float32)
    kp2 = kp1 + np.array([[3, 4], [0, 1], [30, 40], [0, 2], [0, 0], [3, 4]], np.float32)        # distances 5, 1, 50, 2, 0, 5
    kp2[5] = kp2[0]                                                        # a duplicate candidate: index 0 wins
    d = np.array([5000, 5000, 5000, 0, -1, 5000], np.int32)
    w = dr.pose_depth_nn(kp1, kp2, d, dr.rigid(np.eye(3), [0, 0, 0]), cam, 3.0)
    assert list(w["gt_of_row"]) == [-1, 1, -1, -2, -2, -1] and w["valid_count"] == 4 and w["gt_count"] == 1
    assert np.array_equal(w["gt_matches"], [[1, 1]] + [[0, 0]] * 5)
    assert abs(w["dist_sum"] - 61.0) <= CLOSED and abs(w["dist_median"] - 5.0) <= CLOSED, "sorted 1, 5, 5, 50: the middle two"
    w = dr.pose_depth_nn(kp1, kp2, d, dr.rigid(np.eye(3), [0, 0, 0]), cam, 6.0)
    assert list(w["gt_of_row"]) == [0, 1, -1, -2, -2, 0], "rows 0 and 5 both take the LOWEST of the two equal candidates"
    w = dr.pose_depth_nn(kp1[:3], kp2, d[:3], dr.rigid(np.eye(3), [0, 0, 0]), cam, 3.0)
    assert abs(w["dist_median"] - 5.0) <= CLOSED, "an odd count: the middle value twice"
    w = dr.pose_depth_nn(kp1, kp2, np.zeros(6, np.int32), dr.rigid(np.eye(3), [0, 0, 0]), cam, 3.0)
    assert (w["valid_count"], w["gt_count"], w["dist_sum"], w["dist_median"]) == (0, 0, 0.0, 0.0) and (w["gt_of_row"] == -2).all()
    a = dr.absent(4)
    assert a["valid_count"] == 0 and (a["gt_of_row"] == -1).all() and a["dist_median"] == 0.0


def test_restated_known_score():
    row = np.array([2, -2, -1, 0, -2], np.int32)
    pred = [[0, 2], [1, 3], [2, 0], [3, 1], [4, -2], [9, 0], [-1, 0]]
    tp, fp, fn, un, vs = dr.match_score_known(pred, [0.5] * 7, row, 2)
    assert (tp, fp, fn, un, vs) == (1, 4, 1, 2, 3.5), "a row on -2 is unknown whatever idx2 says; idx1 outside is a false positive"
    c = cases.score_case()
    assert (c["gt_of_row"] == -2).any() and (c["gt_of_row"] == -1).any() and (c["gt_of_row"] >= 0).any() and not (c["plain"] == -2).any()
    for p in range(len(c["count"])):
        n = int(np.clip(c["count"][p], 0, c["n1"]))
        tp, fp, fn, un, _ = dr.match_score_known(c["matches"][p, :n], c["value"][p, :n], c["gt_of_row"][p], c["gt_count"][p])
        assert tp + fp + un == n and min(tp, fp, un) >= 0
        tp2, fp2, fn2, _ = pr.match_score(c["matches"][p, :n], c["value"][p, :n], c["plain"][p], c["gt_count"][p])
        assert (tp2, fn2) == (tp, fn) and fp2 == fp + un, "without -2 the unknown rows are the older entry's false positives"
    assert dr.match_score_known(c["matches"][0], c["value"][0], c["gt_of_row"][0], c["gt_count"][0])[3] > 0


# ------------------------------------------------------------------------------------------------------------ host functions
def test_relative_transform_is_inverse_b_times_a_in_float64():
    from sslam_amd import evaluation as ev
    poses = pr.golden()["seq_poses"]
    a, b = poses[2], poses[7]
    T = ev.relative_transform(a, b)
    assert T.dtype == np.float64 and T.shape == (4, 4) and np.array_equal(T, np.linalg.inv(b) @ a)
    assert not np.array_equal(T, T.astype(np.float32).astype(np.float64)), "not rounded to float32"
    x_a = np.array([0.3, -0.2, 1.5, 1.0])
    assert np.abs(b @ (T @ x_a) - a @ x_a).max() <= 1e-12, "camera-to-world poses: the same world point from both cameras"
    assert not np.allclose(T, ev.relative_pose(a, b).astype(np.float64), atol=1e-4), "the reference's pose2 @ inv(pose1) is another map"
    assert "relative_pose" in ev.relative_transform.__doc__ and "deliberately" in ev.relative_transform.__doc__
    pt = ev.pair_transforms(poses, [(2, 7), (0, 0)])
    assert pt.shape == (2, 3, 4) and pt.dtype == np.float64 and np.array_equal(pt[0], T[:3])
    assert np.abs(pt[1] - np.eye(4)[:3]).max() <= 1e-15
    assert ev.pair_transforms(poses, []).shape == (0, 3, 4)
    with pytest.raises(ValueError):
        ev.relative_transform(a[:3], b)
    with pytest.raises(ValueError):
        ev.pair_transforms(poses, [(0, 12)])
    with pytest.raises(ValueError):
        ev.pair_transforms(poses[0], [(0, 0)])
    c = ev.Camera()
    assert (c.fx, c.fy, c.cx, c.cy, c.depth_scale, c.width, c.height) == (525.0, 525.0, 319.5, 239.5, 5000.0, 640, 480)


def test_camera_for_names_the_calibrated_intrinsics():
    from sslam_amd import evaluation as ev
    from sslam_amd.tum import camera_for
    assert camera_for("rgbd_dataset_freiburg1_xyz") == ev.Camera(fx=517.3, fy=516.5, cx=318.6, cy=255.3)
    assert camera_for("/data/tum/rgbd_dataset_freiburg2_desk") == ev.Camera(fx=520.9, fy=521.0, cx=325.1, cy=249.7)
    assert camera_for("rgbd_dataset_freiburg3_long_office_household") == ev.Camera(fx=535.4, fy=539.2, cx=320.1, cy=247.6)
    assert camera_for("synthetic") == ev.Camera() and camera_for("") == ev.Camera()
    c = camera_for("rgbd_dataset_freiburg1_desk")
    assert (c.depth_scale, c.width, c.height) == (5000.0, 640, 480)


def test_load_depth_raw_reads_the_pngs_as_they_are(tmp_path):
    from PIL import Image

    from sslam_amd.tum import TUMSequence
    os.makedirs(tmp_path / "rgb")
    os.makedirs(tmp_path / "depth")
    rng = np.random.default_rng(5)
    want = rng.integers(0, 65536, (3, 6, 8)).astype(np.uint16)
    want[1, 2, 3], want[2, 0, 0] = 0, 65535
    for i in (2, 0, 1):                                                   # written out of order: the reader sorts by name
        Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(tmp_path / "rgb" / f"100.{i}00000.png")
        Image.fromarray(want[i]).save(tmp_path / "depth" / f"100.{i}00500.png")
    tum = TUMSequence(str(tmp_path))
    got = tum.load_depth_raw(range(3))
    assert got.dtype == np.uint16 and got.shape == (3, 6, 8) and np.array_equal(got, want)
    assert np.array_equal(tum.load_depth_raw([2, 0]), want[[2, 0]])
    assert np.array_equal(tum.load_depth(1), want[1].astype(np.float32) / 5000.0), "the metre form is unchanged"
    with pytest.raises(ValueError, match="cover"):
        tum.load_depth_raw([3])
    os.makedirs(tmp_path / "bare" / "rgb")
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(tmp_path / "bare" / "rgb" / "1.0.png")
    with pytest.raises(ValueError, match="no depth"):
        TUMSequence(str(tmp_path / "bare")).load_depth_raw([0])


def test_depth_summaries_arithmetic_and_zero_denominators():
    from sslam_amd import evaluation as ev
    st = dict(num_keypoints=8, gt_count=[2, 0, 3], valid_count=[4, 0, 6], dist_sum=[10.0, 0.0, 3.0], dist_median=[2.5, 0.0, 0.5],
              tp=[1, 0, 2], fp=[1, 0, 0], fn=[1, 0, 1], unknown=[2, 3, 0], value_sum=[1.0, 0.75, 0.5], match_count=[4, 3, 2])
    r = ev.depth_repeatability_summary(st, "s")
    assert list(r) == ["sequence", "num_pairs", "pairs_without_ground_truth", "mean_repeatability", "std_repeatability", "median_repeatability",
                       "min_repeatability", "max_repeatability", "mean_distance", "median_distance", "all_results"]
    assert (r["num_pairs"], r["pairs_without_ground_truth"]) == (3, 1)
    assert [x["repeatability"] for x in r["all_results"]] == [0.5, 0.0, 0.5] and [x["valid_keypoints"] for x in r["all_results"]] == [4, 0, 6]
    assert [x["mean_nn_distance"] for x in r["all_results"]] == [2.5, 0.0, 0.5] and r["all_results"][0]["total_keypoints"] == 8
    assert list(r["all_results"][0]) == ["repeatability", "repeatable_count", "total_keypoints", "valid_keypoints", "mean_nn_distance",
                                        "median_nn_distance"]
    assert r["mean_repeatability"] == 0.5 and r["mean_distance"] == 1.5 and r["min_repeatability"] == 0.5, "pair 1 is left out, not a zero"
    q = ev.depth_descriptor_quality_summary(st, "s")
    assert (q["num_pairs"], q["pairs_without_ground_truth"]) == (3, 1)
    a, b, c = q["all_results"]
    assert (a["tp"], a["fp"], a["fn"], a["num_unknown_matches"], a["num_pred_matches"], a["num_gt_matches"]) == (1, 1, 1, 2, 4, 2)
    assert a["inlier_ratio"] == 0.5 and a["precision"] == 0.5 and a["recall"] == 0.5 and a["mean_match_distance"] == 0.25
    assert b["inlier_ratio"] == 0.0 and b["precision"] == 0.0 and b["num_unknown_matches"] == 3, "3 matches, all unknown: 0 / 0 is 0.0"
    assert c["inlier_ratio"] == 1.0 and c["recall"] == 2 / 3 and c["valid_keypoints"] == 6
    assert q["mean_inlier_ratio"] == 0.75 and q["mean_num_matches"] == 3.0 and q["mean_match_distance"] == 0.25
    m = ev.known_match_metrics(0, 0, 0, 0, 0, 0)
    assert (m["precision"], m["recall"], m["f1"], m["inlier_ratio"], m["num_unknown_matches"]) == (0.0, 0.0, 0.0, 0.0, 0)
    none = dict(st, valid_count=[0, 0, 0])
    with pytest.raises(ValueError, match="ground truth"):
        ev.depth_repeatability_summary(none)
    with pytest.raises(ValueError, match="ground truth"):
        ev.depth_descriptor_quality_summary(none)
    with pytest.raises(ValueError):
        ev.depth_repeatability_summary({k: v for k, v in st.items() if k != "valid_count"})


def test_evaluate_with_depth_refuses_before_any_device_work():
    from sslam_amd import evaluation as ev
    from sslam_amd import harness, lib
    before = lib.launch_count()
    toks, poses = np.zeros((3, 5 + 4, 384), np.float32), np.stack([np.eye(4)] * 3)
    depth = np.zeros((3, 480, 640), np.uint16)
    with pytest.raises(ValueError, match="depth= needs poses"):
        ev.evaluate(None, None, None, tokens=toks, depth=depth, use_pose=False)
    with pytest.raises(ValueError, match="depth= needs poses"):
        ev.evaluate_result(None, {}, None, depth=depth, use_pose=False)
    with pytest.raises(ValueError, match="needs depth="):
        ev.evaluate(None, None, poses, tokens=toks, camera=ev.Camera())
    with pytest.raises(ValueError, match="use_pose=False"):
        ev.evaluate(None, None, poses, tokens=toks, depth=depth, use_pose=False)
    with pytest.raises(ValueError, match="uint16"):
        ev.evaluate(None, None, poses, tokens=toks, depth=depth.astype(np.float32))
    with pytest.raises(ValueError, match="uint16"):
        ev.evaluate(None, None, poses, tokens=toks, depth=depth[0])
    with pytest.raises(ValueError, match="frames"):
        ev.evaluate(None, None, poses, tokens=toks, depth=depth[:2])
    with pytest.raises(ValueError, match="camera describes"):
        ev.evaluate(None, None, poses, tokens=toks, depth=depth[:, :100])
    with pytest.raises(ValueError, match="camera fx"):
        ev.evaluate(None, None, poses, tokens=toks, depth=depth, camera=ev.Camera(fx=0.0))
    with pytest.raises(ValueError, match="camera must have"):
        ev.evaluate(None, None, poses, tokens=toks, depth=depth, camera=(525.0, 525.0))
    with pytest.raises(TypeError):
        ev.evaluate(None, None, poses, 1, 50, True, 0.9, 3.0, toks, "", depth)        # keyword-only
    with pytest.raises(ValueError, match="flag"):
        harness.run_directory("/nonexistent", evaluate={"depth": depth})
    with pytest.raises(ValueError, match='"depth": True'):
        harness.run_directory("/nonexistent", evaluate={"camera": ev.Camera()})
    assert lib.launch_count() == before


# ----------------------------------------------------------------------------------------------------------- the C entries
def _gather(L, depth=P[0], n=2, h=6, w=8, kp=P[1], K=5, sx=1.0, sy=1.0, out=P[2]):
    return L.sslam_keypoint_depth(depth, n, h, w, kp, K, ctypes.c_double(sx), ctypes.c_double(sy), out, None)


def _nn(L, kp=P[0], kd=P[1], n_bank=3, K=8, n1=8, n2=8, first=P[2], second=P[3], n_pairs=2, T=P[4], fx=525.0, fy=525.0, cx=319.5, cy=239.5,
        ds=5000.0, sx=1.0, sy=1.0, vw=640.0, vh=480.0, thr=3.0, gt=P[5], cnt=P[6], row=P[7], valid=P[8], dsum=P[9], dmed=P[10]):
    return L.sslam_pose_depth_nn_pairs(kp, kd, n_bank, K, n1, n2, first, second, n_pairs, T,
                                       *(ctypes.c_double(v) for v in (fx, fy, cx, cy, ds, sx, sy, vw, vh, thr)), gt, cnt, row, valid, dsum,
                                       dmed, None)


def _score(L, m=P[0], v=P[1], c=P[2], row=P[3], gtc=P[4], n1=8, n_pairs=2, tp=P[5], fp=P[6], fn=P[7], un=P[8], vs=P[9]):
    return L.sslam_match_score_known_pairs(m, v, c, row, gtc, n1, n_pairs, tp, fp, fn, un, vs, None)


def test_c_entries_refuse_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    before = lib.launch_count()
    nan, inf = float("nan"), float("inf")
    for kw in [dict(depth=None), dict(kp=None), dict(out=None), dict(n=0), dict(h=0), dict(w=-1), dict(K=0), dict(sx=0.0), dict(sy=-1.0),
               dict(sx=nan), dict(sy=inf), dict(depth=P[0] + 1), dict(kp=P[1] + 4), dict(out=P[2] + 2)]:
        assert _gather(L, **kw) == E_INVALID, kw
    assert _gather(L, n=1 << 20, K=1 << 12) == E_UNSUPPORTED
    bad = [dict(kp=None), dict(kd=None), dict(first=None), dict(second=None), dict(T=None), dict(gt=None), dict(cnt=None), dict(row=None),
           dict(valid=None), dict(dsum=None), dict(dmed=None), dict(n_bank=0), dict(K=0), dict(n1=0), dict(n2=0), dict(n1=9), dict(n2=9),
           dict(n_pairs=0), dict(thr=-3.0), dict(thr=nan), dict(thr=inf), dict(kp=P[0] + 4), dict(kd=P[1] + 2), dict(T=P[4] + 4),
           dict(first=P[2] + 2), dict(second=P[3] + 1)]
    for name in ("fx", "fy", "ds", "sx", "sy", "vw", "vh"):
        bad += [{name: 0.0}, {name: -1.0}, {name: nan}, {name: inf}]
    bad += [dict(cx=nan), dict(cy=inf)]
    for kw in bad:
        assert _nn(L, **kw) == E_INVALID, kw
    for kw in (dict(K=4097, n1=4097, n2=4097), dict(K=4097), dict(K=1 << 20, n1=500, n2=500)):
        assert _nn(L, **kw) == E_UNSUPPORTED, kw
    assert _nn(L, cx=-10.0, cy=0.0, K=5000, n1=5001) == E_INVALID, "n1 > K is an invalid argument at any K"
    for kw in [dict(m=None), dict(v=None), dict(c=None), dict(row=None), dict(gtc=None), dict(tp=None), dict(fp=None), dict(fn=None),
               dict(un=None), dict(vs=None), dict(n1=0), dict(n1=-1), dict(n_pairs=0)]:
        assert _score(L, **kw) == E_INVALID, kw
    assert _score(L, n1=4097) == E_UNSUPPORTED
    assert lib.launch_count() == before, "a refused call launches nothing"


def test_entries_are_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sslam_hip.h")).read()
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    for entry in ("sslam_keypoint_depth", "sslam_pose_depth_nn_pairs", "sslam_match_score_known_pairs"):
        assert re.search(r"^int\s+" + entry + r"\s*\(", hdr, flags=re.M), entry
        assert entry in lib.EXPORTS and re.search(r"\bT\s+" + entry + r"$", dyn, flags=re.M), entry
    L = lib.lib()
    assert L.sslam_version() > 620, "new entries raise the version"
    assert len(L.sslam_keypoint_depth.argtypes) == 10 and len(L.sslam_pose_depth_nn_pairs.argtypes) == 27
    assert len(L.sslam_match_score_known_pairs.argtypes) == 13
    for text in ("floor(u + 0.5)", "X = ((u - cx) * z) / fx", "u' = (fx * X') / Z' + cx", "HAS NO GROUND TRUTH", "-0.5 <= u' < view_w - 0.5",
                 "(dist[(v-1)>>1] + dist[v>>1]) / 2", "fp = count - tp - unknown", "no occlusion test"):
        assert text in hdr, text
    assert os.path.exists(os.path.join(lib.CSRC, "evaluate.hip"))
    assert lib.POSE_DEPTH_SCORE_KEYS == ("gt_matches", "gt_count", "gt_of_row", "valid_count", "dist_sum", "dist_median")
    assert lib.MATCH_KNOWN_SCORE_KEYS == ("tp", "fp", "fn", "unknown", "value_sum")
    import torch
    sh = lib.pose_depth_score_shapes(3, 7)
    assert sh["valid_count"] == ((3,), torch.int32) and sh["unknown"] == ((3,), torch.int32) and sh["gt_of_row"] == ((3, 7), torch.int32)
    assert {k: v for k, v in sh.items() if k not in ("valid_count", "unknown")} == lib.pose_score_shapes(3, 7)


def test_bindings_and_pipeline_refuse_malformed_arguments_before_any_device_work():
    import torch

    from sslam_amd import evaluation as ev
    from sslam_amd import lib
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    cam = ev.Camera()
    kp, kd = torch.zeros((3, 8, 2)), torch.zeros((3, 8), dtype=torch.int32)
    f, s = torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    T = torch.zeros((2, 12), dtype=torch.float64)
    depth = torch.zeros((3, 6, 8), dtype=torch.uint16)
    before = lib.launch_count()
    with pytest.raises(ValueError, match="depth must"):
        lib.keypoint_depth(depth.to(torch.int32), kp)
    with pytest.raises(ValueError, match="depth must"):
        lib.keypoint_depth(depth[0], kp)
    with pytest.raises(ValueError, match="kp_pixel"):
        lib.keypoint_depth(depth, kp[:2])
    with pytest.raises(ValueError, match="kp_pixel"):
        lib.keypoint_depth(depth, kp.double())
    with pytest.raises(ValueError, match="scale_x"):
        lib.keypoint_depth(depth, kp, 0.0)
    with pytest.raises(ValueError, match="scale_y"):
        lib.keypoint_depth(depth, kp, 1.0, float("nan"))
    with pytest.raises(ValueError, match="kp_depth"):
        lib.keypoint_depth(depth, kp, out=kd[:, :7])
    with pytest.raises(ValueError):                                 # well-formed host tensors: refused for where they live
        lib.keypoint_depth(depth, kp)
    with pytest.raises(ValueError, match="kp_bank"):
        lib.pose_depth_nn_pairs(kp.double(), kd, f, s, T, cam)
    with pytest.raises(ValueError, match="kp_depth_bank"):
        lib.pose_depth_nn_pairs(kp, kd.long(), f, s, T, cam)
    with pytest.raises(ValueError, match="kp_depth_bank"):
        lib.pose_depth_nn_pairs(kp, None, f, s, T, cam)
    with pytest.raises(ValueError, match="int32"):
        lib.pose_depth_nn_pairs(kp, kd, f.long(), s, T, cam)
    with pytest.raises(ValueError, match="threshold"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T, cam, threshold=-1.0)
    with pytest.raises(ValueError, match="T must"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T.float(), cam)
    with pytest.raises(ValueError, match="T must"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, None, cam)
    with pytest.raises(ValueError, match="T must"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, torch.zeros((3, 12), dtype=torch.float64), cam)
    with pytest.raises(ValueError, match="camera depth_scale"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T, ev.Camera(depth_scale=float("inf")))
    with pytest.raises(ValueError, match="camera cx"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T, ev.Camera(cx=float("nan")))
    with pytest.raises(ValueError, match="camera must have"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T, None)
    with pytest.raises(ValueError, match="scale_x"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T, cam, scale_x=-1.0)
    with pytest.raises(ValueError, match="n2"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T, cam, n2=9)
    with pytest.raises(lib.SslamHipError, match="4096"):
        lib.pose_depth_nn_pairs(torch.zeros((2, 4097, 2)), torch.zeros((2, 4097), dtype=torch.int32), f, s, T, cam)
    with pytest.raises(ValueError, match="out must hold 6"):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T, cam, out=(kd,))
    with pytest.raises(ValueError):
        lib.pose_depth_nn_pairs(kp, kd, f, s, T, cam)
    m, v, c = torch.zeros((2, 8, 2), dtype=torch.int64), torch.zeros((2, 8)), torch.zeros(2, dtype=torch.int32)
    row = torch.zeros((2, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match="gt_of_row"):
        lib.match_score_known_pairs(m, v, c, row[:, :7], c)
    with pytest.raises(ValueError, match="gt_count"):
        lib.match_score_known_pairs(m, v, c, row, None)
    with pytest.raises(ValueError, match="out `unknown`"):
        lib.match_score_known_pairs(m, v, c, row, c, out=(c, c, c, c.long(), torch.zeros(2, dtype=torch.float64)))
    with pytest.raises(ValueError):
        lib.match_score_known_pairs(m, v, c, row, c)
    pipe = SequencePipeline.__new__(SequencePipeline)               # no packing, no device: the checks come first
    pipe.cfg, pipe.device = ExtractorConfig(), torch.device("cpu")
    assert pipe.depth_scales(cam) == (640 / 448, 480 / 448)
    with pytest.raises(ValueError, match="depth_u16"):
        pipe.keypoint_depth(np.zeros((3, 6, 8), np.uint16), kp)
    with pytest.raises(ValueError, match="keypoints_pixel"):
        pipe.pose_depth_scores(kp[:, :, 0], kd, [0], [1], T[:1], cam)
    with pytest.raises(ValueError, match="kp_depth"):
        pipe.pose_depth_scores(kp, kd[:, :7], [0], [1], T[:1], cam)
    with pytest.raises(ValueError, match="both pair lists"):
        pipe.pose_depth_scores(kp, kd, [0], None, T[:1], cam)
    with pytest.raises(ValueError, match="threshold"):
        pipe.pose_depth_scores(kp, kd, [0], [1], T[:1], cam, threshold=float("nan"))
    with pytest.raises(ValueError, match="T must"):
        pipe.pose_depth_scores(kp, kd, [0, 1], [1, 2], np.zeros((2, 3, 3)), cam)
    with pytest.raises(ValueError, match="T .* is required"):
        pipe.pose_depth_scores(kp, kd, [0, 1], [1, 2], None, cam)
    with pytest.raises(ValueError, match="camera must have"):
        pipe.pose_depth_scores(kp, kd, [0, 1], [1, 2], np.zeros((2, 4, 4)), None)
    with pytest.raises(ValueError, match="matches"):
        pipe.pose_depth_scores(kp, kd, [0, 1], [1, 2], np.zeros((2, 4, 4)), cam, matches={"matches": m})
    bufs = pipe.alloc_pose_depth_scores(5, 8)
    assert set(bufs) == set(lib.POSE_DEPTH_SCORE_KEYS + lib.MATCH_KNOWN_SCORE_KEYS) and bufs["valid_count"].shape == (5,)
    assert set(pipe.alloc_pose_depth_scores(5, 8, with_matches=False)) == set(lib.POSE_DEPTH_SCORE_KEYS)
    assert lib.launch_count() == before


def test_run_directory_judges_the_depth_scoring_before_it_runs_the_sequence(tmp_path):
    """No pipeline, no weights, no device: each refusal below comes before anything is decoded, extracted or matched."""
    import synth
    from PIL import Image

    from sslam_amd import evaluation as ev
    from sslam_amd import harness, lib
    before = lib.launch_count()
    name = "rgbd_dataset_freiburg1_desk"
    synth.write_tum_sequence(str(tmp_path / name))                  # 32 x 24 frames: not what freiburg1's 640 x 480 camera describes
    with pytest.raises(ValueError, match="camera describes 640 x 480"):
        harness.run_directory(str(tmp_path), name, (1,), evaluate={"depth": True})
    with pytest.raises(ValueError, match="camera fx"):
        harness.run_directory(str(tmp_path), name, (1,), evaluate={"depth": True, "camera": ev.Camera(fx=-1.0, width=32, height=24)})
    os.makedirs(tmp_path / "bare" / "rgb")
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(tmp_path / "bare" / "rgb" / "1.0.png")
    with pytest.raises(ValueError, match="no depth images"):
        harness.run_directory(str(tmp_path / "bare"), evaluate={"depth": True})
    os.makedirs(tmp_path / "bare" / "depth")
    Image.fromarray(np.zeros((6, 8), np.uint16)).save(tmp_path / "bare" / "depth" / "1.0.png")
    with pytest.raises(ValueError, match="needs poses"):
        harness.run_directory(str(tmp_path / "bare"), evaluate={"depth": True, "camera": ev.Camera(width=8, height=6)})
    assert lib.launch_count() == before


def test_kp_depth_and_drop_in_arguments_are_judged_before_any_device_work():
    import torch

    import evaluation as dropin
    from sslam_amd import evaluation as ev
    from sslam_amd import lib
    before = lib.launch_count()
    poses = np.stack([np.eye(4)] * 3)
    kp = torch.zeros((3, 8, 2))
    mm = {key: torch.zeros(1) for key in ("matches", "value", "match_count")}
    result = {"frames": {"keypoints_pixel": kp}, 1: mm}
    kd = torch.zeros((3, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match="pass one"):
        ev.evaluate_result(None, result, poses, depth=np.zeros((3, 480, 640), np.uint16), kp_depth=kd)
    with pytest.raises(ValueError, match="kp_depth must be"):
        ev.evaluate_result(None, result, poses, kp_depth=kd[:, :7])
    with pytest.raises(ValueError, match="kp_depth must be"):
        ev.evaluate_result(None, result, poses, kp_depth=kd.long())
    with pytest.raises(ValueError, match="depth= needs poses"):
        ev.evaluate_result(None, result, None, kp_depth=kd, use_pose=False)
    with pytest.raises(ValueError, match="camera fy"):
        ev.evaluate_result(None, result, poses, kp_depth=kd, camera=ev.Camera(fy=0.0))
    ev.check_depth_size(640, 480, ev.Camera())
    with pytest.raises(ValueError, match="camera describes"):
        ev.check_depth_size(480, 640, ev.Camera())
    k = np.zeros((4, 2), np.float32)
    for fn in (dropin.compute_repeatability_depth, dropin.compute_ground_truth_matches_depth):
        with pytest.raises(ValueError, match="camera describes 640 x 480"):
            fn(k, k, np.zeros((24, 32), np.uint16), np.eye(4), ev.Camera())
        with pytest.raises(ValueError, match="uint16"):
            fn(k, k, np.zeros((480, 640), np.float32), np.eye(4), ev.Camera())
        with pytest.raises(ValueError, match="camera must have"):
            fn(k, k, np.zeros((480, 640), np.uint16), np.eye(4), None)
    assert lib.launch_count() == before
