"""The pose-based scoring stage (sslam_pose_nn_pairs / sslam_match_score_pairs, sslam_amd.evaluation) as far as a machine without
a GPU can see it: the float64 restatement of tests/pose_eval_ref.py against what the reference's own methods returned
(tests/golden/pose_eval.npz), the host composition against the reference's two test_sequence summaries, relative_pose's float32
rounding, pair_list, the refusals of the two C entries (which come before any launch), and the entries against the header, the
built library and sslam_amd.lib.

Tolerances (none comes from what the code under test gives):
  integers         equal: repeatable counts, ground-truth matches, tp / fp / fn, list lengths.  The fixture generator keeps
                   every distance >= 1e-6 px away from its threshold and every runner-up location >= 1e-6 px behind the winner,
                   a million times the rounding below, so no integer can turn on a rounding.
  floats, H given  |d| <= 1e-10 px.  Coordinates are at most 960; a warped coordinate carries at most four roundings of 2^-53
                   relative (two products, two sums; the division adds one more to the quotient), 4e-13 px; a distance or a mean
                   of distances at most twice that.  1e-10 is a 100-fold margin and covers a BLAS that fuses the 3 x 3 product.
  floats, H None   1e-6 relative: the reference stays in float32 there (float32 keypoints, float32 norm, float32 pairwise mean
                   of n <= 4096 terms: (log2 n + 1) 2^-24 ~ 7.8e-7); the same for mean_match_distance, a float32 mean of 1 - sim.
  ratios           1e-12 relative: float64 quotients of exact integers in the reference's order of operations.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pose_eval_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
# never dereferenced: every call below is refused by the entry's own checks, which come before the launch
P = [0x10000 * (i + 1) for i in range(12)]


def _present(g):
    return [p for p, (a, b) in enumerate(zip(g["first"], g["second"])) if a >= 0 and b >= 0]


@pytest.mark.parametrize("name", pr.group_names())
def test_restatement_equals_the_reference_per_pair(name):
    g = pr.group(name)
    posed = g["H"] is not None
    ours = pr.pose_nn_pairs(g["bank"], g["first"], g["second"], g["H"], g["threshold"])
    k = g["bank"].shape[1]
    for p, o in enumerate(ours):
        assert o["gt_count"] == g["count"][p], (name, p)
        if p not in _present(g):
            assert o["gt_count"] == 0 and not o["gt_matches"].any() and (o["gt_of_row"] == -1).all()
            continue
        assert pr.close(o["dist_sum"] / k, g["mean"][p], "mean_nn_distance", posed), (name, p, o["dist_sum"] / k, g["mean"][p])
        assert pr.close(o["dist_median"], g["median"][p], "median_nn_distance", posed), (name, p, o["dist_median"], g["median"][p])
        assert pr.close(np.int64(o["gt_count"]) / k, g["rep"][p], "repeatability", posed)
        if posed:
            assert np.array_equal(o["gt_matches"], g["gt"][p]), (name, p)
        # the two forms of the ground truth say the same
        c = o["gt_count"]
        assert np.array_equal(o["gt_of_row"][o["gt_matches"][:c, 0]], o["gt_matches"][:c, 1]) and (o["gt_of_row"] >= 0).sum() == c


@pytest.mark.parametrize("name", [n for n in pr.group_names() if "pred" in pr.group(n)])
def test_restated_scores_and_host_metrics_equal_the_reference(name):
    from sslam_amd import evaluation as ev
    g = pr.group(name)
    ours = pr.pose_nn_pairs(g["bank"], g["first"], g["second"], g["H"], g["threshold"])
    seen = 0
    for p in _present(g):
        c = int(g["pred_count"][p])
        tp, fp, fn, vs = pr.match_score(g["pred"][p, :c], g["pred_value"][p, :c], ours[p]["gt_of_row"], ours[p]["gt_count"])
        m = ev.match_metrics(tp, fp, fn, c, ours[p]["gt_count"])
        assert list(m) == list(pr.METRIC_KEYS), "evaluate_matches' keys, in its order"
        for i, key in enumerate(pr.METRIC_KEYS):
            assert pr.close(m[key], g["metrics"][p, i], key, True), (name, p, key, m[key], g["metrics"][p, i])
        seen += c
    assert seen > 0 or "far" in name or "w0" in name or "thr0" in name


def test_the_goldens_cover_what_they_must():
    names = pr.group_names()
    banks = {n.split("_")[0] for n in names}
    assert {"g28", "g40", "g60"} <= banks and {f"lat{k}" for k in (1, 2, 3, 63, 64, 65, 127, 129)} <= banks
    assert {pr.group(n)["threshold"] for n in names} == {3.0, 0.0, 1e9}
    g = pr.group("g28_rot")
    assert -1 in g["first"] and any(a == b and a >= 0 for a, b in zip(g["first"], g["second"])) and list(g["second"]).count(1) > 1
    for b in ("g28", "g40", "g60"):                                 # selector output holds duplicate keypoints
        bank = pr.golden()["bank_" + b]
        assert any(len(np.unique(f, axis=0)) < len(f) for f in bank), b
    assert not pr.group("g28_far")["count"].any() and pr.group("g28_thrbig")["count"][0] == 500
    w0 = pr.group("lat65_w0")
    assert np.isinf(w0["mean"]).all() and np.isfinite(w0["median"]).all()
    lists = pr.group("g28_rot")
    assert lists["pred_count"][3] == 0 and np.array_equal(lists["pred"][4], lists["gt"][4]) and lists["pred_count"][0] > 0
    # the generator's margin condition holds for every kept case (it replaces a seed that fails; nothing is filtered here)
    for n in names:
        g = pr.group(n)
        for p in _present(g):
            edge, gap = pr.margins(g["bank"][g["first"][p]], g["bank"][g["second"][p]], None if g["H"] is None else g["H"][p], g["threshold"])
            assert edge >= 1e-6 and gap >= 1e-6, (n, p, edge, gap)
    assert os.path.getsize(pr.GOLDEN) < 1 << 20


# ------------------------------------------------------------------------------------------------------- host composition
@pytest.fixture(scope="module")
def oracle_sequence():
    """Keypoints, descriptors and canonical-order M4 lists of the 12-frame synthetic sequence from the CPU oracle (the device
    pipeline gives the same bits), and the restated per-pair statistics evaluation's summaries are composed from."""
    from oracle import ora
    from sslam_amd import evaluation as ev
    inp = pr.sequence_inputs()
    n, g = pr.SEQ_FRAMES, pr.SEQ_GRID
    feat = ora.bn_tokens(inp["tokens"])[0].reshape(n, g, g, 384)
    kp, _, _, _ = ora.select_keypoints(ora.selector_saliency(feat, inp["selector"]), pr.SEQ_K)
    desc = ora.refine(ora.gather(feat, kp), inp["refiner"])
    kp = ora.patch_to_pixel(kp)

    def stats(spacing, num_pairs, use_pose):
        pairs = ev.pair_list(n, spacing, num_pairs)
        H = ev.pair_homographies(inp["poses"], pairs)
        rep = [pr.pose_nn(kp[a], kp[b], H[p] if use_pose else None, 3.0) for p, (a, b) in enumerate(pairs)]
        st = dict(num_keypoints=pr.SEQ_K, gt_count=[r["gt_count"] for r in rep], dist_sum=[r["dist_sum"] for r in rep],
                  dist_median=[r["dist_median"] for r in rep])
        dq = None
        if use_pose:
            rows = []
            for p, (a, b) in enumerate(pairs):
                pm, dist = ora.find_mnn_m4(desc[a], desc[b])
                rows.append(pr.match_score(pm, dist, rep[p]["gt_of_row"], rep[p]["gt_count"]) + (len(pm),))
            dq = dict(num_keypoints=pr.SEQ_K, gt_count=st["gt_count"], tp=[r[0] for r in rows], fp=[r[1] for r in rows],
                      fn=[r[2] for r in rows], value_sum=[r[3] for r in rows], match_count=[r[4] for r in rows])
        return st, dq
    return stats


@pytest.mark.parametrize("name", pr.sequence_names())
def test_host_composition_equals_the_reference_summaries(name, oracle_sequence):
    from sslam_amd import evaluation as ev
    s = pr.sequence(name)
    st, dq = oracle_sequence(s["spacing"], s["num_pairs"], s["use_pose"])
    pr.check_summary(ev.repeatability_summary(st, "synthetic"), s["rep_summary"], s["rep_results"], pr.REP_SUMMARY_KEYS, pr.REP_RESULT_KEYS,
                  s["use_pose"], name + " repeatability")
    if s["use_pose"]:
        pr.check_summary(ev.descriptor_quality_summary(dq, "synthetic"), s["dq_summary"], s["dq_results"], pr.DQ_SUMMARY_KEYS,
                      pr.DQ_RESULT_KEYS, True, name + " descriptor quality")
    else:
        assert s["dq_summary"] is None


def test_summaries_follow_the_zero_denominator_rules():
    from sslam_amd import evaluation as ev
    m = ev.match_metrics(0, 0, 0, 0, 0)
    assert (m["precision"], m["recall"], m["f1"], m["inlier_ratio"]) == (0.0, 0.0, 0.0, 0.0)
    m = ev.match_metrics(0, 3, 2, 3, 2)
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["f1"] == 0.0 and m["inlier_ratio"] == 0.0
    s = ev.descriptor_quality_summary(dict(num_keypoints=8, gt_count=[2, 0], tp=[1, 0], fp=[1, 0], fn=[1, 0], value_sum=[0.5, 0.0],
                                           match_count=[2, 0]))
    assert s["all_results"][1]["mean_match_distance"] == 0.0 and s["all_results"][0]["mean_match_distance"] == 0.25
    assert s["mean_num_matches"] == 1.0 and s["num_pairs"] == 2
    with pytest.raises(ValueError):
        ev.repeatability_summary(dict(num_keypoints=8, gt_count=[], dist_sum=[], dist_median=[]))
    with pytest.raises(ValueError):
        ev.repeatability_summary(dict(gt_count=[1], dist_sum=[1.0], dist_median=[1.0]))


def test_relative_pose_is_rounded_to_float32_and_the_homography_is_float64():
    from sslam_amd import evaluation as ev
    poses = pr.golden()["seq_poses"]
    T = ev.relative_pose(poses[2], poses[7])
    full = poses[7] @ np.linalg.inv(poses[2])
    assert T.dtype == np.float32 and np.array_equal(T, full.astype(np.float32)) and not np.array_equal(T.astype(np.float64), full)
    H = ev.homography(T)
    assert H.dtype == np.float64 and np.array_equal(H, ev.TUM_K @ T[:3, :3] @ np.linalg.inv(ev.TUM_K))
    assert not np.array_equal(H, ev.TUM_K @ full[:3, :3] @ np.linalg.inv(ev.TUM_K)), "the float32 rounding must reach H"
    assert np.array_equal(ev.TUM_K, [[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])
    assert np.array_equal(ev.pair_homographies(poses, [(2, 7), (0, 0)])[0], H)
    with pytest.raises(ValueError):
        ev.relative_pose(poses[0][:3], poses[1])
    with pytest.raises(ValueError):
        ev.pair_homographies(poses, [(0, 12)])


def test_pair_list_is_the_testers_walk_not_process_spacing():
    from sslam_amd import evaluation as ev
    assert ev.pair_list(12, 1, 50) == [(i, i + 1) for i in range(11)]
    assert ev.pair_list(12, 5, 50) == [(i, i + 5) for i in range(7)]          # every i, not i = 0, 5, 10
    assert ev.pair_list(12, 5, 4) == [(i, i + 5) for i in range(4)]
    assert ev.pair_list(100, 3, 10) == [(i, i + 3) for i in range(10)]
    assert ev.pair_list(5, 5, 50) == [] and ev.pair_list(0, 1, 50) == [] and ev.pair_list(12, 1, 0) == []
    for bad in (dict(spacing=0), dict(spacing=1.0), dict(num_pairs=-1), dict(n_frames=True)):
        with pytest.raises(ValueError):
            ev.pair_list(**{**dict(n_frames=12, spacing=1, num_pairs=5), **bad})


def test_evaluate_refuses_before_any_device_work():
    from sslam_amd import evaluation as ev
    from sslam_amd import lib
    before = lib.launch_count()
    with pytest.raises(ValueError, match="poses"):
        ev.evaluate(None, np.zeros((3, 8, 8, 3), np.uint8), None)
    with pytest.raises(ValueError, match="poses"):
        ev.evaluate_result(None, {}, None)
    with pytest.raises(ValueError, match="result"):
        ev.evaluate_result(None, {}, np.zeros((3, 4, 4)))
    with pytest.raises(ValueError, match="images_u8 or tokens"):
        ev.evaluate(None, None, np.zeros((3, 4, 4)))
    for bad in (-1.0, float("nan"), float("inf"), "3", True):
        with pytest.raises(ValueError, match="threshold"):
            lib.check_threshold(bad)
    assert lib.check_threshold(0) == 0.0 and lib.check_threshold(1e9) == 1e9
    assert lib.launch_count() == before


# ----------------------------------------------------------------------------------------------------------- the C entries
def _nn(L, kp=P[0], n_bank=3, K=8, n1=8, n2=8, first=P[1], second=P[2], n_pairs=2, H=P[3], thr=3.0, gt=P[4], cnt=P[5], row=P[6],
        dsum=P[7], dmed=P[8]):
    return L.sslam_pose_nn_pairs(kp, n_bank, K, n1, n2, first, second, n_pairs, H, ctypes.c_double(thr), gt, cnt, row, dsum, dmed, None)


def _score(L, m=P[0], v=P[1], c=P[2], row=P[3], gtc=P[4], n1=8, n_pairs=2, tp=P[5], fp=P[6], fn=P[7], vs=P[8]):
    return L.sslam_match_score_pairs(m, v, c, row, gtc, n1, n_pairs, tp, fp, fn, vs, None)


def test_c_entries_refuse_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    before = lib.launch_count()
    bad = [dict(kp=None), dict(first=None), dict(second=None), dict(gt=None), dict(cnt=None), dict(row=None), dict(dsum=None),
           dict(dmed=None), dict(n_bank=0), dict(K=0), dict(K=-1), dict(n1=0), dict(n2=0), dict(n1=9), dict(n2=9), dict(n_pairs=0),
           dict(n_pairs=-2), dict(thr=-1e-300), dict(thr=-3.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(kp=P[0] + 4),
           dict(H=P[3] + 4), dict(first=P[1] + 2)]
    for kw in bad:
        assert _nn(L, **kw) == E_INVALID, kw
    for kw in (dict(K=4097, n1=4097, n2=4097), dict(K=4097), dict(K=1 << 20, n1=500, n2=500)):
        assert _nn(L, **kw) == E_UNSUPPORTED, kw
    assert _nn(L, K=5000, n1=5001) == E_INVALID, "n1 > K is an invalid argument at any K"
    for kw in [dict(m=None), dict(v=None), dict(c=None), dict(row=None), dict(gtc=None), dict(tp=None), dict(fp=None), dict(fn=None),
               dict(vs=None), dict(n1=0), dict(n1=-1), dict(n_pairs=0)]:
        assert _score(L, **kw) == E_INVALID, kw
    assert _score(L, n1=4097) == E_UNSUPPORTED
    assert lib.launch_count() == before, "a refused call launches nothing"


def test_entries_are_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sslam_hip.h")).read()
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    for entry in ("sslam_pose_nn_pairs", "sslam_match_score_pairs"):
        assert re.search(r"^int\s+" + entry + r"\s*\(", hdr, flags=re.M), entry
        assert entry in lib.EXPORTS and re.search(r"\bT\s+" + entry + r"$", dyn, flags=re.M), entry
    L = lib.lib()
    assert L.sslam_version() > 610, "new entries raise the version"
    assert len(L.sslam_pose_nn_pairs.argtypes) == 16 and len(L.sslam_match_score_pairs.argtypes) == 12
    m = re.search(r"#define\s+SSLAM_EVAL_MAX_K\s+(\d+)", hdr)
    assert m and int(m.group(1)) == lib.EVAL_MAX_K == 4096
    for text in ("test/test_repeatability.py:79-128", "test/test_descriptor_quality.py:144-185", "test/test_descriptor_quality.py:187-231",
                 "LOWEST index", "idx1 is unique", "outside the contract", "W is exactly 0"):
        assert text in hdr, text
    assert os.path.exists(os.path.join(lib.CSRC, "evaluate.hip"))


def test_binding_and_pipeline_refuse_malformed_arguments_before_any_device_work():
    import torch

    from sslam_amd import lib
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    kp = torch.zeros((3, 8, 2))
    f, s = torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    before = lib.launch_count()
    with pytest.raises(ValueError, match="kp_bank"):
        lib.pose_nn_pairs(kp[:, :, :1], f, s)
    with pytest.raises(ValueError, match="kp_bank"):
        lib.pose_nn_pairs(kp.double(), f, s)
    with pytest.raises(ValueError, match="int32"):
        lib.pose_nn_pairs(kp, f.long(), s)
    with pytest.raises(ValueError, match="threshold"):
        lib.pose_nn_pairs(kp, f, s, None, -1.0)
    with pytest.raises(ValueError, match="H must"):
        lib.pose_nn_pairs(kp, f, s, torch.zeros((2, 9)))
    with pytest.raises(ValueError, match="H must"):
        lib.pose_nn_pairs(kp, f, s, torch.zeros((3, 9), dtype=torch.float64))
    with pytest.raises(ValueError, match="n1"):
        lib.pose_nn_pairs(kp, f, s, n1=9)
    with pytest.raises(lib.SslamHipError, match="4096"):
        lib.pose_nn_pairs(torch.zeros((2, 4097, 2)), f, s)
    with pytest.raises(ValueError):                                 # well-formed host tensors: refused for where they live
        lib.pose_nn_pairs(kp, f, s)
    m, v, c = torch.zeros((2, 8, 2), dtype=torch.int64), torch.zeros((2, 8)), torch.zeros(2, dtype=torch.int32)
    row = torch.zeros((2, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match="gt_of_row"):
        lib.match_score_pairs(m, v, c, row[:, :7], c)
    with pytest.raises(ValueError, match="value"):
        lib.match_score_pairs(m, v.double(), c, row, c)
    with pytest.raises(ValueError, match="gt_count"):
        lib.match_score_pairs(m, v, c, row, None)
    with pytest.raises(ValueError, match="out `tp`"):
        lib.match_score_pairs(m, v, c, row, c, out=(c.long(), c, c, torch.zeros(2, dtype=torch.float64)))
    with pytest.raises(ValueError):
        lib.match_score_pairs(m, v, c, row, c)
    pipe = SequencePipeline.__new__(SequencePipeline)               # no packing, no device: the checks come first
    pipe.cfg, pipe.device = ExtractorConfig(), torch.device("cpu")
    with pytest.raises(ValueError, match="keypoints_pixel"):
        pipe.pose_scores(kp[:, :, 0], [0], [1], None)
    with pytest.raises(ValueError, match="both pair lists"):
        pipe.pose_scores(kp, [0], None, None)
    with pytest.raises(ValueError, match="threshold"):
        pipe.pose_scores(kp, [0], [1], None, threshold=float("nan"))
    with pytest.raises(ValueError, match="H must"):
        pipe.pose_scores(kp, [0, 1], [1, 2], np.zeros((3, 3, 3)))
    with pytest.raises(ValueError, match="matches"):
        pipe.pose_scores(kp, [0, 1], [1, 2], None, matches={"matches": m})
    bufs = pipe.alloc_pose_scores(5, 8)
    assert set(bufs) == set(lib.POSE_SCORE_KEYS + lib.MATCH_SCORE_KEYS) and bufs["gt_matches"].shape == (5, 8, 2)
    assert bufs["dist_sum"].dtype == torch.float64 and set(pipe.alloc_pose_scores(5, 8, with_matches=False)) == set(lib.POSE_SCORE_KEYS)
    assert lib.launch_count() == before


def test_run_directory_refuses_a_rule_that_is_not_m4_beside_evaluate(tmp_path):
    from sslam_amd import harness
    from sslam_amd.pipeline import MatchRule
    with pytest.raises(ValueError, match="M4"):
        harness.run_directory(str(tmp_path), rule=MatchRule.ratio(), evaluate={})
    with pytest.raises(ValueError, match="spacing"):
        harness.run_directory(str(tmp_path), evaluate={"spacing": 1})


@pytest.mark.skipif(not os.path.isdir("/root/reference/semantic-slam"), reason="the reference lives in the build container only")
def test_the_generator_reproduces_the_committed_fixture(tmp_path):
    out = tmp_path / "pose_eval.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_pose_eval.py"), str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    new, old = np.load(out), pr.golden()
    assert set(new.files) == set(old)
    for key in new.files:
        a, b = new[key], old[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        if a.dtype.kind == "f":
            # the reference's matrix products go through BLAS, whose summation order may depend on the host: its float32
            # similarities (128 terms, |sum| <= 1) move by up to 128 * 2^-24 ~ 8e-6, its float64 3 x 3 warps by ~1e-13 px
            from_sims = a.dtype == np.float32 or "_dq_" in key
            assert np.allclose(a, b, rtol=0, atol=2e-5 if from_sims else 1e-9, equal_nan=True), key
        else:
            assert np.array_equal(a, b), key
