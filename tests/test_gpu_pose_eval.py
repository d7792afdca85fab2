"""GPU tests of the pose-based scoring stage: sslam_pose_nn_pairs and sslam_match_score_pairs through sslam_amd.lib, the drop-in
functions of evaluation.py, SequencePipeline.pose_scores, sslam_amd.evaluation.evaluate / evaluate_result and
harness.run_directory(evaluate=).

References: what the reference's own methods returned (tests/golden/pose_eval.npz) and the float64 restatement of
tests/pose_eval_ref.py, itself held to those goldens in tests/test_pose_eval_cpu.py - whose docstring derives the tolerances used
here: integers equal; float64 distances with H given within 1e-10 px; H=None (float32 in the reference) and mean_match_distance
within 1e-6 relative; ratios of integers within 1e-12 relative.  Against the restatement, which is float64 like the device, the
distances are held to 1e-10 px with or without H."""
import numpy as np
import pytest

import guarded
import pose_eval_ref as pr
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev(T, a, name=None):
    """The device copy of an input; `name`, its argument in include/sslam_hip.h, places it under a guarded.Placement."""
    return guarded.device_input(T, a, name)


def _outputs(T, keys, n_pairs, n1):
    """Poisoned outputs between guard bands: {key: (whole, middle, tensor handed to the entry)}; float64 lies in an int64 layout."""
    from sslam_amd import lib
    shapes, out = lib.pose_score_shapes(n_pairs, n1), {}
    for key in keys:
        shape, dt = shapes[key]
        whole, mid = guarded.guarded(T, shape, T.int64 if dt == T.float64 else dt, name=key)
        out[key] = (whole, mid, mid.view(T.float64) if dt == T.float64 else mid)
    return out


def _collect(out, what):
    for key, (whole, mid, _) in out.items():
        guarded.assert_guards(whole, mid, f"{what} {key}")
        guarded.assert_written(mid, f"{what} {key}")
    return {key: t.cpu().numpy() for key, (_, _, t) in out.items()}


def pose_nn(T, bank, first, second, H, thr, n1=None, n2=None):
    """One launch into poisoned, guarded outputs; the inputs come back untouched.  -> dict of numpy arrays."""
    from sslam_amd import lib
    db, df, ds, dh = (_dev(T, bank, "kp_bank"), _dev(T, np.asarray(first, np.int32), "pair_first"),
                      _dev(T, np.asarray(second, np.int32), "pair_second"), _dev(T, H, "H"))
    out = _outputs(T, lib.POSE_SCORE_KEYS, len(first), bank.shape[1] if n1 is None else n1)
    n0 = lib.launch_count()
    lib.pose_nn_pairs(db, df, ds, dh, thr, n1=n1, n2=n2, out=tuple(out[key][2] for key in lib.POSE_SCORE_KEYS))
    assert lib.launch_count() - n0 == 1, "one launch"
    assert T.equal(db, _dev(T, bank)) and (dh is None or T.equal(dh, _dev(T, H)))
    return _collect(out, "pose_nn_pairs")


def match_score(T, pred, value, count, gt_of_row, gt_count):
    from sslam_amd import lib
    ins = [_dev(T, np.asarray(a, dt), name) for a, dt, name in ((pred, np.int64, "matches"), (value, np.float32, "value"),
                                                                  (count, np.int32, "count"), (gt_of_row, np.int32, "gt_of_row"),
                                                                  (gt_count, np.int32, "gt_count"))]
    out = _outputs(T, lib.MATCH_SCORE_KEYS, pred.shape[0], pred.shape[1])
    n0 = lib.launch_count()
    lib.match_score_pairs(*ins, out=tuple(out[key][2] for key in lib.MATCH_SCORE_KEYS))
    assert lib.launch_count() - n0 == 1, "one launch"
    return _collect(out, "match_score_pairs")


def check_against_restatement(got, want, k, where):
    """got: the device's arrays for P pairs; want: pose_eval_ref's list of dicts.  Integers equal, distances within 1e-10 px."""
    for p, w in enumerate(want):
        assert got["gt_count"][p] == w["gt_count"], (where, p, int(got["gt_count"][p]), w["gt_count"])
        assert np.array_equal(got["gt_matches"][p], w["gt_matches"]), (where, p)          # zero rows past the count included
        assert np.array_equal(got["gt_of_row"][p], w["gt_of_row"]), (where, p)
        for key in ("dist_sum", "dist_median"):
            scale = k if key == "dist_sum" else 1
            a, b = got[key][p] / scale, w[key] / scale
            print(f"{where} pair {p} {key} / {scale}: device {a!r} restatement {b!r}")
            assert a == b or abs(a - b) <= pr.ABS_POSED, (where, p, key, a, b)


# --------------------------------------------------------------------------------------------------- 1. both entries, per group
@pytest.mark.parametrize("name", pr.group_names())
def test_entries_equal_the_reference_and_the_restatement(T, name):
    g = pr.group(name)
    bank, posed = g["bank"], g["H"] is not None
    k, P = bank.shape[1], len(g["first"])
    got = pose_nn(T, bank, g["first"], g["second"], g["H"], g["threshold"])
    assert got["gt_matches"].dtype == np.int64 and got["gt_of_row"].dtype == np.int32 and got["dist_sum"].dtype == np.float64
    want = pr.pose_nn_pairs(bank, g["first"], g["second"], g["H"], g["threshold"])
    check_against_restatement(got, want, k, name)
    for p in range(P):                                               # the reference's own numbers
        assert got["gt_count"][p] == g["count"][p], (name, p)
        if g["first"][p] < 0 or g["second"][p] < 0:
            assert got["dist_sum"][p] == 0 and got["dist_median"][p] == 0 and (got["gt_of_row"][p] == -1).all()
            continue
        mean, med = got["dist_sum"][p] / k, got["dist_median"][p]
        print(f"{name} pair {p}: mean {mean!r} reference {g['mean'][p]!r}; median {med!r} reference {g['median'][p]!r}")
        assert pr.close(mean, g["mean"][p], "mean_nn_distance", posed), (name, p, mean, g["mean"][p])
        assert pr.close(med, g["median"][p], "median_nn_distance", posed), (name, p, med, g["median"][p])
        assert pr.close(np.int64(got["gt_count"][p]) / k, g["rep"][p], "repeatability", posed)
        if posed:
            assert np.array_equal(got["gt_matches"][p], g["gt"][p]), (name, p)
    again = pose_nn(T, bank, g["first"], g["second"], g["H"], g["threshold"])
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), f"{name} {key}: the same call gave other bytes"

    # the score entry: the reference's lists where the group has them, else each pair's own ground truth (tp = count)
    if "pred" in g:
        pred, pc, pv = g["pred"], g["pred_count"], g["pred_value"]
    else:
        pred, pc, pv = got["gt_matches"], got["gt_count"], np.zeros((P, k), np.float32)
    sc = match_score(T, pred, pv, pc, got["gt_of_row"], got["gt_count"])
    sc2 = match_score(T, pred, pv, pc, got["gt_of_row"], got["gt_count"])
    for key in sc:
        assert sc[key].tobytes() == sc2[key].tobytes(), f"{name} {key}: the same call gave other bytes"
    from sslam_amd import evaluation as ev
    for p in range(P):
        c = int(pc[p])
        tp, fp, fn, vs = pr.match_score(pred[p, :c], pv[p, :c], want[p]["gt_of_row"], want[p]["gt_count"])
        assert (sc["tp"][p], sc["fp"][p], sc["fn"][p]) == (tp, fp, fn), (name, p)
        assert abs(sc["value_sum"][p] - vs) <= 1e-12 * max(1.0, abs(vs)), (name, p, sc["value_sum"][p], vs)      # float64 sums of fp32 terms
        if "pred" in g and g["first"][p] >= 0 and g["second"][p] >= 0:
            m = ev.match_metrics(sc["tp"][p], sc["fp"][p], sc["fn"][p], c, got["gt_count"][p])
            for i, key in enumerate(pr.METRIC_KEYS):
                assert pr.close(m[key], g["metrics"][p, i], key, True), (name, p, key, m[key], g["metrics"][p, i])
        elif "pred" not in g:
            assert tp == c and fp == 0 and fn == 0


@pytest.mark.parametrize("k,n1,n2", [(1025, 1025, 1025), (4096, 4096, 4096), (300, 257, 131), (1500, 1024, 1500)])
def test_sizes_at_the_launch_shape_boundaries(T, k, n1, n2):
    """One row past the 256-thread shape (n1 = 1025), the shape's last size (1024) against more candidates, the LDS limit (4096),
    and unequal n1 / n2 below K: free float32 coordinates against the restatement (random points: no two roundings apart)."""
    rng = np.random.default_rng(k)
    bank = rng.uniform(0, 960, (2, k, 2)).astype(np.float32)
    bank[1, : k // 2] = bank[0, rng.permutation(k)[: k // 2]] + rng.normal(0, 1.5, (k // 2, 2)).astype(np.float32)
    bank[1, -3:] = bank[1, :3]                                       # duplicates: exact ties, the lowest index wins
    H = np.stack([np.array([[1.0, 0.002, -1.5], [-0.002, 1.0, 2.0], [1e-6, -2e-6, 1.0]]).reshape(9)] * 2)
    first, second = [0, 1], [1, 0]
    for a, b, h in ((0, 1, H[0]), (1, 0, H[1])):
        edge, gap = pr.margins(bank[a, :n1], bank[b, :n2], h, 3.0)
        assert edge >= 1e-6 and gap >= 1e-6, "a seed on the margin: choose another"
    got = pose_nn(T, bank, first, second, H, 3.0, n1=n1, n2=n2)
    want = [pr.pose_nn(bank[a, :n1], bank[b, :n2], H[p], 3.0) for p, (a, b) in enumerate(zip(first, second))]
    assert 0 < want[0]["gt_count"] < n1
    check_against_restatement(got, want, n1, f"K {k} n1 {n1} n2 {n2}")


def test_refusals_on_the_device_launch_nothing(T):
    from sslam_amd import lib
    bank = T.zeros((2, 4097, 2), device="cuda")
    f = T.zeros(1, dtype=T.int32, device="cuda")
    n0 = lib.launch_count()
    with pytest.raises(lib.SslamHipError, match="4096"):
        lib.pose_nn_pairs(bank, f, f + 1)
    with pytest.raises(ValueError, match="threshold"):
        lib.pose_nn_pairs(bank[:, :8].contiguous(), f, f + 1, None, float("inf"))
    assert lib.launch_count() == n0


# ------------------------------------------------------------------------------------------------------------ 2. capture
def test_a_captured_replay_equals_the_direct_launches(T):
    from sslam_amd import lib
    g = pr.group("g28_rot")
    bank, f, s, H = _dev(T, g["bank"]), _dev(T, g["first"]), _dev(T, g["second"]), _dev(T, g["H"])
    pred, pv, pc = _dev(T, g["pred"]), _dev(T, g["pred_value"]), _dev(T, g["pred_count"])
    direct = lib.pose_nn_pairs(bank, f, s, H, 3.0)
    direct += lib.match_score_pairs(pred, pv, pc, direct[2], direct[1])
    P, k = len(g["first"]), g["bank"].shape[1]
    shapes = lib.pose_score_shapes(P, k)
    keys = lib.POSE_SCORE_KEYS + lib.MATCH_SCORE_KEYS
    out = [T.full(shapes[key][0], -5, dtype=shapes[key][1], device="cuda") for key in keys]
    T.cuda.synchronize()
    graph = T.cuda.CUDAGraph()
    with T.cuda.graph(graph):
        lib.pose_nn_pairs(bank, f, s, H, 3.0, out=tuple(out[:5]))
        lib.match_score_pairs(pred, pv, pc, out[2], out[1], out=tuple(out[5:]))
    for t in out:
        t.fill_(-5)                                                  # what the capture may have written is gone
    graph.replay()
    T.cuda.synchronize()
    for key, a, b in zip(keys, direct, out):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{key}: the replayed capture gave other bytes"


# ------------------------------------------------------------------------------------------------------------ 3. drop-ins
@pytest.mark.parametrize("name", pr.dropin_names())
@pytest.mark.parametrize("on_device", [False, True])
def test_drop_in_functions(T, name, on_device):
    import evaluation as dropin
    d = pr.dropin(name)
    conv = (lambda a: None if a is None else T.from_numpy(a).cuda()) if on_device else (lambda a: a)
    k1, k2, H = conv(d["kpts1"]), conv(d["kpts2"]), conv(d["H"])
    posed = d["H"] is not None
    r = dropin.compute_repeatability(k1, k2, H, threshold=d["threshold"])
    assert list(r) == list(pr.REP_RESULT_KEYS)
    for i, key in enumerate(pr.REP_RESULT_KEYS):
        print(f"{name} {key}: {r[key]!r} reference {d['rep'][i]!r}")
        assert pr.close(r[key], d["rep"][i], key, posed), (name, key, r[key], d["rep"][i])
    if not posed:
        with pytest.raises(ValueError):
            dropin.compute_ground_truth_matches(k1, k2, None)
        return
    gt = dropin.compute_ground_truth_matches(k1, k2, H, d["threshold"])
    assert isinstance(gt, T.Tensor if on_device else np.ndarray)
    gt_h = gt.cpu().numpy() if on_device else gt
    assert gt_h.dtype == np.int64 and np.array_equal(gt_h, d["gt"]), name
    n, m = len(d["kpts1"]), len(d["kpts2"])
    want = pr.pose_nn(d["kpts1"], d["kpts2"], d["H"].reshape(9), d["threshold"])
    half = gt_h[::2].copy()
    half[::3, 1] = (half[::3, 1] + 1) % m                            # a third of the kept half points at the wrong partner
    for pred in (gt_h, gt_h[:0], half):
        got = dropin.evaluate_matches(conv(pred), gt, n, m)
        tp, fp, fn, _ = pr.match_score(pred, np.zeros(len(pred)), want["gt_of_row"], want["gt_count"])
        assert list(got) == list(pr.METRIC_KEYS)
        assert (got["tp"], got["fp"], got["fn"], got["num_pred_matches"], got["num_gt_matches"]) == (tp, fp, fn, len(pred), len(gt_h))
        assert got["precision"] == (tp / (tp + fp) if tp + fp else 0.0) and got["recall"] == (tp / (tp + fn) if tp + fn else 0.0)
        assert got["inlier_ratio"] == (tp / len(pred) if len(pred) else 0.0)


# ------------------------------------------------------------------------------------------------- 4. the whole evaluation
@pytest.fixture(scope="module")
def seq(T):
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K), inp["selector"], inp["refiner"], device="cuda")
    return pipe, T.from_numpy(inp["tokens"]).cuda(), inp["poses"]


def check_summaries(got, s, what):
    pr.check_summary(got["repeatability"], s["rep_summary"], s["rep_results"], pr.REP_SUMMARY_KEYS, pr.REP_RESULT_KEYS, s["use_pose"],
                  what + " repeatability")
    pr.check_summary(got["descriptor_quality"], s["dq_summary"], s["dq_results"], pr.DQ_SUMMARY_KEYS, pr.DQ_RESULT_KEYS, True,
                  what + " descriptor quality")


@pytest.mark.parametrize("name", ["seq_s1", "seq_s5", "seq_s5_n4"])
def test_evaluate_and_evaluate_result_equal_the_reference_summaries(T, seq, name):
    from sslam_amd import evaluation as ev
    from sslam_amd.harness import StreamingSequence
    from sslam_amd.pipeline import MatchRule
    pipe, toks, poses = seq
    s = pr.sequence(name)
    got = ev.evaluate(pipe, None, poses, spacing=s["spacing"], num_pairs=s["num_pairs"], tokens=toks, sequence="synthetic")
    check_summaries(got, s, name + " evaluate")
    result = StreamingSequence(pipe, (1, 5), rule=MatchRule.mnn_ratio(0.9)).run(toks)
    again = ev.evaluate_result(pipe, result, poses, spacing=s["spacing"], num_pairs=s["num_pairs"], sequence="synthetic")
    check_summaries(again, s, name + " evaluate_result")
    for part in ("repeatability", "descriptor_quality"):
        assert repr(got[part]) == repr(again[part]), f"{name} {part}: evaluate and evaluate_result disagree"


def test_evaluate_without_pose_correction_and_without_poses(T, seq):
    from sslam_amd import evaluation as ev
    pipe, toks, poses = seq
    s = pr.sequence("seq_s1_raw")
    got = ev.evaluate(pipe, None, None, spacing=1, use_pose=False, tokens=toks, sequence="synthetic")
    assert got["descriptor_quality"] is None, "descriptor quality needs poses, as in the reference"
    pr.check_summary(got["repeatability"], s["rep_summary"], s["rep_results"], pr.REP_SUMMARY_KEYS, pr.REP_RESULT_KEYS, False, "raw")
    both = ev.evaluate(pipe, None, poses, spacing=1, use_pose=False, tokens=toks, sequence="synthetic")
    assert repr(both["repeatability"]) == repr(got["repeatability"])
    posed = pr.sequence("seq_s1")
    pr.check_summary(both["descriptor_quality"], posed["dq_summary"], posed["dq_results"], pr.DQ_SUMMARY_KEYS, pr.DQ_RESULT_KEYS, True, "raw + dq")
    with pytest.raises(ValueError, match="poses"):
        ev.evaluate(pipe, None, None, tokens=toks)
    with pytest.raises(ValueError, match="not matched under a rule"):
        from sslam_amd.harness import StreamingSequence
        ev.evaluate_result(pipe, StreamingSequence(pipe, (1,)).run(toks[:3]), poses[:3])


def test_pose_scores_cuts_more_than_65535_pairs(T):
    """65 537 pairs of a 3-frame bank of 2 keypoints: the second launch scores the last two pairs like the first ones."""
    from sslam_amd.pipeline import MAX_PAIRS_PER_LAUNCH, ExtractorConfig, SequencePipeline
    pipe = SequencePipeline.__new__(SequencePipeline)                 # the stage needs no weights
    pipe.cfg, pipe.device = ExtractorConfig(num_keypoints=2), T.device("cuda")
    bank = np.array([[[8, 8], [24, 8]], [[9, 8], [200, 8]], [[24, 10], [8, 9]]], np.float32)
    n = MAX_PAIRS_PER_LAUNCH + 2
    first, second = np.arange(n) % 3, (np.arange(n) // 3) % 3
    first[5] = -1
    matches = {"matches": T.tensor([[0, 0], [1, 1]], device="cuda").repeat(n, 1, 1), "value": T.full((n, 2), 0.25, device="cuda"),
               "match_count": (T.arange(n, device="cuda") % 3).int()}
    got = {key: v.cpu().numpy() for key, v in pipe.pose_scores(T.from_numpy(bank).cuda(), first.astype(np.int32), second.astype(np.int32), None,
                                                              matches=matches).items()}
    for p in list(range(12)) + list(range(n - 6, n)):
        w = pr.pose_nn_pairs(bank, [first[p]], [second[p]], None, 3.0)[0]
        c = p % 3
        tp, fp, fn, vs = pr.match_score([[0, 0], [1, 1]][:c], [0.25] * c, w["gt_of_row"], w["gt_count"])
        assert (got["gt_count"][p], got["tp"][p], got["fp"][p], got["fn"][p], got["value_sum"][p]) == (w["gt_count"], tp, fp, fn, vs), p
        assert np.array_equal(got["gt_matches"][p], w["gt_matches"]) and got["dist_sum"][p] == w["dist_sum"]


def test_run_directory_with_evaluate(T, tmp_path):
    """run_directory(evaluate=...) on the TUM fixture tree of tests/test_tum_reader.py: the 'evaluation' entry per spacing equals
    evaluate_result on the returned result and the restatement on the result's own keypoints and M4 lists, with the poses of
    groundtruth.txt; without evaluate= the result has no such entry."""
    from sslam_amd import evaluation as ev
    from sslam_amd.harness import run_directory
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    from sslam_amd.tum import TUMSequence
    name, g, k = "rgbd_dataset_freiburg1_desk", 5, 12
    synth.write_tum_sequence(str(tmp_path / name))
    tum = TUMSequence(str(tmp_path), name)
    n = len(tum)
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    toks = T.from_numpy(synth.token_sequence(n, g)).cuda()
    kw = dict(pipe=pipe, tokens_fn=lambda a, b: toks[a:b], chunk=4, decode_workers=2)
    plain = run_directory(str(tmp_path), name, (1, 3), rule=MatchRule.mnn_ratio(0.9), **kw)
    assert "evaluation" not in plain
    got = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(num_pairs=4, threshold=20.0), **kw)
    assert set(got["evaluation"]) == {1, 3}
    for key in ("matches", "value", "match_count"):
        assert T.equal(got[1][key], plain[1][key]), key
    kp = got["frames"]["keypoints_pixel"].cpu().numpy()
    for sp in (1, 3):
        e = got["evaluation"][sp]
        direct = ev.evaluate_result(pipe, got, tum.poses, spacing=sp, num_pairs=4, threshold=20.0, sequence=name)
        assert repr(e) == repr(direct)
        pairs = ev.pair_list(n, sp, 4)
        assert e["repeatability"]["num_pairs"] == len(pairs) == min(4, n - sp) and e["repeatability"]["sequence"] == name
        H = ev.pair_homographies(tum.poses, pairs)
        mt, val, cnt = (got[sp][key].cpu().numpy() for key in ("matches", "value", "match_count"))
        for p, (a, b) in enumerate(pairs):
            w = pr.pose_nn(kp[a], kp[b], H[p].reshape(9), 20.0)
            r, q = e["repeatability"]["all_results"][p], e["descriptor_quality"]["all_results"][p]
            assert r["repeatable_count"] == w["gt_count"] and r["total_keypoints"] == k
            assert abs(r["mean_nn_distance"] - w["dist_sum"] / k) <= pr.ABS_POSED and abs(r["median_nn_distance"] - w["dist_median"]) <= pr.ABS_POSED
            tp, fp, fn, vs = pr.match_score(mt[p, :cnt[p]], val[p, :cnt[p]], w["gt_of_row"], w["gt_count"])
            assert (q["tp"], q["fp"], q["fn"], q["num_pred_matches"], q["num_gt_matches"]) == (tp, fp, fn, cnt[p], w["gt_count"])
