"""A float64 numpy restatement of the pose-based scoring stage (csrc/evaluate.hip; include/sslam_hip.h states the contract), and
the loaders of tests/golden/pose_eval.npz - what the reference's own RepeatabilityTester / DescriptorQualityTester methods
returned on the same inputs (tests/golden/make_golden_pose_eval.py).

The restatement works in float64 whatever H is (the reference stays in float32 with H=None) and spells the warp out as the
header does - X = (h00 x + h01 y) + h02 - where the reference leaves the order to the 3 x 3 matrix product.  Checked against the
goldens in tests/test_pose_eval_cpu.py; the GPU tests compare the device with both.
"""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pose_eval.npz")

# the tolerances the goldens are held to (the reasoning: the docstring of tests/test_pose_eval_cpu.py)
ABS_POSED = 1e-10       # px: float64 distances, means and medians with H given
REL_RAW = 1e-6          # H=None (the reference works in float32 there) and the float32 mean_match_distance
REL_RATIO = 1e-12       # ratios of exact integers in the reference's order of operations


def warp(kp1, H):
    """(n, 2) float64: the float32 keypoints through H (9 float64 values, or None)."""
    x, y = kp1[:, 0].astype(np.float64), kp1[:, 1].astype(np.float64)
    if H is None:
        return np.stack([x, y], axis=1)
    h = np.asarray(H, dtype=np.float64).reshape(9)
    with np.errstate(divide="ignore", invalid="ignore"):
        X = (h[0] * x + h[1] * y) + h[2]
        Y = (h[3] * x + h[4] * y) + h[5]
        W = (h[6] * x + h[7] * y) + h[8]
        return np.stack([X / W, Y / W], axis=1)


def distances(kp1, kp2, H):
    """(n, m) float64 distances sqrt(dx*dx + dy*dy) from the warped kp1 to kp2."""
    w = warp(kp1, H)
    k2 = kp2.astype(np.float64)
    with np.errstate(invalid="ignore"):
        dx, dy = w[:, None, 0] - k2[None, :, 0], w[:, None, 1] - k2[None, :, 1]
        return np.sqrt(dx * dx + dy * dy)


def pose_nn(kp1, kp2, H, threshold):
    """One pair: dict of gt_matches (n, 2) int64 zero-padded, gt_count, gt_of_row (n,) int32, dist_sum, dist_median, min_dists."""
    d = distances(kp1, kp2, H)
    nn = d.argmin(axis=1)                                   # the first index among equal distances
    md = d[np.arange(len(d)), nn]
    keep = md < threshold
    idx1 = np.where(keep)[0]
    gt = np.zeros((len(d), 2), np.int64)
    gt[:len(idx1)] = np.stack([idx1, nn[idx1]], axis=1)
    return dict(gt_matches=gt, gt_count=int(keep.sum()), gt_of_row=np.where(keep, nn, -1).astype(np.int32), dist_sum=float(md.sum()),
                dist_median=float(np.median(md)), min_dists=md)


def absent(n):
    return dict(gt_matches=np.zeros((n, 2), np.int64), gt_count=0, gt_of_row=np.full(n, -1, np.int32), dist_sum=0.0, dist_median=0.0,
                min_dists=np.zeros(n))


def pose_nn_pairs(bank, first, second, H, threshold):
    """The listed pairs of a bank (n_bank, K, 2): a list of pose_nn dicts, absent pairs as the entry writes them."""
    out = []
    for p, (a, b) in enumerate(zip(first, second)):
        if not (0 <= a < len(bank) and 0 <= b < len(bank)):
            out.append(absent(bank.shape[1]))
        else:
            out.append(pose_nn(bank[a], bank[b], None if H is None else H[p], threshold))
    return out


def match_score(pred, values, gt_of_row, gt_count):
    """tp, fp, fn, value_sum of one pair's list pred (c, 2) / values (c,) against gt_of_row / gt_count."""
    pred = np.asarray(pred).reshape(-1, 2)
    tp = int(sum(0 <= i < len(gt_of_row) and gt_of_row[i] == j for i, j in pred))
    return tp, len(pred) - tp, int(gt_count) - tp, float(np.asarray(values, dtype=np.float64).sum())


def margins(kp1, kp2, H, threshold):
    """The two figures the fixture generator holds every case to, from the float64 distances: min |dist - threshold| over the
    rows, and over the rows inside the threshold the least gap to the nearest point at ANOTHER location (inf without one)."""
    d = distances(kp1, kp2, H)
    md = d.min(axis=1)
    with np.errstate(invalid="ignore"):
        edge = float(np.min(np.abs(md - threshold)))
    gap = np.inf
    for i in np.where(md < threshold)[0]:
        j = d[i].argmin()
        other = np.any(kp2 != kp2[j], axis=1)
        if other.any():
            gap = min(gap, float(d[i][other].min() - md[i]))
    return edge, gap


# ------------------------------------------------------------------------------------------------------------ the goldens
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as g:
            _golden = {key: g[key] for key in g.files}
    return _golden


def group_names():
    return [str(s) for s in golden()["groups"]]


def group(name: str) -> dict:
    """One device-call-sized case: bank (n_bank, K, 2) fp32, first / second int32, H (P, 9) float64 or None, threshold, and the
    reference's per-pair outputs count, mean, median, repeatability (P,), gt (P, K, 2) int64 zero-padded (None with H=None, where
    the reference has no ground-truth matches); with lists: pred (P, K, 2) int64, pred_count (P,), pred_value (P, K) fp32 and the
    reference's metrics (P, 9) float64 in the order of METRIC_KEYS."""
    g = golden()
    out = dict(name=name, bank=g["bank_" + str(g[name + "_bank"])], first=g[name + "_first"], second=g[name + "_second"],
               threshold=float(g[name + "_thr"]), count=g[name + "_count"], mean=g[name + "_mean"], median=g[name + "_median"],
               rep=g[name + "_rep"])
    H = g[name + "_H"]
    out["H"] = H if H.size else None
    out["gt"] = g[name + "_gt"].astype(np.int64) if name + "_gt" in g else None
    if name + "_pred" in g:
        out.update(pred=g[name + "_pred"].astype(np.int64), pred_count=g[name + "_pred_count"], pred_value=g[name + "_pred_value"],
                   metrics=g[name + "_metrics"])
    return out


METRIC_KEYS = ("tp", "fp", "fn", "precision", "recall", "f1", "inlier_ratio", "num_pred_matches", "num_gt_matches")
REP_SUMMARY_KEYS = ("num_pairs", "mean_repeatability", "std_repeatability", "median_repeatability", "min_repeatability",
                    "max_repeatability", "mean_distance", "median_distance")
REP_RESULT_KEYS = ("repeatability", "repeatable_count", "total_keypoints", "mean_nn_distance", "median_nn_distance")
DQ_SUMMARY_KEYS = ("num_pairs", "mean_precision", "std_precision", "mean_recall", "std_recall", "mean_f1", "std_f1",
                   "mean_inlier_ratio", "std_inlier_ratio", "mean_num_matches", "mean_match_distance")
DQ_RESULT_KEYS = METRIC_KEYS + ("mean_match_distance",)
INT_KEYS = ("num_pairs", "repeatable_count", "total_keypoints", "tp", "fp", "fn", "num_pred_matches", "num_gt_matches")
RAW_KEYS = ("mean_match_distance",)                       # float32 in the reference whatever H is


def dropin_names():
    return [str(s) for s in golden()["dropins"]]


def dropin(name: str) -> dict:
    """One call of the drop-in functions: kpts1 (N, 2), kpts2 (M, 2) fp32, H (3, 3) or None, threshold and the reference's
    dictionary values rep (REP_RESULT_KEYS order) and gt (count, 2) int64 (None with H=None)."""
    g = golden()
    H = g[name + "_H"]
    return dict(name=name, kpts1=g[name + "_kp1"], kpts2=g[name + "_kp2"], H=H.reshape(3, 3) if H.size else None,
                threshold=float(g[name + "_thr"]), rep=g[name + "_rep"], gt=g[name + "_gt"].astype(np.int64) if name + "_gt" in g else None)


def sequence_names():
    return [str(s) for s in golden()["sequences"]]


def sequence(name: str) -> dict:
    """One run of the reference's two test_sequence methods on the 12-frame synthetic sequence: spacing, num_pairs, use_pose and
    the summaries - rep_summary / dq_summary (the scalar keys in the order of *_SUMMARY_KEYS) and rep_results (P, 5) /
    dq_results (P, 10) (the per-pair dictionaries in the order of *_RESULT_KEYS); dq_* are None where the run had no poses."""
    g = golden()
    out = dict(name=name, spacing=int(g[name + "_spacing"]), num_pairs=int(g[name + "_num_pairs"]), use_pose=bool(g[name + "_use_pose"]),
               rep_summary=g[name + "_rep_summary"], rep_results=g[name + "_rep_results"])
    out["dq_summary"] = g[name + "_dq_summary"] if name + "_dq_summary" in g else None
    out["dq_results"] = g[name + "_dq_results"] if name + "_dq_results" in g else None
    return out


def sequence_inputs():
    """tokens (12, 5 + 28 * 28, 384) of the synthetic sequence (from tests/synth.py seeds), its poses (12, 4, 4) float64 (stored) and
    the weights' seeds: what the sequence goldens were computed from."""
    import synth
    return dict(tokens=synth.token_sequence(SEQ_FRAMES, SEQ_GRID), poses=golden()["seq_poses"], selector=synth.selector_state(0),
                refiner=synth.refiner_state(0))


SEQ_FRAMES, SEQ_GRID, SEQ_K = 12, 28, 500


def close(a, b, key: str, posed: bool) -> bool:
    """a (ours) against b (the reference's) for one dictionary key, by the tolerance its kind is held to."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if key in INT_KEYS:
        return bool(np.array_equal(a, b))
    if "distance" in key:
        if key in RAW_KEYS or not posed:
            return bool(np.all(np.abs(a - b) <= REL_RAW * np.abs(b)))
        with np.errstate(invalid="ignore"):
            return bool(np.all((np.abs(a - b) <= ABS_POSED) | (a == b)))              # a == b: infinite distances
    return bool(np.all(np.abs(a - b) <= REL_RATIO * np.abs(b)))


def summary_rows(summary: dict, keys, result_keys):
    """A test_sequence dictionary as (scalars in `keys` order, per-pair rows in `result_keys` order), float64."""
    return (np.array([summary[key] for key in keys], dtype=np.float64),
            np.array([[r[key] for key in result_keys] for r in summary["all_results"]], dtype=np.float64))


def check_summary(summary, want_scalars, want_rows, keys, result_keys, posed, what):
    """A summary of sslam_amd.evaluation against the reference's: its keys in its order, every value by the tolerance of its kind."""
    assert list(summary) == ["sequence"] + list(keys) + ["all_results"], f"{what}: test_sequence's keys, in its order"
    scalars, rows = summary_rows(summary, keys, result_keys)
    assert all(list(r) == list(result_keys) for r in summary["all_results"]), what
    assert rows.shape == want_rows.shape, what
    for i, key in enumerate(keys):
        assert close(scalars[i], want_scalars[i], key, posed), (what, key, scalars[i], want_scalars[i])
    for j, key in enumerate(result_keys):
        assert close(rows[:, j], want_rows[:, j], key, posed), (what, key, rows[:, j], want_rows[:, j])
