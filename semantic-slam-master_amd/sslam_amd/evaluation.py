"""Pose-based scoring of a checkpoint: the reference's two headline quality figures - keypoint repeatability
(RepeatabilityTester.test_sequence, test/test_repeatability.py:130-215) and descriptor quality
(DescriptorQualityTester.test_sequence, test/test_descriptor_quality.py:233-305) - from the per-pair numbers of the HIP
scoring stage (SequencePipeline.pose_scores; csrc/evaluate.hip).

The reference walks the pairs (i, i + spacing) one at a time on host numpy, extracting both frames of every pair.  Here every
frame is extracted once, all pairs are matched under M4 (MatchRule.mnn_ratio) and scored in a few launches, and the per-pair
integers and float64 sums are read back once; the functions below - small host functions in float64 - put the two summary
dictionaries together from them, in the reference's order of operations:

  per pair, repeatability     repeatability = repeatable / K, mean_nn_distance = dist_sum / K, median_nn_distance = dist_median
  per pair, descriptor quality  precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 p r / (p + r),
                              inlier_ratio = tp / num_pred_matches - each 0.0 on a zero denominator, as evaluate_matches has it -
                              and mean_match_distance = value_sum / num_pred_matches (0.0 for an empty list)
  summaries                   np.mean / np.std / np.median / np.min / np.max over the pairs, key for key the reference's

The warp is the reference's: H = K R K^-1 with the TUM intrinsics 525 / 319.5 / 239.5 (test_repeatability.py:179-192), R the
rotation of the relative pose pose2 pose1^-1 ROUNDED TO FLOAT32 (data/tum_dataset.py:191-195 hands it over as a float tensor);
the translation is ignored, as there.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib
from .pipeline import MatchRule

TUM_K = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])      # test_repeatability.py:179-183

_REP_KEYS = ("gt_count", "dist_sum", "dist_median")
_DQ_KEYS = ("gt_count", "tp", "fp", "fn", "value_sum", "match_count")


def relative_pose(pose1, pose2) -> np.ndarray:
    """T_rel = pose2 @ inv(pose1) in float64, rounded to float32 once (tum_dataset.py:191, :195)."""
    pose1, pose2 = np.asarray(pose1, dtype=np.float64), np.asarray(pose2, dtype=np.float64)
    if pose1.shape != (4, 4) or pose2.shape != (4, 4):
        raise ValueError(f"two 4 x 4 poses expected, got {pose1.shape} and {pose2.shape}")
    return (pose2 @ np.linalg.inv(pose1)).astype(np.float32)


def homography(T_rel, K=TUM_K) -> np.ndarray:
    """H = K @ R @ inv(K) in float64, R = T_rel[:3, :3] as it is (float32 from relative_pose): test_repeatability.py:186-192."""
    T_rel = np.asarray(T_rel)
    if T_rel.shape != (4, 4):
        raise ValueError(f"a 4 x 4 relative pose expected, got {T_rel.shape}")
    K = np.asarray(K, dtype=np.float64)
    return K @ T_rel[:3, :3] @ np.linalg.inv(K)


def pair_list(n_frames: int, spacing: int = 1, num_pairs: int = 50) -> list:
    """The pairs the two testers visit: (i, i + spacing) for i < min(num_pairs, n - spacing) with n = min(n_frames,
    num_pairs + spacing) - their TUMDataset(frame_spacing=spacing, max_frames=num_pairs + spacing) - NOT the strided walk of
    visualize_matches_sequence.py's process_spacing."""
    for name, v, lo in (("n_frames", n_frames, 0), ("spacing", spacing, 1), ("num_pairs", num_pairs, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    n = min(int(n_frames), int(num_pairs) + int(spacing))
    return [(i, i + int(spacing)) for i in range(min(int(num_pairs), max(0, n - int(spacing))))]


def pair_homographies(poses, pairs, K=TUM_K) -> np.ndarray:
    """(P, 3, 3) float64: homography(relative_pose(poses[a], poses[b])) for every pair (a, b)."""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f"poses (N, 4, 4) expected, got {poses.shape}")
    if any(not (0 <= a < len(poses) and 0 <= b < len(poses)) for a, b in pairs):
        raise ValueError(f"{len(poses)} poses do not cover the pairs")
    return np.stack([homography(relative_pose(poses[a], poses[b]), K) for a, b in pairs]) if pairs else np.zeros((0, 3, 3))


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _pair_arrays(stats: dict, keys) -> dict:
    missing = [key for key in keys + ("num_keypoints",) if key not in stats]
    if missing:
        raise ValueError(f"stats lack {missing}")
    out = {key: _host(stats[key]) for key in keys}
    n = {len(v) for v in out.values()}
    if len(n) != 1 or 0 in n:
        raise ValueError("stats must hold one entry per pair, for at least one pair")
    return out


def repeatability_summary(stats: dict, sequence: str = "") -> dict:
    """RepeatabilityTester.test_sequence's dictionary from per-pair gt_count, dist_sum, dist_median and the number
    num_keypoints: sequence, num_pairs, mean / std / median / min / max_repeatability, mean_distance, median_distance (both over
    the per-pair MEANS, as there) and all_results - per pair repeatability, repeatable_count, total_keypoints,
    mean_nn_distance, median_nn_distance."""
    s, k = _pair_arrays(stats, _REP_KEYS), int(stats["num_keypoints"])
    results = []
    for c, dsum, dmed in zip(s["gt_count"], s["dist_sum"], s["dist_median"]):
        results.append({"repeatability": np.int64(c) / k, "repeatable_count": np.int64(c), "total_keypoints": k,
                        "mean_nn_distance": np.float64(dsum) / k, "median_nn_distance": np.float64(dmed)})
    rep = [r["repeatability"] for r in results]
    md = [r["mean_nn_distance"] for r in results]
    return {"sequence": sequence, "num_pairs": len(results), "mean_repeatability": np.mean(rep), "std_repeatability": np.std(rep),
            "median_repeatability": np.median(rep), "min_repeatability": np.min(rep), "max_repeatability": np.max(rep),
            "mean_distance": np.mean(md), "median_distance": np.median(md), "all_results": results}


def match_metrics(tp: int, fp: int, fn: int, num_pred: int, num_gt: int) -> dict:
    """evaluate_matches' dictionary from its three counts (test_descriptor_quality.py:213-231), zero denominators as there."""
    tp, fp, fn, num_pred, num_gt = int(tp), int(fp), int(fn), int(num_pred), int(num_gt)
    precision = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0.0
    inlier_ratio = tp / num_pred if num_pred > 0 else 0.0
    return {"tp": tp, "fp": fp, "fn": fn, "precision": precision, "recall": recall, "f1": f1, "inlier_ratio": inlier_ratio,
            "num_pred_matches": num_pred, "num_gt_matches": num_gt}


def descriptor_quality_summary(stats: dict, sequence: str = "") -> dict:
    """DescriptorQualityTester.test_sequence's dictionary from per-pair gt_count, tp, fp, fn, value_sum and match_count:
    sequence, num_pairs, mean / std of precision, recall, f1 and inlier_ratio, mean_num_matches, mean_match_distance and
    all_results - per pair evaluate_matches' dictionary plus mean_match_distance."""
    s = _pair_arrays(stats, _DQ_KEYS)
    results = []
    for g, tp, fp, fn, vs, c in zip(*(s[key] for key in _DQ_KEYS)):
        m = match_metrics(tp, fp, fn, c, g)
        m["mean_match_distance"] = float(vs) / int(c) if int(c) > 0 else 0.0
        results.append(m)
    out = {"sequence": sequence, "num_pairs": len(results)}
    for key in ("precision", "recall", "f1", "inlier_ratio"):
        out[f"mean_{key}"] = np.mean([r[key] for r in results])
        out[f"std_{key}"] = np.std([r[key] for r in results])
    out["mean_num_matches"] = np.mean([r["num_pred_matches"] for r in results])
    out["mean_match_distance"] = np.mean([r["mean_match_distance"] for r in results])
    out["all_results"] = results
    return out


def _score(pipe, keypoints_pixel, pairs, poses, use_pose: bool, threshold: float, matches: dict, sequence: str) -> dict:
    """Score the listed pairs of a keypoint bank and, with poses, their M4 lists; ONE host read-back of (rows, P) float64."""
    if poses is None and use_pose:
        raise ValueError("use_pose=True needs poses (N, 4, 4); pass use_pose=False for the raw repeatability")
    if not pairs:
        raise ValueError("no pairs to evaluate")
    lib.check_threshold(threshold)
    first, second = [a for a, _ in pairs], [b for _, b in pairs]
    H = None if poses is None else pair_homographies(poses, pairs)
    k = int(keypoints_pixel.shape[1])
    rows = []
    if H is not None:                                    # descriptor quality: always against the posed ground truth
        dq = pipe.pose_scores(keypoints_pixel, first, second, H, threshold, matches=matches)
        rows += [dq[key] if key != "match_count" else matches["match_count"] for key in _DQ_KEYS]
    rep = dq if (H is not None and use_pose) else pipe.pose_scores(keypoints_pixel, first, second, None, threshold)
    rows += [rep[key] for key in _REP_KEYS]
    host = torch.stack([r.to(torch.float64) for r in rows]).cpu().numpy()       # integers up to 4096: exact in float64
    out = {"descriptor_quality": None}
    if H is not None:
        st = {key: (host[i] if key == "value_sum" else host[i].astype(np.int64)) for i, key in enumerate(_DQ_KEYS)}
        out["descriptor_quality"] = descriptor_quality_summary(dict(st, num_keypoints=k), sequence)
        host = host[len(_DQ_KEYS):]
    st = {key: (host[i].astype(np.int64) if key == "gt_count" else host[i]) for i, key in enumerate(_REP_KEYS)}
    out["repeatability"] = repeatability_summary(dict(st, num_keypoints=k), sequence)
    return out


def evaluate(pipe, images_u8=None, poses=None, spacing: int = 1, num_pairs: int = 50, use_pose: bool = True,
             ratio_threshold: float = 0.9, threshold: float = 3.0, tokens=None, sequence: str = "") -> dict:
    """Score a checkpoint the way the reference's two testers score it, on the device: the frames images_u8 (N, H, W, 3) uint8
    (a pipeline built with vit=) or their ViT tokens (tokens=, as SequencePipeline.run takes them), the camera poses (N, 4, 4)
    float64 as TUMSequence.poses holds them.  Only the first num_pairs + spacing frames are used, as the testers' max_frames cuts
    them; they are extracted once, the pairs pair_list(...) matched under MatchRule.mnn_ratio(ratio_threshold) and scored at
    `threshold` pixels; the per-pair numbers are read back once, at the end.
    use_pose=False: the repeatability of the raw coordinates (the tester's --no_pose).  Descriptor quality needs poses, as in the
    reference: without them its entry is None; poses=None with use_pose=True raises ValueError.
    Returns {'repeatability': RepeatabilityTester.test_sequence's dictionary, 'descriptor_quality':
    DescriptorQualityTester.test_sequence's} (repeatability_summary / descriptor_quality_summary state the keys)."""
    if poses is None and use_pose:
        raise ValueError("use_pose=True needs poses (N, 4, 4); pass use_pose=False for the raw repeatability")
    src = tokens if tokens is not None else images_u8
    if src is None:
        raise ValueError("images_u8 or tokens= required")
    pairs = pair_list(int(src.shape[0]), spacing, num_pairs)
    if not pairs:
        raise ValueError(f"{int(src.shape[0])} frames hold no pair at spacing {spacing}")
    n = pairs[-1][1] + 1
    rule = MatchRule.mnn_ratio(ratio_threshold)
    ex = pipe.extract(pipe.tokens_from_images(images_u8[:n]) if tokens is None else tokens[:n], None)
    matches = None
    if poses is not None:
        matches = pipe.match_pairs(ex["descriptors"], ex["scores"], first=[a for a, _ in pairs], second=[b for _, b in pairs], rule=rule)
    return _score(pipe, ex["keypoints_pixel"], pairs, poses, use_pose, threshold, matches, sequence)


def evaluate_result(pipe, result: dict, poses, spacing: int = 1, num_pairs: int = 50, use_pose: bool = True,
                    threshold: float = 3.0, sequence: str = "") -> dict:
    """evaluate() for a StreamingSequence.result() / run_frames / run_directory result that was matched under
    MatchRule.mnn_ratio (rule=): the keypoints and the M4 lists of every pair (i, i + spacing) are already in device memory, so
    nothing is extracted or matched again - the first min(num_pairs, N - spacing) rows of result[spacing] are scored."""
    if poses is None and use_pose:
        raise ValueError("use_pose=True needs poses (N, 4, 4); pass use_pose=False for the raw repeatability")
    if not isinstance(result, dict) or "frames" not in result or "keypoints_pixel" not in result["frames"]:
        raise ValueError("a StreamingSequence / run_directory result expected")
    kp = result["frames"]["keypoints_pixel"]
    pairs = pair_list(int(kp.shape[0]), spacing, num_pairs)
    if not pairs or spacing not in result:
        raise ValueError(f"the result holds no pair at spacing {spacing}")
    mm = result[spacing]
    if "value" not in mm:
        raise ValueError("the result was not matched under a rule: run it with rule=MatchRule.mnn_ratio(...)")
    p = len(pairs)
    matches = None if poses is None else {key: mm[key][:p] for key in ("matches", "value", "match_count")}
    return _score(pipe, kp, pairs, poses, use_pose, threshold, matches, sequence)
