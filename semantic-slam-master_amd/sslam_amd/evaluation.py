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

A second, opt-in ground truth uses the D of RGB-D (depth=, camera=; csrc/evaluate.hip): every keypoint is back-projected
with its depth, moved by the full relative pose relative_transform = inv(pose_b) @ pose_a (float64, not rounded) and projected
into the other frame with the sequence's own intrinsics (Camera; tum.camera_for).  A keypoint without a depth measurement, behind
the other camera or outside its view has no ground truth: it leaves the repeatability's denominator, and a match on it is counted
as unknown, not as wrong.  Without depth= every function returns what it returned before.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import lib
from .pipeline import MatchRule, _np
from .readback import Readback

TUM_K = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])      # test_repeatability.py:179-183

_REP_KEYS = ("gt_count", "dist_sum", "dist_median")
_DQ_KEYS = ("gt_count", "tp", "fp", "fn", "value_sum", "match_count")
_SUMS = ("value_sum", "dist_sum", "dist_median")       # the float64 figures among the per-pair numbers; the others are counts


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


@dataclass(frozen=True)
class Camera:
    """Pinhole intrinsics of the depth image, in ITS pixels (width x height), and the raw-depth units per metre.  The defaults
    are the constants of the ROS driver that TUM's tools assume for any sequence; tum.camera_for names the calibrated ones."""
    fx: float = 525.0
    fy: float = 525.0
    cx: float = 319.5
    cy: float = 239.5
    depth_scale: float = 5000.0
    width: int = 640
    height: int = 480


def relative_transform(pose_a, pose_b) -> np.ndarray:
    """inv(pose_b) @ pose_a, (4, 4) float64, NOT rounded to float32.  TUM's groundtruth.txt poses are camera-to-world, so this is
    the map that takes camera-a coordinates to camera-b coordinates: X_b = inv(pose_b) pose_a X_a.
    It deliberately differs from relative_pose, which stays the reference's pose2 @ inv(pose1) (rounded to float32) for the
    homography path: that product is the reference's own convention and the existing figures are pinned to it; this one is
    the geometry a point with a depth needs."""
    pose_a, pose_b = np.asarray(pose_a, dtype=np.float64), np.asarray(pose_b, dtype=np.float64)
    if pose_a.shape != (4, 4) or pose_b.shape != (4, 4):
        raise ValueError(f"two 4 x 4 poses expected, got {pose_a.shape} and {pose_b.shape}")
    return np.linalg.inv(pose_b) @ pose_a


def pair_transforms(poses, pairs) -> np.ndarray:
    """(P, 3, 4) float64: the [R | t] rows of relative_transform(poses[a], poses[b]) for every pair (a, b)."""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f"poses (N, 4, 4) expected, got {poses.shape}")
    if any(not (0 <= a < len(poses) and 0 <= b < len(poses)) for a, b in pairs):
        raise ValueError(f"{len(poses)} poses do not cover the pairs")
    return np.stack([relative_transform(poses[a], poses[b])[:3] for a, b in pairs]) if pairs else np.zeros((0, 3, 4))


def _pair_arrays(stats: dict, keys) -> dict:
    missing = [key for key in keys + ("num_keypoints",) if key not in stats]
    if missing:
        raise ValueError(f"stats lack {missing}")
    out = {key: _np(stats[key]) for key in keys}
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


_DEPTH_REP_KEYS = ("gt_count", "valid_count", "dist_sum", "dist_median")
_DEPTH_DQ_KEYS = ("gt_count", "tp", "fp", "fn", "unknown", "value_sum", "match_count")


def _with_ground_truth(valid, what):
    """Indices of the pairs that have at least one row with ground truth; ValueError if none has."""
    keep = [i for i, v in enumerate(valid) if int(v) > 0]
    if not keep:
        raise ValueError(f"{what}: no pair has a keypoint with ground truth (no depth under any keypoint, or no overlap of the views)")
    return keep


def depth_repeatability_summary(stats: dict, sequence: str = "") -> dict:
    """repeatability_summary for the depth ground truth, from per-pair gt_count, valid_count, dist_sum, dist_median and the
    number num_keypoints.  Per pair: repeatability = gt_count / valid_count and mean_nn_distance = dist_sum / valid_count (0.0 on a
    zero denominator), repeatable_count, total_keypoints, valid_keypoints, median_nn_distance.  The summary's keys are
    repeatability_summary's plus pairs_without_ground_truth: the pairs with valid_count == 0, which stay in all_results and are
    left out of every mean, median, min and max; ValueError if every pair is one."""
    s, k = _pair_arrays(stats, _DEPTH_REP_KEYS), int(stats["num_keypoints"])
    results = []
    for c, v, dsum, dmed in zip(*(s[key] for key in _DEPTH_REP_KEYS)):
        v = np.int64(v)
        results.append({"repeatability": np.int64(c) / v if v > 0 else 0.0, "repeatable_count": np.int64(c), "total_keypoints": k,
                        "valid_keypoints": v, "mean_nn_distance": np.float64(dsum) / v if v > 0 else 0.0,
                        "median_nn_distance": np.float64(dmed)})
    keep = _with_ground_truth(s["valid_count"], "repeatability")
    rep = [results[i]["repeatability"] for i in keep]
    md = [results[i]["mean_nn_distance"] for i in keep]
    return {"sequence": sequence, "num_pairs": len(results), "pairs_without_ground_truth": len(results) - len(keep),
            "mean_repeatability": np.mean(rep), "std_repeatability": np.std(rep), "median_repeatability": np.median(rep),
            "min_repeatability": np.min(rep), "max_repeatability": np.max(rep), "mean_distance": np.mean(md),
            "median_distance": np.median(md), "all_results": results}


def known_match_metrics(tp: int, fp: int, fn: int, unknown: int, num_pred: int, num_gt: int) -> dict:
    """match_metrics where `unknown` of the num_pred matches sit on a keypoint without ground truth: tp + fp + unknown = num_pred,
    inlier_ratio = tp / (num_pred - unknown) (0.0 on a zero denominator); precision, recall and f1 from tp, fp, fn as there."""
    m = match_metrics(tp, fp, fn, num_pred, num_gt)
    known = int(num_pred) - int(unknown)
    m["inlier_ratio"] = int(tp) / known if known > 0 else 0.0
    m["num_unknown_matches"] = int(unknown)
    return m


def depth_descriptor_quality_summary(stats: dict, sequence: str = "") -> dict:
    """descriptor_quality_summary for the depth ground truth, from per-pair gt_count, tp, fp, fn, unknown, value_sum, match_count
    and valid_count.  Per pair known_match_metrics plus valid_keypoints and mean_match_distance; the summary's keys are
    descriptor_quality_summary's plus pairs_without_ground_truth, and such pairs are left out of the means as in
    depth_repeatability_summary."""
    s = _pair_arrays(stats, _DEPTH_DQ_KEYS + ("valid_count",))
    results = []
    for g, tp, fp, fn, un, vs, c, v in zip(*(s[key] for key in _DEPTH_DQ_KEYS + ("valid_count",))):
        m = known_match_metrics(tp, fp, fn, un, c, g)
        m["valid_keypoints"] = int(v)
        m["mean_match_distance"] = float(vs) / int(c) if int(c) > 0 else 0.0
        results.append(m)
    keep = _with_ground_truth(s["valid_count"], "descriptor quality")
    out = {"sequence": sequence, "num_pairs": len(results), "pairs_without_ground_truth": len(results) - len(keep)}
    for key in ("precision", "recall", "f1", "inlier_ratio"):
        out[f"mean_{key}"] = np.mean([results[i][key] for i in keep])
        out[f"std_{key}"] = np.std([results[i][key] for i in keep])
    out["mean_num_matches"] = np.mean([results[i]["num_pred_matches"] for i in keep])
    out["mean_match_distance"] = np.mean([results[i]["mean_match_distance"] for i in keep])
    out["all_results"] = results
    return out


DEPTH_CHUNK = 64        # depth frames uploaded per gather launch: 64 x 480 x 640 uint16 = 39 MB on the device at a time


def check_depth_size(width: int, height: int, camera) -> None:
    """ValueError unless depth images of width x height pixels are what `camera` describes."""
    _, _, _, _, _, w, h = lib.check_camera(camera)
    if (int(width), int(height)) != (w, h):
        raise ValueError(f"depth images of {int(width)} x {int(height)} pixels, the camera describes {w:g} x {h:g}")


def _check_depth(depth, kp_depth, poses, use_pose, camera, keypoints_shape, n_frames):
    """The depth= / kp_depth= / camera= arguments of evaluate / evaluate_result, before any device work -> the Camera to use."""
    if poses is None:
        raise ValueError("depth= needs poses (N, 4, 4): the depth ground truth moves every point by the full relative pose")
    if not use_pose:
        raise ValueError("depth= scores against the poses: it has no use_pose=False form")
    camera = Camera() if camera is None else camera
    lib.check_camera(camera)
    if kp_depth is not None:
        if depth is not None:
            raise ValueError("depth= and kp_depth= are two forms of one argument: pass one")
        if not isinstance(kp_depth, torch.Tensor) or kp_depth.dtype != torch.int32 or tuple(kp_depth.shape) != tuple(keypoints_shape[:2]):
            raise ValueError(f"kp_depth must be the int32 tensor {tuple(keypoints_shape[:2])} gather_keypoint_depth returned for these keypoints")
        return camera
    ok = (isinstance(depth, np.ndarray) and depth.dtype == np.uint16) or (isinstance(depth, torch.Tensor) and depth.dtype == torch.uint16)
    if not ok or depth.ndim != 3:
        raise ValueError("depth must be (N, h, w) uint16 raw depth images, numpy or tensor")
    if int(depth.shape[0]) < n_frames:
        raise ValueError(f"depth holds {int(depth.shape[0])} frames, the pairs name {n_frames}")
    check_depth_size(depth.shape[2], depth.shape[1], camera)
    return camera


def check_subcell(subcell):
    """subcell= of the scoring and odometry calls: None (follow the pipeline), True or False - judged before any device work."""
    if subcell not in (None, False, True):
        raise ValueError(f"subcell must be None, True or False, got {subcell!r}")
    return subcell


def geometry_bank(frames: dict, subcell=None):
    """The keypoint bank (N, K, 2) geometry reads from an extract() dictionary or a result's "frames": subcell None - the refined
    keypoints_subpixel where the pipeline wrote them (ExtractorConfig.subcell), else the cell centres keypoints_pixel
    (SequencePipeline.geometry_keypoints); False - the cell centres whatever is there; True - the refined ones, or ValueError."""
    check_subcell(subcell)
    if subcell is False:
        return frames["keypoints_pixel"]
    if subcell and "keypoints_subpixel" not in frames:
        raise ValueError("subcell=True needs the refined keypoints: build the pipeline with ExtractorConfig(subcell=True)")
    return frames["keypoints_subpixel"] if "keypoints_subpixel" in frames else frames["keypoints_pixel"]


def gather_keypoint_depth(pipe, depth, keypoints_pixel, n_frames: int):
    """(N, K) int32 device bank of the raw depth under every keypoint of the first n_frames frames (-1 in the frames behind them):
    the depth images go to the device DEPTH_CHUNK frames at a time and do not stay there."""
    kp_depth = torch.full(tuple(keypoints_pixel.shape[:2]), -1, dtype=torch.int32, device=keypoints_pixel.device)
    for a in range(0, n_frames, DEPTH_CHUNK):
        b = min(a + DEPTH_CHUNK, n_frames)
        d = depth[a:b]
        d = torch.from_numpy(np.ascontiguousarray(d)) if isinstance(d, np.ndarray) else d
        pipe.keypoint_depth(d.to(keypoints_pixel.device).contiguous(), keypoints_pixel[a:b], out=kp_depth[a:b])
    return kp_depth


def _score_depth(pipe, keypoints_pixel, pairs, poses, depth, camera, threshold: float, matches: dict, sequence: str,
                 kp_depth=None) -> dict:
    """_score against the depth ground truth: the gather (unless kp_depth holds its result already), the two scoring launches, ONE
    host read-back of the ten per-pair figures."""
    lib.check_threshold(threshold)
    first, second = [a for a, _ in pairs], [b for _, b in pairs]
    T = pair_transforms(poses, pairs)
    k = int(keypoints_pixel.shape[1])
    if kp_depth is None:
        kp_depth = gather_keypoint_depth(pipe, depth, keypoints_pixel, pairs[-1][1] + 1)
    sc = pipe.pose_depth_scores(keypoints_pixel, kp_depth, first, second, T, camera, threshold, matches=matches)
    rb = Readback()
    for key in _DEPTH_DQ_KEYS + ("valid_count", "dist_sum", "dist_median"):
        rb.add(key, sc[key] if key != "match_count" else matches["match_count"], np.float64 if key in _SUMS else np.int64)
    st = dict(rb.fetch(), num_keypoints=k)                  # the ONE read-back
    return {"repeatability": depth_repeatability_summary(st, sequence), "descriptor_quality": depth_descriptor_quality_summary(st, sequence)}


def _score(pipe, keypoints_pixel, pairs, poses, use_pose: bool, threshold: float, matches: dict, sequence: str) -> dict:
    """Score the listed pairs of a keypoint bank and, with poses, their M4 lists; ONE host read-back of the per-pair figures."""
    if poses is None and use_pose:
        raise ValueError("use_pose=True needs poses (N, 4, 4); pass use_pose=False for the raw repeatability")
    if not pairs:
        raise ValueError("no pairs to evaluate")
    lib.check_threshold(threshold)
    first, second = [a for a, _ in pairs], [b for _, b in pairs]
    H = None if poses is None else pair_homographies(poses, pairs)
    k = int(keypoints_pixel.shape[1])
    rb = Readback()
    if H is not None:                                    # descriptor quality: always against the posed ground truth
        dq = pipe.pose_scores(keypoints_pixel, first, second, H, threshold, matches=matches)
        for key in _DQ_KEYS:
            rb.add("dq." + key, dq[key] if key != "match_count" else matches["match_count"], np.float64 if key in _SUMS else np.int64)
    rep = dq if (H is not None and use_pose) else pipe.pose_scores(keypoints_pixel, first, second, None, threshold)
    for key in _REP_KEYS:
        rb.add("rep." + key, rep[key], np.float64 if key in _SUMS else np.int64)
    host = rb.fetch()                                    # the ONE read-back
    of = lambda prefix, keys: dict({key: host[prefix + key] for key in keys}, num_keypoints=k)
    return {"descriptor_quality": None if H is None else descriptor_quality_summary(of("dq.", _DQ_KEYS), sequence),
            "repeatability": repeatability_summary(of("rep.", _REP_KEYS), sequence)}


def evaluate(pipe, images_u8=None, poses=None, spacing: int = 1, num_pairs: int = 50, use_pose: bool = True,
             ratio_threshold: float = 0.9, threshold: float = 3.0, tokens=None, sequence: str = "", *, depth=None,
             camera=None, subcell=None) -> dict:
    """Score a checkpoint the way the reference's two testers score it, on the device: the frames images_u8 (N, H, W, 3) uint8
    (a pipeline built with vit=) or their ViT tokens (tokens=, as SequencePipeline.run takes them), the camera poses (N, 4, 4)
    float64 as TUMSequence.poses holds them.  Only the first num_pairs + spacing frames are used, as the testers' max_frames cuts
    them; they are extracted once, the pairs pair_list(...) matched under MatchRule.mnn_ratio(ratio_threshold) and scored at
    `threshold` pixels; the per-pair numbers are read back once, at the end.
    use_pose=False: the repeatability of the raw coordinates (the tester's --no_pose).  Descriptor quality needs poses, as in the
    reference: without them its entry is None; poses=None with use_pose=True raises ValueError.
    depth=: the frames' raw depth images (N, h, w) uint16, numpy or tensor (TUMSequence.load_depth_raw), and camera=: their
    Camera (tum.camera_for; the default Camera() if left out) - the pairs are then scored against the translation-aware ground
    truth: the depth under every keypoint is gathered chunk by chunk for the frames used, and the two dictionaries come from
    depth_repeatability_summary / depth_descriptor_quality_summary (extra keys: valid_keypoints, num_unknown_matches,
    pairs_without_ground_truth).  depth= needs poses and use_pose=True.
    subcell: on a pipeline with ExtractorConfig(subcell=True) the depth lookups and every score read the refined keypoints
    (geometry_bank); subcell=False forces the cell centres.  The matcher is the same either way.
    Returns {'repeatability': RepeatabilityTester.test_sequence's dictionary, 'descriptor_quality':
    DescriptorQualityTester.test_sequence's} (repeatability_summary / descriptor_quality_summary state the keys)."""
    check_subcell(subcell)
    if depth is None and camera is not None:
        raise ValueError("camera= describes the depth images: it needs depth=")
    if depth is not None and poses is None:
        raise ValueError("depth= needs poses (N, 4, 4): the depth ground truth moves every point by the full relative pose")
    if poses is None and use_pose:
        raise ValueError("use_pose=True needs poses (N, 4, 4); pass use_pose=False for the raw repeatability")
    src = tokens if tokens is not None else images_u8
    if src is None:
        raise ValueError("images_u8 or tokens= required")
    pairs = pair_list(int(src.shape[0]), spacing, num_pairs)
    if not pairs:
        raise ValueError(f"{int(src.shape[0])} frames hold no pair at spacing {spacing}")
    n = pairs[-1][1] + 1
    if depth is not None:
        camera = _check_depth(depth, None, poses, use_pose, camera, None, n)
    rule = MatchRule.mnn_ratio(ratio_threshold)
    ex = pipe.extract(pipe.tokens_from_images(images_u8[:n]) if tokens is None else tokens[:n], None)
    matches = None
    if poses is not None:
        matches = pipe.match_pairs(ex["descriptors"], ex["scores"], first=[a for a, _ in pairs], second=[b for _, b in pairs], rule=rule)
    kp = geometry_bank(ex, subcell)
    if depth is not None:
        return _score_depth(pipe, kp, pairs, poses, depth, camera, threshold, matches, sequence)
    return _score(pipe, kp, pairs, poses, use_pose, threshold, matches, sequence)


def evaluate_result(pipe, result: dict, poses, spacing: int = 1, num_pairs: int = 50, use_pose: bool = True,
                    threshold: float = 3.0, sequence: str = "", *, depth=None, camera=None, kp_depth=None, subcell=None) -> dict:
    """evaluate() for a StreamingSequence.result() / run_frames / run_directory result that was matched under
    MatchRule.mnn_ratio (rule=): the keypoints and the M4 lists of every pair (i, i + spacing) are already in device memory, so
    nothing is extracted or matched again - the first min(num_pairs, N - spacing) rows of result[spacing] are scored.
    depth=, camera=: as in evaluate() - the raw depth images of the result's frames.  kp_depth=: instead of depth=, the (N, K) int32
    bank gather_keypoint_depth(pipe, depth, result["frames"]["keypoints_pixel"], n) returned - it depends on the frames alone, so a
    caller that scores several spacings gathers once, for the most frames any spacing names, and passes it to each call.
    subcell: as in evaluate() - a result of a pipeline with subcell=True is scored on its refined keypoints unless subcell=False;
    a kp_depth= bank must have been gathered under the same bank (geometry_bank(result["frames"], subcell))."""
    depth_given = depth is not None or kp_depth is not None
    if not depth_given and camera is not None:
        raise ValueError("camera= describes the depth images: it needs depth=")
    if depth_given and poses is None:
        raise ValueError("depth= needs poses (N, 4, 4): the depth ground truth moves every point by the full relative pose")
    if poses is None and use_pose:
        raise ValueError("use_pose=True needs poses (N, 4, 4); pass use_pose=False for the raw repeatability")
    if not isinstance(result, dict) or "frames" not in result or "keypoints_pixel" not in result["frames"]:
        raise ValueError("a StreamingSequence / run_directory result expected")
    kp = geometry_bank(result["frames"], subcell)
    pairs = pair_list(int(kp.shape[0]), spacing, num_pairs)
    if not pairs or spacing not in result:
        raise ValueError(f"the result holds no pair at spacing {spacing}")
    mm = result[spacing]
    if "value" not in mm:
        raise ValueError("the result was not matched under a rule: run it with rule=MatchRule.mnn_ratio(...)")
    p = len(pairs)
    matches = None if poses is None else {key: mm[key][:p] for key in ("matches", "value", "match_count")}
    if depth_given:
        camera = _check_depth(depth, kp_depth, poses, use_pose, camera, kp.shape, pairs[-1][1] + 1)
        return _score_depth(pipe, kp, pairs, poses, depth, camera, threshold, matches, sequence, kp_depth)
    return _score(pipe, kp, pairs, poses, use_pose, threshold, matches, sequence)
