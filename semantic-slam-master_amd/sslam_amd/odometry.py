"""Frame-to-frame odometry from the device's own features: the relative pose of every pair from its match list and the depth under
the keypoints (SequencePipeline.estimate_poses; csrc/pose_estimate.hip), the chained trajectory, and the two figures the
reference judges itself against ORB-SLAM3 by - RPE and ATE (scripts/evaluate_baseline.py:57-129, which computes them with evo
for a baseline's trajectory file and has no way to produce either for its own features).

Everything here is host-side float64 numpy on the per-pair numbers read back ONCE: extraction, the depth gather, matching, the
RANSAC launch and - with refine=True - the refinement launch behind it (SequencePipeline.refine_poses; csrc/pose_refine.hip:
Gauss-Newton on the Huber reprojection cost over RANSAC's inliers) all stay on the device.

  per pair          E = inv(T_gt) @ T_est with T_gt = evaluation.relative_transform(pose_a, pose_b); the translation error is
                    |E[:3, 3]| in metres, the rotation error the angle of E[:3, :3] in degrees (evo's RPE of one pair);
                    inlier_ratio = inlier_count / match_count - a quality figure that needs no ground truth
  rpe_summary       rmse / mean / median / std (np.std, evo's) of both, the keys of the reference's compute_rpe
  ate_summary       the estimated positions aligned to the true ones by a rigid motion WITHOUT scale (Kabsch), then the same
                    statistics and min / max of the position errors: the keys of compute_ate
  chain             pose_{i+1} = pose_i @ inv(T_i): camera-to-world poses, as TUM's groundtruth.txt has them, from the
                    camera-i -> camera-(i+1) transforms of consecutive pairs

The keypoints are patch centres on a 16-pixel grid - or, on a pipeline with ExtractorConfig(subcell=True), the refined
keypoints_subpixel, which everything here then reads (evaluation.geometry_bank).  Nobody has measured which reprojection threshold suits them on real data:
no real RGB-D sequence was at hand when this was written.  3.0 keypoint units is only the scoring stage's default, taken over here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib
from .evaluation import Camera, check_depth_size, check_subcell, gather_keypoint_depth, geometry_bank, relative_transform
from .pipeline import MatchRule, PoseWeights

_INT_KEYS = ("inlier_count", "usable_count", "best_hypothesis", "refit_kept")


def _as44(T) -> np.ndarray:
    """(P, 4, 4) float64 from (P, 12), (P, 3, 4) or (P, 4, 4)."""
    T = np.asarray(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, dtype=np.float64)
    if T.ndim == 2 and T.shape[1] == 12:
        T = T.reshape(-1, 3, 4)
    if T.ndim != 3 or tuple(T.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"transforms (P, 12), (P, 3, 4) or (P, 4, 4) expected, got {T.shape}")
    if T.shape[1] == 3:
        T = np.concatenate([T, np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (len(T), 1, 4))], axis=1)
    return T


def _check_poses(poses) -> np.ndarray:
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f"poses (N, 4, 4) expected, got {poses.shape}")
    return poses


def rotation_angle_deg(R) -> float:
    """The angle of a 3 x 3 rotation in degrees: arccos((trace - 1) / 2), the argument clipped to [-1, 1]."""
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(R, dtype=np.float64)) - 1.0) / 2.0, -1.0, 1.0))))


def relative_pose_errors(T_est, poses, pairs) -> dict:
    """Per pair (a, b) of `pairs`: E = inv(T_gt) @ T_est with T_gt = relative_transform(poses[a], poses[b]).
    T_est: (P, 12), (P, 3, 4) or (P, 4, 4), camera a -> camera b.  Returns {'translation': (P,) metres, 'rotation': (P,) degrees}."""
    T_est, poses = _as44(T_est), _check_poses(poses)
    if len(T_est) != len(pairs):
        raise ValueError(f"{len(T_est)} transforms for {len(pairs)} pairs")
    if any(not (0 <= a < len(poses) and 0 <= b < len(poses)) for a, b in pairs):
        raise ValueError(f"{len(poses)} poses do not cover the pairs")
    E = [np.linalg.inv(relative_transform(poses[a], poses[b])) @ T for (a, b), T in zip(pairs, T_est)]
    return {"translation": np.array([np.linalg.norm(e[:3, 3]) for e in E], dtype=np.float64),
            "rotation": np.array([rotation_angle_deg(e[:3, :3]) for e in E], dtype=np.float64)}


def _statistics(v, extremes: bool = False) -> dict:
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 1 or v.size == 0:
        raise ValueError("one error per pair (or pose) expected, for at least one")
    out = {"rmse": float(np.sqrt(np.mean(v * v))), "mean": float(np.mean(v)), "median": float(np.median(v)), "std": float(np.std(v))}
    if extremes:
        out.update(min=float(np.min(v)), max=float(np.max(v)))
    return out


def rpe_summary(errors: dict) -> dict:
    """relative_pose_errors' dictionary -> the reference's compute_rpe dictionary: {'translation': rmse / mean / median / std in
    metres, 'rotation': the same in degrees}."""
    if not isinstance(errors, dict) or any(key not in errors for key in ("translation", "rotation")):
        raise ValueError("the dictionary relative_pose_errors returned expected")
    return {"translation": _statistics(errors["translation"]), "rotation": _statistics(errors["rotation"])}


def align_rigid(src, dst) -> tuple:
    """(R, t) of the rigid motion WITHOUT scale that takes the points src (N, 3) closest to dst (N, 3) in the least-squares sense
    (Kabsch, with the reflection guard): dst ~ R src + t."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if src.shape != dst.shape or src.ndim != 2 or src.shape[1] != 3 or len(src) == 0:
        raise ValueError(f"two (N, 3) point sets expected, got {src.shape} and {dst.shape}")
    cs, cd = src.mean(axis=0), dst.mean(axis=0)
    U, _, Vt = np.linalg.svd((dst - cd).T @ (src - cs))
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ S @ Vt
    return R, cd - R @ cs


def ate_summary(trajectory, poses) -> dict:
    """The reference's compute_ate dictionary (rmse / mean / median / std / min / max, metres) for an estimated trajectory (N, 4, 4)
    against the true poses (N, 4, 4), both camera-to-world: the positions are aligned rigidly without scale, then compared."""
    est, gt = _as44(trajectory), _check_poses(poses)
    if len(est) != len(gt):
        raise ValueError(f"{len(est)} estimated poses against {len(gt)} true ones")
    R, t = align_rigid(est[:, :3, 3], gt[:, :3, 3])
    return _statistics(np.linalg.norm(est[:, :3, 3] @ R.T + t - gt[:, :3, 3], axis=1), extremes=True)


def chain(T, start=None) -> np.ndarray:
    """(P + 1, 4, 4) camera-to-world poses from the P transforms camera i -> camera i + 1 of consecutive pairs:
    pose_0 = start (the identity if None), pose_{i+1} = pose_i @ inv(T_i)."""
    T = _as44(T)
    pose = np.eye(4) if start is None else np.asarray(start, dtype=np.float64)
    if pose.shape != (4, 4):
        raise ValueError(f"start must be a 4 x 4 pose, got {pose.shape}")
    out = [pose]
    for Ti in T:
        out.append(out[-1] @ np.linalg.inv(Ti))
    return np.stack(out)


def consecutive_pairs(n_frames: int, spacing: int = 1, num_pairs=None) -> list:
    """The pairs (i, i + spacing), i = 0 .. n_frames - spacing - 1, the first num_pairs of them if given."""
    for name, v, lo in (("n_frames", n_frames, 0), ("spacing", spacing, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    if num_pairs is not None and (isinstance(num_pairs, bool) or not isinstance(num_pairs, (int, np.integer)) or num_pairs < 1):
        raise ValueError(f"num_pairs must be None or an integer >= 1, got {num_pairs!r}")
    p = max(0, int(n_frames) - int(spacing))
    return [(i, i + int(spacing)) for i in range(p if num_pairs is None else min(p, int(num_pairs)))]


def _check_arguments(depth, kp_depth, camera, poses, threshold, hypotheses, seed, n_frames, keypoints_shape=None):
    """Everything odometry / odometry_result can refuse before any device work -> the Camera to use."""
    lib.check_threshold(threshold)
    lib.check_hypotheses(hypotheses)
    lib.check_seed(seed)
    camera = Camera() if camera is None else camera
    lib.check_camera(camera)
    if poses is not None and len(_check_poses(poses)) < n_frames:
        raise ValueError(f"{len(poses)} poses, the pairs name {n_frames} frames")
    if kp_depth is not None:
        if depth is not None:
            raise ValueError("depth= and kp_depth= are two forms of one argument: pass one")
        if not isinstance(kp_depth, torch.Tensor) or kp_depth.dtype != torch.int32 or \
                (keypoints_shape is not None and tuple(kp_depth.shape) != tuple(keypoints_shape[:2])):
            raise ValueError("kp_depth must be the int32 tensor gather_keypoint_depth returned for these keypoints")
        return camera
    ok = (isinstance(depth, np.ndarray) and depth.dtype == np.uint16) or (isinstance(depth, torch.Tensor) and depth.dtype == torch.uint16)
    if not ok or depth.ndim != 3:
        raise ValueError("odometry needs depth: (N, h, w) uint16 raw depth images, numpy or tensor")
    if int(depth.shape[0]) < n_frames:
        raise ValueError(f"depth holds {int(depth.shape[0])} frames, the pairs name {n_frames}")
    check_depth_size(depth.shape[2], depth.shape[1], camera)
    return camera


def info_matrix(info) -> np.ndarray:
    """(P, 6, 6) symmetric information matrices from refine_poses' info (P, 21), the upper triangles row-major."""
    info = np.asarray(info.detach().cpu().numpy() if isinstance(info, torch.Tensor) else info, dtype=np.float64)
    if info.ndim != 2 or info.shape[1] != 21:
        raise ValueError(f"info (P, 21) expected, got {info.shape}")
    iu = np.triu_indices(6)
    H = np.zeros((len(info), 6, 6))
    H[:, iu[0], iu[1]] = info
    H[:, iu[1], iu[0]] = info
    return H


def _summaries(out: dict, T, poses, pairs, spacing) -> None:
    """The figures built from the transforms T: inlier_ratio, the chained trajectory, RPE and ATE, written into out."""
    out["inlier_ratio"] = np.where(out["match_count"] > 0, out["inlier_count"] / np.maximum(out["match_count"], 1), 0.0)
    if spacing == 1:
        out["trajectory"] = chain(T, None if poses is None else np.asarray(poses, dtype=np.float64)[pairs[0][0]])
    if poses is not None:
        out["rpe"] = rpe_summary(relative_pose_errors(T, poses, pairs))
        out["ate"] = ate_summary(out["trajectory"], np.asarray(poses, dtype=np.float64)[:len(pairs) + 1]) if spacing == 1 else None


_REFINE_INT = ("status", "iterations", "selected_count", "inlier_count")
_REFINE_REAL = ("cost_in", "cost", "rms")


def _check_refine(refine, threshold, huber, iterations) -> None:
    """What the refinement's arguments can be refused for, before any device work."""
    if not isinstance(refine, bool):
        raise ValueError(f"refine must be a bool, got {refine!r}")
    if refine:
        lib.check_huber(float(threshold) / 3.0 if huber is None else huber)
        lib.check_iterations(iterations)


def _check_weights(pipe, weights, refine) -> None:
    """What weights= can be refused for, before any device work: it is a PoseWeights, it needs the refinement it weights and a
    pipeline that extracts the confidence it is made of."""
    if weights is None:
        return
    if not isinstance(weights, PoseWeights):
        raise ValueError(f"weights must be None or a PoseWeights, got {type(weights).__name__}")
    if not refine:
        raise ValueError("weights= weights the refinement: it needs refine=True")
    if not getattr(pipe.cfg, "confidence", False):
        raise ValueError("weights= is made of the keypoint confidence: the pipeline needs ExtractorConfig(confidence=True)")


def _launch(pipe, keypoints_pixel, kp_depth, pairs, matches, camera, threshold, hypotheses, seed, refine, huber, iterations, weight=None):
    """The RANSAC launch on the listed pairs (and, with refine, the refinement launch behind it) -> ((P, 18) float64 device tensor -
    (P, 58) with refine, (P, 59) with a weight tensor (P, n1): weight_sum last -, refine_poses' dictionary or None).  No host read."""
    return _launch_lists(pipe, keypoints_pixel, kp_depth, [a for a, _ in pairs], [b for _, b in pairs], matches, camera, threshold, hypotheses,
                         seed, refine, huber, iterations, weight)


def _launch_lists(pipe, keypoints_pixel, kp_depth, first, second, matches, camera, threshold, hypotheses, seed, refine, huber, iterations,
                  weight=None):
    """_launch on pair lists as match_pairs takes them: host sequences, or int32 device tensors that nothing here reads."""
    est = pipe.estimate_poses(keypoints_pixel, kp_depth, first, second, matches, camera, threshold, hypotheses, seed)
    cols = [est["T"]] + [est[key].to(torch.float64)[:, None] for key in _INT_KEYS] + \
           [matches["match_count"].to(torch.float64)[:, None], est["rms"][:, None]]
    ref = None
    if refine:
        ref = pipe.refine_poses(keypoints_pixel, kp_depth, first, second, matches, camera, est, threshold, huber, iterations, weights=weight)
        cols += [ref["T"]] + [ref[key].to(torch.float64)[:, None] for key in _REFINE_INT] + [ref[key][:, None] for key in _REFINE_REAL] + \
                [ref["info"]]
        if weight is not None:
            cols.append(ref["weight_sum"][:, None])         # the one column a weighted row grows by
    return torch.cat(cols, dim=1), ref                      # integers up to 4096: exact in float64


def _unpack(host, pairs, poses, spacing, refine) -> dict:
    """The host-side figures from the rows _launch packed, read back."""
    T = _as44(host[:, :12])
    out = {"pairs": list(pairs), "T": T}
    out.update({key: host[:, 12 + i].astype(np.int64) for i, key in enumerate(_INT_KEYS)})
    out["match_count"] = host[:, 16].astype(np.int64)
    out["rms"] = host[:, 17].copy()
    if not refine:
        _summaries(out, T, poses, pairs, spacing)
        return out
    ransac = {key: out[key] for key in ("T", "inlier_count", "rms", "match_count")}
    _summaries(ransac, T, poses, pairs, spacing)
    del ransac["match_count"]
    r = host[:, 18:]
    out["T"] = _as44(r[:, :12])
    got = {key: r[:, 12 + i].astype(np.int64) for i, key in enumerate(_REFINE_INT)}
    out["inlier_count"] = got["inlier_count"]
    out["rms"] = r[:, 18].copy()
    _summaries(out, out["T"], poses, pairs, spacing)
    out["ransac"] = ransac
    out["refine"] = {"status": got["status"], "iterations": got["iterations"], "selected_count": got["selected_count"],
                     "cost_in": r[:, 16].copy(), "cost": r[:, 17].copy(), "info": info_matrix(r[:, 19:40])}
    if r.shape[1] > 40:                                      # a weighted row: weight_sum behind info
        out["refine"]["weight_sum"] = r[:, 40].copy()
    return out


def _estimate(pipe, keypoints_pixel, kp_depth, pairs, matches, camera, poses, spacing, threshold, hypotheses, seed, refine=False,
              huber=None, iterations=5, weight=None) -> dict:
    """The RANSAC launch on the listed pairs (and, with refine, the refinement launch behind it), ONE host read-back of (P, 18)
    float64 ((P, 58) with refine, (P, 59) weighted), the host-side figures."""
    packed, _ = _launch(pipe, keypoints_pixel, kp_depth, pairs, matches, camera, threshold, hypotheses, seed, refine, huber, iterations,
                        weight)
    return _unpack(packed.cpu().numpy(), pairs, poses, spacing, refine)


def odometry(pipe, images_u8=None, depth=None, camera=None, poses=None, spacing: int = 1, num_pairs=None, rule=None,
             threshold: float = 3.0, hypotheses: int = 256, seed: int = 0, tokens=None, refine: bool = False, huber=None,
             iterations: int = 5, *, subcell=None, weights=None) -> dict:
    """The relative pose of every pair (i, i + spacing) of a sequence, from its own features: the frames images_u8 (N, H, W, 3)
    uint8 (a pipeline built with vit=) or their ViT tokens (tokens=), their raw depth images depth (N, h, w) uint16 (numpy or
    tensor) and camera (an evaluation.Camera; the default one if None).  The frames are extracted once, the depth under every
    keypoint gathered (evaluation.gather_keypoint_depth), the pairs matched under `rule` (MatchRule.mnn_ratio(0.9) if None) and
    the poses estimated (SequencePipeline.estimate_poses: threshold in keypoint units, hypotheses, seed); ONE read-back.
    Returns, per pair: 'pairs', 'T' (P, 4, 4) camera i -> camera i + spacing, 'inlier_count', 'usable_count', 'best_hypothesis',
    'refit_kept', 'match_count', 'rms', 'inlier_ratio' = inlier_count / match_count; for spacing 1 'trajectory' (P + 1, 4, 4), the
    chained camera-to-world poses starting at the identity (at poses[0] with poses); with poses (N, 4, 4) also 'rpe'
    (rpe_summary) and 'ate' (ate_summary of the trajectory; None for another spacing).
    refine=True puts SequencePipeline.refine_poses behind the RANSAC launch (huber: threshold / 3 if None; iterations Gauss-Newton
    steps at most), still with ONE read-back: 'T', 'inlier_count', 'rms', 'inlier_ratio', 'trajectory', 'rpe' and 'ate' are then the
    refined poses' (a pair whose refinement is not kept or not attempted keeps RANSAC's pose), 'ransac' holds the unrefined 'T',
    'inlier_count', 'rms' and the summaries built from them, and 'refine' holds 'status', 'iterations', 'selected_count', 'cost_in',
    'cost' and 'info' (P, 6, 6), the information matrix of every refined pose.  With refine=False nothing changes.
    subcell: on a pipeline with ExtractorConfig(subcell=True) the depth lookups, RANSAC and the refinement read the refined
    keypoints (evaluation.geometry_bank); subcell=False forces the cell centres.  The match lists are the same either way.
    weights: with refine=True on a pipeline with ExtractorConfig(confidence=True), a PoseWeights: one SequencePipeline.match_weights
    launch makes every match's weight of its two keypoints' confidences and the weighted refinement runs
    (include/sslam_weight.h); 'refine' then also holds 'weight_sum', and 'info' is the weighted information matrix.  Still ONE
    read-back.  With weights=None nothing changes."""
    check_subcell(subcell)
    _check_weights(pipe, weights, refine)
    src = tokens if tokens is not None else images_u8
    if src is None:
        raise ValueError("images_u8 or tokens= required")
    pairs = consecutive_pairs(int(src.shape[0]), spacing, num_pairs)
    if not pairs:
        raise ValueError(f"{int(src.shape[0])} frames hold no pair at spacing {spacing}")
    n = pairs[-1][1] + 1
    camera = _check_arguments(depth, None, camera, poses, threshold, hypotheses, seed, n)
    _check_refine(refine, threshold, huber, iterations)
    rule = MatchRule.mnn_ratio(0.9) if rule is None else rule
    ex = pipe.extract(pipe.tokens_from_images(images_u8[:n]) if tokens is None else tokens[:n], None)
    kp = geometry_bank(ex, subcell)
    kp_depth = gather_keypoint_depth(pipe, depth, kp, n)
    matches = pipe.match_pairs(ex["descriptors"], ex["scores"], first=[a for a, _ in pairs], second=[b for _, b in pairs], rule=rule)
    weight = None if weights is None else pipe.match_weights(ex["confidence"], [a for a, _ in pairs], [b for _, b in pairs], matches, weights)
    return _estimate(pipe, kp, kp_depth, pairs, matches, camera, poses, spacing, threshold, hypotheses, seed, refine,
                     huber, iterations, weight)


def odometry_result(pipe, result: dict, depth=None, camera=None, poses=None, spacing: int = 1, num_pairs=None,
                    threshold: float = 3.0, hypotheses: int = 256, seed: int = 0, *, kp_depth=None, refine: bool = False, huber=None,
                    iterations: int = 5, subcell=None) -> dict:
    """odometry() for a StreamingSequence.result() / run_frames / run_directory result: the keypoints and the match lists of every
    pair (i, i + spacing) are already in device memory, under whichever rule the sequence was run with, so nothing is extracted
    or matched again.  depth=: the raw depth images of the result's frames; kp_depth=: instead, the (N, K) int32 bank
    gather_keypoint_depth returned for result["frames"]["keypoints_pixel"], as evaluation.evaluate_result takes it.
    refine, huber, iterations, subcell: as odometry() takes them; a kp_depth= bank must have been gathered under the same bank
    (evaluation.geometry_bank(result["frames"], subcell))."""
    if not isinstance(result, dict) or "frames" not in result or "keypoints_pixel" not in result["frames"]:
        raise ValueError("a StreamingSequence / run_directory result expected")
    kp = geometry_bank(result["frames"], subcell)
    pairs = consecutive_pairs(int(kp.shape[0]), spacing, num_pairs)
    if not pairs or spacing not in result:
        raise ValueError(f"the result holds no pair at spacing {spacing}")
    n = pairs[-1][1] + 1
    camera = _check_arguments(depth, kp_depth, camera, poses, threshold, hypotheses, seed, n, kp.shape)
    _check_refine(refine, threshold, huber, iterations)
    mm = result[spacing]
    matches = {key: mm[key][:len(pairs)] for key in ("matches", "match_count")}
    if kp_depth is None:
        kp_depth = gather_keypoint_depth(pipe, depth, kp, n)
    return _estimate(pipe, kp, kp_depth, pairs, matches, camera, poses, spacing, threshold, hypotheses, seed, refine, huber, iterations)


# ------------------------------------------------------------------------------------------------ the pose graph over all spacings
GRAPH_SPACINGS = (1, 5, 10, 15, 20)          # the reference's own set
_GRAPH_INT = ("status", "iterations", "used_edges", "skipped_edges", "failed_row")


def _check_graph(spacings, n_frames, num_pairs, band, huber_chi, damping, graph_iterations) -> tuple:
    """What the graph's arguments can be refused for, before any device work -> (the spacings that hold a pair, their pair lists,
    the number of frames they name, the band)."""
    spacings = tuple(spacings)
    if not spacings or len(set(spacings)) != len(spacings) or 1 not in spacings:
        raise ValueError(f"spacings must be distinct and hold 1 (the chain is the initial guess), got {spacings!r}")
    lists = {s: consecutive_pairs(n_frames, s, num_pairs) for s in spacings}
    lists = {s: p for s, p in lists.items() if p}
    if 1 not in lists:
        raise ValueError(f"{n_frames} frames hold no pair at spacing 1")
    n = lists[1][-1][1] + 1                                  # the frames the chain reaches: the graph's nodes
    lists = {s: [(a, b) for a, b in p if b < n] for s, p in lists.items()}
    lists = {s: p for s, p in lists.items() if p}
    band = lib.check_band(max(lists) if band is None else band)
    lib.check_positive("huber_chi", huber_chi), lib.check_damping(damping), lib.check_graph_iterations(graph_iterations)
    if n > lib.GRAPH_MAX_NODES:
        raise lib.SslamHipError(f"odometry_graph: {n} frames, the pose graph takes {lib.GRAPH_MAX_NODES}")
    return tuple(lists), lists, n, band


def _sequence_preamble(pipe, images_u8, tokens, depth, camera, poses, spacings, num_pairs, rule, threshold, hypotheses, seed, huber,
                       iterations, subcell, band, huber_chi, damping, graph_iterations, more=lambda: None) -> tuple:
    """What odometry_graph and odometry_loop_graph do alike before they match: every argument judged (more(): the caller's own,
    where they always stood), the frames extracted once, the geometry bank, the keypoints' depth, the spacings' pair list."""
    check_subcell(subcell)
    src = tokens if tokens is not None else images_u8
    if src is None:
        raise ValueError("images_u8 or tokens= required")
    _, lists, n, band = _check_graph(spacings, int(src.shape[0]), num_pairs, band, huber_chi, damping, graph_iterations)
    opt = more()
    camera = _check_arguments(depth, None, camera, poses, threshold, hypotheses, seed, n)
    _check_refine(True, threshold, huber, iterations)
    rule = MatchRule.mnn_ratio(0.9) if rule is None else rule
    ex = pipe.extract(pipe.tokens_from_images(images_u8[:n]) if tokens is None else tokens[:n], None)
    kp = geometry_bank(ex, subcell)
    return lists, n, band, opt, camera, rule, ex, kp, gather_keypoint_depth(pipe, depth, kp, n), [pr for s in lists for pr in lists[s]]


def _result_preamble(result, keys, depth, kp_depth, camera, poses, spacings, num_pairs, threshold, hypotheses, seed, huber, iterations,
                     subcell, band, huber_chi, damping, graph_iterations, more=lambda: None) -> tuple:
    """What odometry_result_graph and odometry_result_loop_graph do alike: the result must hold `keys` per frame; the geometry
    bank, the result's spacings if none are given, every argument judged (more(): the caller's own)."""
    if not isinstance(result, dict) or "frames" not in result or any(key not in result["frames"] for key in keys):
        raise ValueError("a StreamingSequence / run_directory result expected")
    kp = geometry_bank(result["frames"], subcell)
    if spacings is None:
        spacings = tuple(sorted(k for k in result if isinstance(k, (int, np.integer)) and not isinstance(k, bool)))
    if any(s not in result for s in spacings):
        raise ValueError(f"the result holds no pairs at every spacing of {tuple(spacings)!r}")
    _, lists, n, band = _check_graph(spacings, int(kp.shape[0]), num_pairs, band, huber_chi, damping, graph_iterations)
    opt = more()
    camera = _check_arguments(depth, kp_depth, camera, poses, threshold, hypotheses, seed, n, kp.shape)
    _check_refine(True, threshold, huber, iterations)
    return kp, lists, n, band, opt, camera


def _graph_device(pipe, ref, pairs, lists, n, poses, band, huber_chi, damping, graph_iterations) -> dict:
    """The chain of the refined spacing-1 poses and the banded graph over the refined pairs `ref` (refine_poses' dictionary, one row
    per pair of `pairs`) -> optimize_pose_graph's device tensors.  No host read."""
    start = None
    if poses is not None:                                    # the chain of odometry() starts at poses[0]: so does this one
        c0 = np.linalg.inv(np.asarray(poses, dtype=np.float64)[0])[:3].reshape(1, 12)
        start = torch.from_numpy(np.ascontiguousarray(c0)).to(ref["T"].device)
    n1 = len(lists[1])
    C_init = lib.chain_poses(ref["T"][:n1].contiguous(), n, start=start)[0]
    return pipe.optimize_pose_graph([a for a, _ in pairs], [b for _, b in pairs], ref, ref, n, C_init=C_init, band=band, huber_chi=huber_chi,
                                    damping=damping, iterations=graph_iterations)


def _graph_flat(g) -> list:
    """A graph's device tensors as float64 pieces of one read-back, in _graph_host's order."""
    return [g["C"].reshape(-1)] + [g[key].to(torch.float64).reshape(1) for key in _GRAPH_INT] + \
           [g["cost_in"].reshape(1), g["cost"].reshape(1), g["edge_chi2"]]


def _graph_words(n: int, n_pairs: int) -> int:
    """How many numbers _graph_flat lays out for a graph of n nodes over n_pairs listed pairs: C, the five integers, the two costs,
    edge_chi2.  Whatever follows a graph in a read-back starts there: the one place that says so."""
    return 12 * n + len(_GRAPH_INT) + 2 + n_pairs


def _graph_host(rest, n, pairs, poses) -> dict:
    """The host-side figures of a graph from the _graph_words(n, len(pairs)) numbers _graph_flat laid out."""
    C = rest[:12 * n].reshape(n, 3, 4)
    C44 = np.concatenate([C, np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1, 4))], axis=1)
    graph = {"trajectory": np.stack([np.linalg.inv(c) for c in C44]), "pairs": pairs}
    graph.update({key: int(rest[12 * n + i]) for i, key in enumerate(_GRAPH_INT)})
    graph["cost_in"], graph["cost"] = float(rest[12 * n + 5]), float(rest[12 * n + 6])
    graph["edge_chi2"] = rest[12 * n + 7:_graph_words(n, len(pairs))].copy()
    if poses is not None:
        graph["ate"] = ate_summary(graph["trajectory"], np.asarray(poses, dtype=np.float64)[:n])
    return graph


def _spacings_and_graph(host, rest, lists, pairs, n, poses) -> dict:
    """The read-back split: `host`, a row per pair, into every spacing's dictionary; `rest` (_graph_flat's numbers first) into 'graph'."""
    out, at = {}, 0
    for s in lists:
        out[s] = _unpack(host[at:at + len(lists[s])], lists[s], poses, s, True)
        at += len(lists[s])
    graph = _graph_host(rest, n, pairs, poses)
    if poses is not None:
        graph["ate_chain"] = out[1]["ate"]
    out["graph"] = graph
    return out


def check_tracks(tracks):
    """tracks= of odometry_graph: None (no tracks: nothing is launched), True (the defaults) or a dictionary of some of threshold
    (keypoint units, 3.0) and min_obs (>= 2, 2) -> None or the dictionary with both; anything else ValueError, before any device work."""
    if tracks is None:
        return None
    if tracks is True:
        tracks = {}
    if not isinstance(tracks, dict) or any(key not in TRACK_DEFAULTS for key in tracks):
        raise ValueError(f"tracks must be None, True or a dictionary of some of {', '.join(TRACK_DEFAULTS)}, got {tracks!r}")
    opt = {**TRACK_DEFAULTS, **tracks}
    return dict(threshold=lib.check_threshold(opt["threshold"]), min_obs=lib.check_min_obs(opt["min_obs"]))


TRACK_DEFAULTS = dict(threshold=3.0, min_obs=2)
_TRACK_ROWS = ("length", "status", "n_kept", "rms")


def _tracks_device(pipe, kp, kp_depth, lists, matches, ref, C, n, camera, opt, confidence) -> list:
    """Links from the spacing-1 rows masked by the refinement's inlier_of_slot, their ids, the landmarks under the graph's C ->
    float64 pieces for the one read-back, in _tracks_host's order.  No host read."""
    at = sum(len(lists[s]) for s in list(lists)[:list(lists).index(1)])
    rows = slice(at, at + len(lists[1]))
    links = pipe.link_matches([a for a, _ in lists[1]], [b for _, b in lists[1]], {key: matches[key][rows] for key in ("matches", "match_count")},
                              mask=ref["inlier_of_slot"][rows], n_frames=n, k=int(kp.shape[1]))
    tr = pipe.track_ids(links)
    lm = pipe.landmarks(kp[:n], kp_depth[:n], C.reshape(n, 12), tr, camera, opt["threshold"], opt["min_obs"],
                        weights=None if confidence is None else confidence[:n])
    f64 = lambda t: t.to(torch.float64).reshape(-1)
    return [f64(tr["n_tracks"]), f64(tr["track_id"]), f64(tr["length"]), f64(lm["status"]), f64(lm["n_kept"]), lm["rms"], lm["xyz"].reshape(-1)]


def _tracks_host(rest, n, k) -> dict:
    """The host-side figures of the tracks from the 1 + 8 n k numbers _tracks_device laid out."""
    from .track_numpy import length_statistics
    N = n * k
    nt = int(rest[0])
    track_id = rest[1:1 + N].astype(np.int32).reshape(n, k)
    cols = {key: rest[1 + (i + 1) * N:1 + (i + 2) * N][:nt] for i, key in enumerate(_TRACK_ROWS)}
    out = {"n_tracks": nt, "length": length_statistics(cols["length"].astype(np.int64), [nt]), "track_id": track_id,
           "landmarks": rest[1 + 5 * N:1 + 8 * N].reshape(N, 3)[:nt].copy(), "status": cols["status"].astype(np.int32),
           "n_kept": cols["n_kept"].astype(np.int32), "rms": cols["rms"].copy()}
    del out["length"]["n_tracks"]
    return out


def _graph(pipe, kp, kp_depth, lists, matches, n, camera, poses, threshold, hypotheses, seed, huber, iterations, band, huber_chi, damping,
           graph_iterations, weight=None, tracks=None, confidence=None) -> dict:
    """One RANSAC and one refinement launch over the concatenated pair lists, the chain, the graph, ONE read-back.  weight: the
    (P, n1) weights of the weighted refinement, whose info the graph then reads as it reads the unweighted one.  tracks:
    check_tracks' dictionary - the links, ids and landmarks (weighted by `confidence` where given) join the same read-back."""
    pairs = [pr for s in lists for pr in lists[s]]
    packed, ref = _launch(pipe, kp, kp_depth, pairs, matches, camera, threshold, hypotheses, seed, True, huber, iterations, weight)
    g = _graph_device(pipe, ref, pairs, lists, n, poses, band, huber_chi, damping, graph_iterations)
    more = [] if tracks is None else _tracks_device(pipe, kp, kp_depth, lists, matches, ref, g["C"], n, camera, tracks, confidence)
    flat = torch.cat([packed.reshape(-1)] + _graph_flat(g) + more).cpu().numpy()          # the ONE read-back
    P, w = len(pairs), int(packed.shape[1])
    host, rest = flat[:P * w].reshape(P, w), flat[P * w:]
    out = _spacings_and_graph(host, rest, lists, pairs, n, poses)
    if tracks is not None:
        out["tracks"] = _tracks_host(rest[_graph_words(n, P):], n, int(kp.shape[1]))
    return out


def odometry_graph(pipe, images_u8=None, depth=None, camera=None, poses=None, spacings=GRAPH_SPACINGS, num_pairs=None, rule=None,
                   threshold: float = 3.0, hypotheses: int = 256, seed: int = 0, tokens=None, huber=None, iterations: int = 5, *,
                   subcell=None, band=None, huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 8, weights=None,
                   tracks=None) -> dict:
    """odometry(refine=True) at every spacing of `spacings` at once, and the pose graph over all of their edges
    (SequencePipeline.optimize_pose_graph; csrc_graph/pose_graph.hip): the frames are extracted once, the pairs of all spacings
    matched in one match_pairs call, ONE RANSAC and ONE refinement launch run over the concatenated pair list, the refined
    spacing-1 poses are chained on the device (the initial guess), the graph optimised - every refined pose an edge weighted by its
    own information matrix, a pair whose refinement was not attempted left out - and everything read back ONCE.
    images_u8 .. iterations, subcell: as odometry() takes them (num_pairs: per spacing; the graph's nodes are the frames the
    spacing-1 pairs reach, and pairs that leave them are dropped).  band: the most b - a of a used edge, the largest spacing if
    None; huber_chi, damping, graph_iterations: include/sslam_graph.h.
    Returns {spacing: what odometry(spacing=spacing, refine=True) returns, ..., 'graph': {'trajectory' (N, 4, 4) camera-to-world,
    'pairs', 'status', 'iterations', 'used_edges', 'skipped_edges', 'failed_row', 'cost_in', 'cost', 'edge_chi2' (one per listed
    pair); with poses also 'ate' (ate_summary of the graph's trajectory) and 'ate_chain' (that of the spacing-1 chain)}}.
    weights: as odometry() takes it - ONE match_weights launch over the concatenated pair list, the weighted refinement, every
    spacing's 'refine' with 'weight_sum'; the graph reads the weighted information matrices with no change of its own.
    tracks: None, True or a dictionary of some of threshold (keypoint units, 3.0) and min_obs (2) - feature tracks and the landmark
    map (include/sslam_track.h): the spacing-1 match lists, masked by the refinement's inlier_of_slot, become links
    (SequencePipeline.link_matches), the links tracks (track_ids), the tracks map points under the graph's poses (landmarks; with
    weights= given the keypoint confidences weight the observations), all added to the SAME single read-back.  'tracks' then holds
    'n_tracks', 'length' (mean, median, max, share_ge_2, histogram), 'landmarks' (n_tracks, 3) world points, 'status', 'n_kept',
    'rms' (n_tracks,) and 'track_id' (N, K).  With tracks=None the call returns and launches exactly what it did before.
    Nobody has measured this on real RGB-D data: no real sequence was at hand when this was written."""
    def more():
        _check_weights(pipe, weights, True)
        return check_tracks(tracks)
    lists, n, band, opt, camera, rule, ex, kp, kp_depth, pairs = _sequence_preamble(
        pipe, images_u8, tokens, depth, camera, poses, spacings, num_pairs, rule, threshold, hypotheses, seed, huber, iterations, subcell, band,
        huber_chi, damping, graph_iterations, more)
    matches = pipe.match_pairs(ex["descriptors"], ex["scores"], first=[a for a, _ in pairs], second=[b for _, b in pairs], rule=rule)
    weight = None if weights is None else pipe.match_weights(ex["confidence"], [a for a, _ in pairs], [b for _, b in pairs], matches, weights)
    return _graph(pipe, kp, kp_depth, lists, matches, n, camera, poses, threshold, hypotheses, seed, huber, iterations, band, huber_chi,
                  damping, graph_iterations, weight, opt, None if weights is None or opt is None else ex["confidence"])


def odometry_result_graph(pipe, result: dict, depth=None, camera=None, poses=None, spacings=None, num_pairs=None, threshold: float = 3.0,
                          hypotheses: int = 256, seed: int = 0, *, kp_depth=None, huber=None, iterations: int = 5, subcell=None, band=None,
                          huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 8) -> dict:
    """odometry_graph() for a StreamingSequence.result() / run_frames / run_directory result: nothing is extracted or matched again.
    spacings: those of the result if None.  depth= / kp_depth=, and everything else: as odometry_result() and odometry_graph()
    take them."""
    kp, lists, n, band, _, camera = _result_preamble(result, ("keypoints_pixel",), depth, kp_depth, camera, poses, spacings, num_pairs, threshold,
                                                     hypotheses, seed, huber, iterations, subcell, band, huber_chi, damping, graph_iterations)
    matches = {key: torch.cat([result[s][key][:len(lists[s])] for s in lists]) for key in ("matches", "match_count")}
    if kp_depth is None:
        kp_depth = gather_keypoint_depth(pipe, depth, kp, n)
    return _graph(pipe, kp, kp_depth, lists, matches, n, camera, poses, threshold, hypotheses, seed, huber, iterations, band, huber_chi,
                  damping, graph_iterations)


# ------------------------------------------------------------------------------------------------------------------ loop closures
LOOP_DEFAULTS = dict(min_gap=30, min_sim=0.3, per_frame=2, suppress=5, min_inliers=12)
_LOOP_INT = ("status", "inlier_count")


def check_loops(loops, cg_iterations=512, cg_tol=1e-3, prune_chi=None) -> dict:
    """What the loop-closure arguments can be refused for, before any device work -> LOOP_DEFAULTS with `loops` laid over it.
    loops: None or True (the defaults) or a dictionary of some of min_gap, min_sim, per_frame, suppress (SequencePipeline.
    find_loop_candidates) and min_inliers, the fewest inliers of its refined pose that make a candidate an edge."""
    if loops is None or loops is True:
        loops = {}
    if not isinstance(loops, dict) or any(key not in LOOP_DEFAULTS for key in loops):
        raise ValueError(f"loops must be True or a dictionary of {', '.join(LOOP_DEFAULTS)}, got {loops!r}")
    opt = dict(LOOP_DEFAULTS, **loops)
    lib.check_loop_arguments(opt["min_gap"], opt["min_sim"], opt["per_frame"], opt["suppress"])
    lib.check_int("min_inliers", opt["min_inliers"], 0)
    lib.check_cg_iterations(cg_iterations), lib.check_cg_tol(cg_tol)
    if prune_chi is not None:
        lib.check_positive("prune_chi", prune_chi)
    return opt


def _sparse_flat(r) -> list:
    return _graph_flat(r) + [r["cg_steps"].to(torch.float64)]


def _sparse_host(rest, n, pairs, poses) -> dict:
    graph = _graph_host(rest, n, pairs, poses)
    at = _graph_words(n, len(pairs))
    graph["cg_steps"] = rest[at:at + lib.SPARSE_MAX_ITER].astype(np.int64)
    return graph


def _loop_graph(pipe, kp, kp_depth, lists, matches, cand, n, camera, poses, threshold, hypotheses, seed, huber, iterations, band, huber_chi,
                damping, graph_iterations, opt, cg_iterations, cg_tol, prune_chi) -> dict:
    """One RANSAC and one refinement launch over the spacings' pairs followed by the candidate slots, the chain and the banded graph
    over the former, the sparse graph over all of them from the banded graph's poses, ONE read-back."""
    pairs = [pr for s in lists for pr in lists[s]]
    P, L, dev = len(pairs), int(cand["first"].shape[0]), kp.device
    of = torch.tensor([a for a, _ in pairs], dtype=torch.int32, device=dev)
    first = torch.cat([of, cand["first"]])
    second = torch.cat([torch.tensor([b for _, b in pairs], dtype=torch.int32, device=dev), cand["second"]])
    packed, ref = _launch_lists(pipe, kp, kp_depth, first, second, matches, camera, threshold, hypotheses, seed, True, huber, iterations)
    g = _graph_device(pipe, {key: ref[key][:P] for key in ("T", "info", "status")}, pairs, lists, n, poses, band, huber_chi, damping,
                      graph_iterations)
    kept = (cand["first"] >= 0) & (ref["status"][P:] != lib.REFINE_NOT_ATTEMPTED) & (ref["inlier_count"][P:] >= int(opt["min_inliers"]))
    absent = torch.full_like(first, -1)
    gfirst = torch.cat([of, torch.where(kept, cand["first"], absent[P:])])
    sparse = lambda f: pipe.optimize_pose_graph_sparse(f, second, ref, ref, n, g["C"], huber_chi, damping, graph_iterations, cg_iterations, cg_tol)
    runs = [sparse(gfirst)]
    if prune_chi is not None:
        runs.append(sparse(torch.where(runs[0]["edge_chi2"] > float(prune_chi) * float(prune_chi), absent, gfirst)))
    pieces = [packed.reshape(-1)] + _graph_flat(g) + [x for r in runs for x in _sparse_flat(r)] + \
             [cand[key].to(torch.float64) for key in ("first", "second", "sim", "count")] + [kept.to(torch.float64)]
    flat = torch.cat(pieces).cpu().numpy()                  # the ONE read-back
    w = int(packed.shape[1])
    host, rest = flat[:(P + L) * w].reshape(P + L, w), flat[(P + L) * w:]
    out = _spacings_and_graph(host, rest, lists, pairs, n, poses)
    rest = rest[_graph_words(n, P):]
    tail = rest[len(runs) * (_graph_words(n, P + L) + lib.SPARSE_MAX_ITER):]
    lf, ls = tail[:L].astype(np.int32), tail[L:2 * L].astype(np.int32)
    rows = host[P:]
    r = rows[:, 18:]
    out["loops"] = {"first": lf, "second": ls, "sim": tail[2 * L:3 * L].astype(np.float32), "count": tail[3 * L:3 * L + n].astype(np.int32),
                    "kept": tail[3 * L + n:] != 0, "match_count": rows[:, 16].astype(np.int64), "T": _as44(r[:, :12]),
                    "status": r[:, 12].astype(np.int64), "inlier_count": r[:, 15].astype(np.int64), "info": info_matrix(r[:, 19:40])}
    all_pairs = pairs + [(int(a), int(b)) for a, b in zip(lf, ls)]
    names = ["loop_graph"] if prune_chi is None else ["loop_graph_unpruned", "loop_graph"]
    for name in names:
        out[name] = _sparse_host(rest, n, all_pairs, poses)
        rest = rest[_graph_words(n, P + L) + lib.SPARSE_MAX_ITER:]
    return out


def odometry_loop_graph(pipe, images_u8=None, depth=None, camera=None, poses=None, spacings=GRAPH_SPACINGS, num_pairs=None, rule=None,
                        threshold: float = 3.0, hypotheses: int = 256, seed: int = 0, tokens=None, huber=None, iterations: int = 5, *,
                        subcell=None, band=None, huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 8, loops=None,
                        cg_iterations: int = 512, cg_tol: float = 1e-3, prune_chi=None) -> dict:
    """odometry_graph() with loop closures: the frames are extracted once; SequencePipeline.find_loop_candidates proposes, for
    every frame, older frames whose place signature resembles its own (loops: check_loops); ONE match_pairs call matches the
    spacings' pairs followed by the candidate slots (an empty slot is an absent pair), ONE RANSAC and ONE refinement launch run over
    that list; the chain and the banded graph run over the spacings' pairs exactly as in odometry_graph; a candidate becomes an
    edge iff its refinement was attempted and its refined pose has at least min_inliers inliers - decided on the device -; the
    sparse graph (SequencePipeline.optimize_pose_graph_sparse; cg_iterations, cg_tol) runs over ALL edges from the banded graph's
    poses; ONE read-back.  prune_chi: when given, a second sparse launch from the same poses without the slots whose edge_chi2
    after the first exceeds prune_chi * prune_chi.
    Returns odometry_graph()'s dictionary - every spacing and 'graph' byte for byte - and 'loops': 'first', 'second' (-1: an empty
    slot), 'sim', 'count' as find_loop_candidates lays them out, 'kept' (the slots that became edges), and per slot 'match_count',
    'T', 'status', 'inlier_count', 'info' of its refined pose; 'loop_graph': 'trajectory', 'pairs' (the spacings' pairs, then the
    candidate slots), 'status', 'iterations', 'used_edges', 'skipped_edges', 'failed_row', 'cost_in', 'cost', 'edge_chi2' (one per
    pair of 'pairs'), 'cg_steps' (16,), with poses 'ate'; with prune_chi 'loop_graph' is the second launch's and
    'loop_graph_unpruned' the first's.  Nobody has measured this on real RGB-D data."""
    lists, n, band, opt, camera, rule, ex, kp, kp_depth, pairs = _sequence_preamble(
        pipe, images_u8, tokens, depth, camera, poses, spacings, num_pairs, rule, threshold, hypotheses, seed, huber, iterations, subcell, band,
        huber_chi, damping, graph_iterations, lambda: check_loops(loops, cg_iterations, cg_tol, prune_chi))
    cand = pipe.find_loop_candidates(ex["descriptors"], ex["scores"], opt["min_gap"], opt["min_sim"], opt["per_frame"], opt["suppress"])
    dev = kp.device
    first = torch.cat([torch.tensor([a for a, _ in pairs], dtype=torch.int32, device=dev), cand["first"]])
    second = torch.cat([torch.tensor([b for _, b in pairs], dtype=torch.int32, device=dev), cand["second"]])
    matches = pipe.match_pairs(ex["descriptors"], ex["scores"], first=first, second=second, rule=rule)
    return _loop_graph(pipe, kp, kp_depth, lists, matches, cand, n, camera, poses, threshold, hypotheses, seed, huber, iterations, band,
                       huber_chi, damping, graph_iterations, opt, cg_iterations, cg_tol, prune_chi)


def odometry_result_loop_graph(pipe, result: dict, depth=None, camera=None, poses=None, spacings=None, num_pairs=None, threshold: float = 3.0,
                               hypotheses: int = 256, seed: int = 0, *, kp_depth=None, huber=None, iterations: int = 5, subcell=None,
                               band=None, huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 8, loops=None,
                               cg_iterations: int = 512, cg_tol: float = 1e-3, prune_chi=None, rule=None) -> dict:
    """odometry_loop_graph() for a StreamingSequence.result() / run_frames / run_directory result: nothing is extracted again and the
    spacings' pairs keep the match lists the sequence was run with; only the candidate slots are matched, in one match_pairs call
    under `rule` (MatchRule.mnn_ratio(0.9) if None - give the rule the sequence was run with).  Everything else: as
    odometry_result_graph() and odometry_loop_graph() take it."""
    kp, lists, n, band, opt, camera = _result_preamble(
        result, ("keypoints_pixel", "descriptors", "scores"), depth, kp_depth, camera, poses, spacings, num_pairs, threshold, hypotheses, seed, huber,
        iterations, subcell, band, huber_chi, damping, graph_iterations, lambda: check_loops(loops, cg_iterations, cg_tol, prune_chi))
    rule = MatchRule.mnn_ratio(0.9) if rule is None else rule
    desc, scores = result["frames"]["descriptors"][:n], result["frames"]["scores"][:n]
    cand = pipe.find_loop_candidates(desc, scores, opt["min_gap"], opt["min_sim"], opt["per_frame"], opt["suppress"])
    far = pipe.match_pairs(desc, scores, first=cand["first"], second=cand["second"], rule=rule)
    matches = {key: torch.cat([result[s][key][:len(lists[s])] for s in lists] + [far[key]]) for key in ("matches", "match_count")}
    if kp_depth is None:
        kp_depth = gather_keypoint_depth(pipe, depth, kp, n)
    return _loop_graph(pipe, kp, kp_depth, lists, matches, cand, n, camera, poses, threshold, hypotheses, seed, huber, iterations, band,
                       huber_chi, damping, graph_iterations, opt, cg_iterations, cg_tol, prune_chi)
