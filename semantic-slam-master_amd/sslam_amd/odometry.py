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

from dataclasses import dataclass

import numpy as np
import torch

from . import lib
from .evaluation import Camera, check_depth_size, check_subcell, gather_keypoint_depth, geometry_bank, relative_transform
from .pipeline import GraphSettings, MatchRule, PoseSettings, _np
from .readback import Readback

_INT_KEYS = ("inlier_count", "usable_count", "best_hypothesis", "refit_kept")


def _as44(T) -> np.ndarray:
    """(P, 4, 4) float64 from (P, 12), (P, 3, 4) or (P, 4, 4)."""
    T = np.asarray(_np(T), dtype=np.float64)
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


def camera_to_world(C) -> np.ndarray:
    """(n, 4, 4) float64 camera-to-world poses - a trajectory as TUM's groundtruth.txt and ate_summary have it - from the
    world-to-camera rows (n, 12) or (n, 3, 4) a pose graph or the window writes: every matrix inverted on its own."""
    C = _as44(C)
    return np.stack([np.linalg.inv(c) for c in C]) if len(C) else np.zeros((0, 4, 4))


def consecutive_pairs(n_frames: int, spacing: int = 1, num_pairs=None) -> list:
    """The pairs (i, i + spacing), i = 0 .. n_frames - spacing - 1, the first num_pairs of them if given."""
    for name, v, lo in (("n_frames", n_frames, 0), ("spacing", spacing, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    if num_pairs is not None and (isinstance(num_pairs, bool) or not isinstance(num_pairs, (int, np.integer)) or num_pairs < 1):
        raise ValueError(f"num_pairs must be None or an integer >= 1, got {num_pairs!r}")
    p = max(0, int(n_frames) - int(spacing))
    return [(i, i + int(spacing)) for i in range(p if num_pairs is None else min(p, int(num_pairs)))]


def _check_arguments(depth, kp_depth, camera, poses, n_frames, keypoints_shape=None):
    """What odometry / odometry_result can refuse of the sequence's own data before any device work (their settings are judged where
    the PoseSettings is built) -> the Camera to use."""
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
    info = np.asarray(_np(info), dtype=np.float64)
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


def _launch(pipe, rb, keypoints_pixel, kp_depth, pairs, matches, camera, pose, weight=None):
    """_launch_lists on a host list of pairs."""
    return _launch_lists(pipe, rb, keypoints_pixel, kp_depth, [a for a, _ in pairs], [b for _, b in pairs], matches, camera, pose, weight)


def _launch_lists(pipe, rb, keypoints_pixel, kp_depth, first, second, matches, camera, pose, weight=None):
    """The RANSAC launch on the listed pairs and, with pose.refine, the refinement launch behind it (weighted by `weight` (P, n1) where
    given).  first / second as match_pairs takes them: host sequences, or int32 device tensors that nothing here reads.  What the host
    wants of both joins the read-back rb, a row per pair: 'ransac.<key>', 'match_count' and 'refine.<key>'.  No host read ->
    refine_poses' dictionary, or None."""
    est = pipe.estimate_poses(keypoints_pixel, kp_depth, first, second, matches, camera, pose.threshold, pose.hypotheses, pose.seed)
    rb.add("match_count", matches["match_count"], np.int64)
    for key in ("T", "rms"):
        rb.add("ransac." + key, est[key], np.float64)
    for key in _INT_KEYS:
        rb.add("ransac." + key, est[key], np.int64)
    if not pose.refine:
        return None
    ref = pipe.refine_poses(keypoints_pixel, kp_depth, first, second, matches, camera, est, pose.threshold, pose.huber, pose.iterations,
                            weights=weight)
    for key in _REFINE_INT:
        rb.add("refine." + key, ref[key], np.int64)
    for key in ("T", "info") + _REFINE_REAL + (() if weight is None else ("weight_sum",)):
        rb.add("refine." + key, ref[key], np.float64)
    return ref


def _pairs_host(host, rows, pairs, poses, spacing) -> dict:
    """The host-side figures of `pairs`, the rows `rows` (a slice) of the launch whose read-back `host` is."""
    of = lambda name: host[name][rows]
    out = {"pairs": list(pairs), "T": _as44(of("ransac.T"))}
    out.update({key: of("ransac." + key) for key in _INT_KEYS})
    out.update(match_count=of("match_count"), rms=of("ransac.rms"))
    if "refine.T" not in host:
        _summaries(out, out["T"], poses, pairs, spacing)
        return out
    ransac = {key: out[key] for key in ("T", "inlier_count", "rms", "match_count")}
    _summaries(ransac, ransac["T"], poses, pairs, spacing)
    del ransac["match_count"]
    out.update(T=_as44(of("refine.T")), inlier_count=of("refine.inlier_count"), rms=of("refine.rms"))
    _summaries(out, out["T"], poses, pairs, spacing)
    out["ransac"] = ransac
    out["refine"] = {key: of("refine." + key) for key in ("status", "iterations", "selected_count", "cost_in", "cost")}
    out["refine"]["info"] = info_matrix(of("refine.info"))
    if "refine.weight_sum" in host:
        out["refine"]["weight_sum"] = of("refine.weight_sum")
    return out


def _estimate(pipe, keypoints_pixel, kp_depth, pairs, matches, camera, poses, spacing, pose, weight=None) -> dict:
    """The launches of `pose` (a PoseSettings) on the listed pairs, ONE host read-back, the host-side figures."""
    rb = Readback()
    _launch(pipe, rb, keypoints_pixel, kp_depth, pairs, matches, camera, pose, weight)
    return _pairs_host(rb.fetch(), slice(None), pairs, poses, spacing)


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
    pose = PoseSettings(threshold, hypotheses, seed, refine, huber, iterations, weights)
    pose.check_pipeline(pipe)
    src = tokens if tokens is not None else images_u8
    if src is None:
        raise ValueError("images_u8 or tokens= required")
    pairs = consecutive_pairs(int(src.shape[0]), spacing, num_pairs)
    if not pairs:
        raise ValueError(f"{int(src.shape[0])} frames hold no pair at spacing {spacing}")
    n = pairs[-1][1] + 1
    camera = _check_arguments(depth, None, camera, poses, n)
    rule = MatchRule.mnn_ratio(0.9) if rule is None else rule
    ex = pipe.extract(pipe.tokens_from_images(images_u8[:n]) if tokens is None else tokens[:n], None)
    kp = geometry_bank(ex, subcell)
    kp_depth = gather_keypoint_depth(pipe, depth, kp, n)
    matches = pipe.match_pairs(ex["descriptors"], ex["scores"], first=[a for a, _ in pairs], second=[b for _, b in pairs], rule=rule)
    weight = None if weights is None else pipe.match_weights(ex["confidence"], [a for a, _ in pairs], [b for _, b in pairs], matches, weights)
    return _estimate(pipe, kp, kp_depth, pairs, matches, camera, poses, spacing, pose, weight)


def odometry_result(pipe, result: dict, depth=None, camera=None, poses=None, spacing: int = 1, num_pairs=None,
                    threshold: float = 3.0, hypotheses: int = 256, seed: int = 0, *, kp_depth=None, refine: bool = False, huber=None,
                    iterations: int = 5, subcell=None) -> dict:
    """odometry() for a StreamingSequence.result() / run_frames / run_directory result: the keypoints and the match lists of every
    pair (i, i + spacing) are already in device memory, under whichever rule the sequence was run with, so nothing is extracted
    or matched again.  depth=: the raw depth images of the result's frames; kp_depth=: instead, the (N, K) int32 bank
    gather_keypoint_depth returned for result["frames"]["keypoints_pixel"], as evaluation.evaluate_result takes it.
    refine, huber, iterations, subcell: as odometry() takes them; a kp_depth= bank must have been gathered under the same bank
    (evaluation.geometry_bank(result["frames"], subcell))."""
    pose = PoseSettings(threshold, hypotheses, seed, refine, huber, iterations)
    if not isinstance(result, dict) or "frames" not in result or "keypoints_pixel" not in result["frames"]:
        raise ValueError("a StreamingSequence / run_directory result expected")
    kp = geometry_bank(result["frames"], subcell)
    pairs = consecutive_pairs(int(kp.shape[0]), spacing, num_pairs)
    if not pairs or spacing not in result:
        raise ValueError(f"the result holds no pair at spacing {spacing}")
    n = pairs[-1][1] + 1
    camera = _check_arguments(depth, kp_depth, camera, poses, n, kp.shape)
    mm = result[spacing]
    matches = {key: mm[key][:len(pairs)] for key in ("matches", "match_count")}
    if kp_depth is None:
        kp_depth = gather_keypoint_depth(pipe, depth, kp, n)
    return _estimate(pipe, kp, kp_depth, pairs, matches, camera, poses, spacing, pose)


# ------------------------------------------------------------------------------------------------ the pose graph over all spacings
GRAPH_SPACINGS = (1, 5, 10, 15, 20)          # the reference's own set
_GRAPH_INT = ("status", "iterations", "used_edges", "skipped_edges", "failed_row")


def _check_graph(spacings, n_frames, num_pairs, band) -> tuple:
    """What the graph's spacings and band can be refused for, before any device work -> (the spacings that hold a pair, their pair
    lists, the number of frames they name, the band).  The solver's settings are a GraphSettings, judged where it is built."""
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
    if n > lib.GRAPH_MAX_NODES:
        raise lib.SslamHipError(f"odometry_graph: {n} frames, the pose graph takes {lib.GRAPH_MAX_NODES}")
    return tuple(lists), lists, n, band


@dataclass
class _Sequence:
    """What a graph call works on once its arguments are judged: the geometry bank kp and the depth under it, the pair list of every
    spacing that holds one, the n frames they name (the graph's nodes), the band, the camera and the true poses or None; from the
    frames themselves also what was extracted, ex, and the rule to match it under."""
    kp: torch.Tensor
    lists: dict
    n: int
    band: int
    camera: object
    poses: object
    kp_depth: torch.Tensor | None = None
    ex: dict | None = None
    rule: MatchRule | None = None

    @property
    def pairs(self) -> list:
        return [pr for s in self.lists for pr in self.lists[s]]


def _sequence_preamble(pipe, images_u8, tokens, depth, camera, poses, spacings, num_pairs, rule, subcell, band) -> _Sequence:
    """What odometry_graph and odometry_loop_graph do alike before they match: the sequence's arguments judged, the frames extracted
    once, the geometry bank, the keypoints' depth."""
    check_subcell(subcell)
    src = tokens if tokens is not None else images_u8
    if src is None:
        raise ValueError("images_u8 or tokens= required")
    _, lists, n, band = _check_graph(spacings, int(src.shape[0]), num_pairs, band)
    camera = _check_arguments(depth, None, camera, poses, n)
    rule = MatchRule.mnn_ratio(0.9) if rule is None else rule
    ex = pipe.extract(pipe.tokens_from_images(images_u8[:n]) if tokens is None else tokens[:n], None)
    kp = geometry_bank(ex, subcell)
    return _Sequence(kp, lists, n, band, camera, poses, gather_keypoint_depth(pipe, depth, kp, n), ex, rule)


def _result_preamble(pipe, result, keys, depth, kp_depth, camera, poses, spacings, num_pairs, subcell, band) -> _Sequence:
    """What odometry_result_graph and odometry_result_loop_graph do alike: the result must hold `keys` per frame; the geometry bank,
    the result's spacings if none are given, the sequence's arguments judged, the keypoints' depth gathered unless it is given."""
    if not isinstance(result, dict) or "frames" not in result or any(key not in result["frames"] for key in keys):
        raise ValueError("a StreamingSequence / run_directory result expected")
    kp = geometry_bank(result["frames"], subcell)
    if spacings is None:
        spacings = tuple(sorted(k for k in result if isinstance(k, (int, np.integer)) and not isinstance(k, bool)))
    if any(s not in result for s in spacings):
        raise ValueError(f"the result holds no pairs at every spacing of {tuple(spacings)!r}")
    _, lists, n, band = _check_graph(spacings, int(kp.shape[0]), num_pairs, band)
    camera = _check_arguments(depth, kp_depth, camera, poses, n, kp.shape)
    return _Sequence(kp, lists, n, band, camera, poses, gather_keypoint_depth(pipe, depth, kp, n) if kp_depth is None else kp_depth)


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


def _read_graph(rb, name, g) -> None:
    """A graph's device tensors join the read-back rb under '<name>.<key>'; a sparse graph's cg_steps with them."""
    for key in _GRAPH_INT + (("cg_steps",) if "cg_steps" in g else ()):
        rb.add(f"{name}.{key}", g[key], np.int64)
    for key in ("C", "cost_in", "cost", "edge_chi2"):
        rb.add(f"{name}.{key}", g[key], np.float64)


def _graph_host(host, name, pairs, poses) -> dict:
    """The host-side figures of the graph _read_graph recorded as `name`."""
    graph = {"trajectory": camera_to_world(host[name + ".C"]), "pairs": pairs}
    graph.update({key: int(host[f"{name}.{key}"]) for key in _GRAPH_INT})
    graph.update(cost_in=float(host[name + ".cost_in"]), cost=float(host[name + ".cost"]), edge_chi2=host[name + ".edge_chi2"])
    if poses is not None:
        graph["ate"] = ate_summary(graph["trajectory"], np.asarray(poses, dtype=np.float64)[:len(graph["trajectory"])])
    if name + ".cg_steps" in host:
        graph["cg_steps"] = host[name + ".cg_steps"]
    return graph


def _spacings_and_graph(host, lists, pairs, poses) -> dict:
    """Every spacing's dictionary from its rows of the launch, and 'graph'."""
    out, at = {}, 0
    for s in lists:
        out[s] = _pairs_host(host, slice(at, at + len(lists[s])), lists[s], poses, s)
        at += len(lists[s])
    out["graph"] = _graph_host(host, "graph", pairs, poses)
    if poses is not None:
        out["graph"]["ate_chain"] = out[1]["ate"]
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
def _tracks_device(pipe, rb, seq, matches, ref, C, opt, confidence) -> None:
    """Links from the spacing-1 rows masked by the refinement's inlier_of_slot, their ids, the landmarks under the graph's C; what
    the host wants of them joins the read-back rb under 'tracks.<key>'.  No host read."""
    lists, n = seq.lists, seq.n
    at = sum(len(lists[s]) for s in list(lists)[:list(lists).index(1)])
    rows = slice(at, at + len(lists[1]))
    links = pipe.link_matches([a for a, _ in lists[1]], [b for _, b in lists[1]], {key: matches[key][rows] for key in ("matches", "match_count")},
                              mask=ref["inlier_of_slot"][rows], n_frames=n, k=int(seq.kp.shape[1]))
    tr = pipe.track_ids(links)
    lm = pipe.landmarks(seq.kp[:n], seq.kp_depth[:n], C.reshape(n, 12), tr, seq.camera, opt["threshold"], opt["min_obs"],
                        weights=None if confidence is None else confidence[:n])
    rb.add("tracks.n_tracks", tr["n_tracks"], np.int64)
    rb.add("tracks.track_id", tr["track_id"], np.int32)
    for key, t, dtype in (("length", tr["length"], np.int64), ("status", lm["status"], np.int32), ("n_kept", lm["n_kept"], np.int32),
                          ("rms", lm["rms"], np.float64), ("xyz", lm["xyz"], np.float64)):
        rb.add("tracks." + key, t, dtype, rows="tracks.n_tracks")         # a row per keypoint on the device, n_tracks of them filled


def _tracks_host(host) -> dict:
    """The host-side figures of the tracks _tracks_device recorded."""
    from .track_numpy import length_statistics
    nt = int(host["tracks.n_tracks"][0])
    out = {"n_tracks": nt, "length": length_statistics(host["tracks.length"], [nt]), "track_id": host["tracks.track_id"],
           "landmarks": host["tracks.xyz"], "status": host["tracks.status"], "n_kept": host["tracks.n_kept"], "rms": host["tracks.rms"]}
    del out["length"]["n_tracks"]
    return out


def _graph(pipe, seq, matches, pose, graph, weight=None, tracks=None, confidence=None) -> dict:
    """One RANSAC and one refinement launch over the concatenated pair lists of seq, the chain, the graph, ONE read-back.  weight: the
    (P, n1) weights of the weighted refinement, whose info the graph then reads as it reads the unweighted one.  tracks:
    check_tracks' dictionary - the links, ids and landmarks (weighted by `confidence` where given) join the same read-back."""
    rb, pairs = Readback(), seq.pairs
    ref = _launch(pipe, rb, seq.kp, seq.kp_depth, pairs, matches, seq.camera, pose, weight)
    g = _graph_device(pipe, ref, pairs, seq.lists, seq.n, seq.poses, seq.band, graph.huber_chi, graph.damping, graph.iterations)
    _read_graph(rb, "graph", g)
    if tracks is not None:
        _tracks_device(pipe, rb, seq, matches, ref, g["C"], tracks, confidence)
    host = rb.fetch()                                        # the ONE read-back
    out = _spacings_and_graph(host, seq.lists, pairs, seq.poses)
    if tracks is not None:
        out["tracks"] = _tracks_host(host)
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
    pose = PoseSettings(threshold, hypotheses, seed, True, huber, iterations, weights)
    pose.check_pipeline(pipe)
    graph, opt = GraphSettings(huber_chi, damping, graph_iterations), check_tracks(tracks)
    seq = _sequence_preamble(pipe, images_u8, tokens, depth, camera, poses, spacings, num_pairs, rule, subcell, band)
    ex, first, second = seq.ex, [a for a, _ in seq.pairs], [b for _, b in seq.pairs]
    matches = pipe.match_pairs(ex["descriptors"], ex["scores"], first=first, second=second, rule=seq.rule)
    weight = None if weights is None else pipe.match_weights(ex["confidence"], first, second, matches, weights)
    return _graph(pipe, seq, matches, pose, graph, weight, opt, None if weights is None or opt is None else ex["confidence"])


def odometry_result_graph(pipe, result: dict, depth=None, camera=None, poses=None, spacings=None, num_pairs=None, threshold: float = 3.0,
                          hypotheses: int = 256, seed: int = 0, *, kp_depth=None, huber=None, iterations: int = 5, subcell=None, band=None,
                          huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 8) -> dict:
    """odometry_graph() for a StreamingSequence.result() / run_frames / run_directory result: nothing is extracted or matched again.
    spacings: those of the result if None.  depth= / kp_depth=, and everything else: as odometry_result() and odometry_graph()
    take them."""
    pose, graph = PoseSettings(threshold, hypotheses, seed, True, huber, iterations), GraphSettings(huber_chi, damping, graph_iterations)
    seq = _result_preamble(pipe, result, ("keypoints_pixel",), depth, kp_depth, camera, poses, spacings, num_pairs, subcell, band)
    matches = {key: torch.cat([result[s][key][:len(seq.lists[s])] for s in seq.lists]) for key in ("matches", "match_count")}
    return _graph(pipe, seq, matches, pose, graph)


# ------------------------------------------------------------------------------------------------------------------ loop closures
LOOP_DEFAULTS = dict(min_gap=30, min_sim=0.3, per_frame=2, suppress=5, min_inliers=12)


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


def _loop_graph(pipe, seq, matches, cand, pose, graph, opt, cg_iterations, cg_tol, prune_chi) -> dict:
    """One RANSAC and one refinement launch over the spacings' pairs followed by the candidate slots, the chain and the banded graph
    over the former, the sparse graph over all of them from the banded graph's poses, ONE read-back."""
    rb, pairs = Readback(), seq.pairs
    P, dev = len(pairs), seq.kp.device
    of = torch.tensor([a for a, _ in pairs], dtype=torch.int32, device=dev)
    first = torch.cat([of, cand["first"]])
    second = torch.cat([torch.tensor([b for _, b in pairs], dtype=torch.int32, device=dev), cand["second"]])
    ref = _launch_lists(pipe, rb, seq.kp, seq.kp_depth, first, second, matches, seq.camera, pose)
    g = _graph_device(pipe, {key: ref[key][:P] for key in ("T", "info", "status")}, pairs, seq.lists, seq.n, seq.poses, seq.band,
                      graph.huber_chi, graph.damping, graph.iterations)
    kept = (cand["first"] >= 0) & (ref["status"][P:] != lib.REFINE_NOT_ATTEMPTED) & (ref["inlier_count"][P:] >= int(opt["min_inliers"]))
    absent = torch.full_like(first, -1)
    gfirst = torch.cat([of, torch.where(kept, cand["first"], absent[P:])])
    sparse = lambda f: pipe.optimize_pose_graph_sparse(f, second, ref, ref, seq.n, g["C"], graph.huber_chi, graph.damping, graph.iterations,
                                                       cg_iterations, cg_tol)
    runs = {"loop_graph": sparse(gfirst)}
    if prune_chi is not None:
        gone = runs["loop_graph"]["edge_chi2"] > float(prune_chi) * float(prune_chi)
        runs = {"loop_graph_unpruned": runs["loop_graph"], "loop_graph": sparse(torch.where(gone, absent, gfirst))}
    _read_graph(rb, "graph", g)
    for name, r in runs.items():
        _read_graph(rb, name, r)
    for key, dtype in (("first", np.int32), ("second", np.int32), ("sim", np.float32), ("count", np.int32)):
        rb.add("loops." + key, cand[key], dtype)
    rb.add("loops.kept", kept, np.bool_)
    host = rb.fetch()                                        # the ONE read-back
    out = _spacings_and_graph(host, seq.lists, pairs, seq.poses)
    out["loops"] = {key: host["loops." + key] for key in ("first", "second", "sim", "count", "kept")}
    out["loops"].update(match_count=host["match_count"][P:], T=_as44(host["refine.T"][P:]), status=host["refine.status"][P:],
                        inlier_count=host["refine.inlier_count"][P:], info=info_matrix(host["refine.info"][P:]))
    all_pairs = pairs + [(int(a), int(b)) for a, b in zip(host["loops.first"], host["loops.second"])]
    for name in runs:
        out[name] = _graph_host(host, name, all_pairs, seq.poses)
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
    pose, graph = PoseSettings(threshold, hypotheses, seed, True, huber, iterations), GraphSettings(huber_chi, damping, graph_iterations)
    opt = check_loops(loops, cg_iterations, cg_tol, prune_chi)
    seq = _sequence_preamble(pipe, images_u8, tokens, depth, camera, poses, spacings, num_pairs, rule, subcell, band)
    ex, pairs, dev = seq.ex, seq.pairs, seq.kp.device
    cand = pipe.find_loop_candidates(ex["descriptors"], ex["scores"], opt["min_gap"], opt["min_sim"], opt["per_frame"], opt["suppress"])
    first = torch.cat([torch.tensor([a for a, _ in pairs], dtype=torch.int32, device=dev), cand["first"]])
    second = torch.cat([torch.tensor([b for _, b in pairs], dtype=torch.int32, device=dev), cand["second"]])
    matches = pipe.match_pairs(ex["descriptors"], ex["scores"], first=first, second=second, rule=seq.rule)
    return _loop_graph(pipe, seq, matches, cand, pose, graph, opt, cg_iterations, cg_tol, prune_chi)


def odometry_result_loop_graph(pipe, result: dict, depth=None, camera=None, poses=None, spacings=None, num_pairs=None, threshold: float = 3.0,
                               hypotheses: int = 256, seed: int = 0, *, kp_depth=None, huber=None, iterations: int = 5, subcell=None,
                               band=None, huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 8, loops=None,
                               cg_iterations: int = 512, cg_tol: float = 1e-3, prune_chi=None, rule=None) -> dict:
    """odometry_loop_graph() for a StreamingSequence.result() / run_frames / run_directory result: nothing is extracted again and the
    spacings' pairs keep the match lists the sequence was run with; only the candidate slots are matched, in one match_pairs call
    under `rule` (MatchRule.mnn_ratio(0.9) if None - give the rule the sequence was run with).  Everything else: as
    odometry_result_graph() and odometry_loop_graph() take it."""
    pose, graph = PoseSettings(threshold, hypotheses, seed, True, huber, iterations), GraphSettings(huber_chi, damping, graph_iterations)
    opt = check_loops(loops, cg_iterations, cg_tol, prune_chi)
    seq = _result_preamble(pipe, result, ("keypoints_pixel", "descriptors", "scores"), depth, kp_depth, camera, poses, spacings, num_pairs, subcell,
                           band)
    rule = MatchRule.mnn_ratio(0.9) if rule is None else rule
    desc, scores = result["frames"]["descriptors"][:seq.n], result["frames"]["scores"][:seq.n]
    cand = pipe.find_loop_candidates(desc, scores, opt["min_gap"], opt["min_sim"], opt["per_frame"], opt["suppress"])
    far = pipe.match_pairs(desc, scores, first=cand["first"], second=cand["second"], rule=rule)
    matches = {key: torch.cat([result[s][key][:len(seq.lists[s])] for s in seq.lists] + [far[key]]) for key in ("matches", "match_count")}
    return _loop_graph(pipe, seq, matches, cand, pose, graph, opt, cg_iterations, cg_tol, prune_chi)
