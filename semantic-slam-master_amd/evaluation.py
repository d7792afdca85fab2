"""Home of the reference's three pose-based scoring functions, with their original signatures, return types and dictionary
keys, running on the HIP kernels sslam_pose_nn_pairs / sslam_match_score_pairs (csrc/evaluate.hip):

    compute_repeatability          RepeatabilityTester.compute_repeatability              test/test_repeatability.py:79-128
    compute_ground_truth_matches   DescriptorQualityTester.compute_ground_truth_matches   test/test_descriptor_quality.py:144-185
    evaluate_matches               DescriptorQualityTester.evaluate_matches               test/test_descriptor_quality.py:187-231

Beside them, with the same return conventions, the two functions of the depth ground truth (csrc/evaluate.hip):
compute_repeatability_depth and compute_ground_truth_matches_depth - and, beside matching.py's matchers, the step that follows
them: estimate_relative_pose, the rigid motion a match list agrees on (csrc/pose_estimate.hip), and refine_relative_pose, that
motion - or any other initial pose - refined on the reprojection error (csrc/pose_refine.hip), and optimize_pose_graph, the
poses of a whole sequence from those motions and their information matrices (csrc_graph/pose_graph.hip), with find_loop_candidates and
optimize_pose_graph_sparse, the loop closures on top of it (csrc_loop/loop.hip).  And, between the selector and all
of them, refine_keypoints_subcell: the selected cells moved to their sub-cell saliency peaks (csrc_ext/subcell.hip).

numpy in -> numpy out like the originals; torch CUDA tensors are accepted too and then nothing leaves the device except the
result.  There is no CPU implementation here: without the GPU library these functions raise.  The exceptions are PoseWindow, the
online sliding-window estimator, and PlaceBank and EdgeLog, the online loop retrieval and its edge list, which are numpy by design
(a front end steps them once per frame on the host) and give the device entries' bits.

The two keypoint sets may differ in size: they go to the device as a two-frame bank (2, max(N, M), 2), zero rows behind the
shorter set, and the entry is told how many rows of each frame count (its n1 / n2 arguments), so the padding is never read.
Keypoints are taken as float32 - what every extractor here and in the reference returns - and all arithmetic is float64,
also with H=None, where the original stays in float32 (its distances differ from these by float32 rounding, ~1e-7 relative).
"""
from __future__ import annotations

import numpy as np
import torch

from sslam_amd import lib
from sslam_amd.evaluation import check_depth_size, match_metrics


def _dev(a, dtype):
    if isinstance(a, torch.Tensor):
        return a.detach().to("cuda", dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


def _pose_nn(kpts1, kpts2, H, threshold):
    k1, k2 = _dev(kpts1, torch.float32), _dev(kpts2, torch.float32)
    if k1.dim() != 2 or k2.dim() != 2 or k1.shape[1] != 2 or k2.shape[1] != 2 or k1.shape[0] < 1 or k2.shape[0] < 1:
        raise ValueError(f"keypoints (N >= 1, 2) and (M >= 1, 2) expected, got {tuple(k1.shape)} and {tuple(k2.shape)}")
    n, m = int(k1.shape[0]), int(k2.shape[0])
    bank = torch.zeros((2, max(n, m), 2), dtype=torch.float32, device=k1.device)
    bank[0, :n], bank[1, :m] = k1, k2
    if H is not None:
        H = _dev(H, torch.float64)
        if tuple(H.shape) != (3, 3):
            raise ValueError(f"H (3, 3) expected, got {tuple(H.shape)}")
        H = H.reshape(1, 9)
    first = torch.zeros((1,), dtype=torch.int32, device=k1.device)
    return n, lib.pose_nn_pairs(bank, first, first + 1, H, threshold, n1=n, n2=m)


def compute_repeatability(kpts1, kpts2, H=None, threshold: float = 3.0) -> dict:
    """Repeatability of kpts1 (N, 2) in kpts2 (M, 2) under the homography H (3, 3) frame 1 -> frame 2, or the raw coordinates.
    Returns the original's dictionary: repeatability, repeatable_count, total_keypoints, mean_nn_distance, median_nn_distance."""
    n, (_, cnt, _, dsum, dmed) = _pose_nn(kpts1, kpts2, H, threshold)
    c, s, med = torch.stack([cnt.to(torch.float64), dsum, dmed]).reshape(3).tolist()      # one read-back
    repeatable = np.int64(c)
    return {"repeatability": repeatable / n, "repeatable_count": repeatable, "total_keypoints": n,
            "mean_nn_distance": np.float64(s) / n, "median_nn_distance": np.float64(med)}


def compute_ground_truth_matches(kpts1, kpts2, H, threshold: float = 3.0):
    """Ground-truth matches (K, 2) int64 [idx1, idx2]: the rows of kpts1 whose warp lands within `threshold` pixels of a point of
    kpts2, with the nearest such point (the lowest index among equally near ones).  numpy for numpy input, a device tensor else."""
    if H is None:
        raise ValueError("compute_ground_truth_matches needs the homography H")
    _, (gt, cnt, _, _, _) = _pose_nn(kpts1, kpts2, H, threshold)
    out = gt[0, :int(cnt.item())]
    return out if isinstance(kpts1, torch.Tensor) else out.cpu().numpy()


def _pose_depth_nn(kpts1, kpts2, depth1, T_rel, camera, threshold):
    lib.check_camera(camera)                                 # the camera and the depth image are judged before any device work
    if isinstance(depth1, np.ndarray):
        depth1 = torch.from_numpy(np.ascontiguousarray(depth1))
    if not isinstance(depth1, torch.Tensor) or depth1.dtype != torch.uint16 or depth1.dim() != 2:
        raise ValueError("depth1 (h, w) uint16 expected: frame 1's raw depth image")
    check_depth_size(depth1.shape[1], depth1.shape[0], camera)   # a camera that is not this image's would score against another view
    k1, k2 = _dev(kpts1, torch.float32), _dev(kpts2, torch.float32)
    if k1.dim() != 2 or k2.dim() != 2 or k1.shape[1] != 2 or k2.shape[1] != 2 or k1.shape[0] < 1 or k2.shape[0] < 1:
        raise ValueError(f"keypoints (N >= 1, 2) and (M >= 1, 2) expected, got {tuple(k1.shape)} and {tuple(k2.shape)}")
    T = _dev(T_rel, torch.float64)
    if tuple(T.shape) not in ((4, 4), (3, 4)):
        raise ValueError(f"T_rel (4, 4) or (3, 4) expected, got {tuple(T.shape)}")
    n, m = int(k1.shape[0]), int(k2.shape[0])
    bank = torch.zeros((2, max(n, m), 2), dtype=torch.float32, device=k1.device)
    bank[0, :n], bank[1, :m] = k1, k2
    kp_depth = torch.full((2, max(n, m)), -1, dtype=torch.int32, device=k1.device)
    lib.keypoint_depth(depth1.to(k1.device).contiguous()[None], bank[:1], out=kp_depth[:1])      # pixel units: scale 1
    first = torch.zeros((1,), dtype=torch.int32, device=k1.device)
    return n, lib.pose_depth_nn_pairs(bank, kp_depth, first, first + 1, T[:3].contiguous().reshape(1, 12), camera, threshold=threshold,
                                      n1=n, n2=m)


def compute_repeatability_depth(kpts1, kpts2, depth1, T_rel, camera, threshold: float = 3.0) -> dict:
    """compute_repeatability against the depth ground truth: kpts1 (N, 2) and kpts2 (M, 2) in the pixels of the depth image
    depth1 (h, w) uint16 of frame 1 (the reference's convention: scale 1), T_rel (4, 4) from camera 1 to camera 2
    (sslam_amd.evaluation.relative_transform), camera an sslam_amd.evaluation.Camera.  Returns compute_repeatability's dictionary
    plus valid_keypoints: repeatability and mean_nn_distance are over the keypoints that HAVE a ground truth (a depth
    measurement, in front of camera 2, inside its view), 0.0 when there is none."""
    n, (_, cnt, _, valid, dsum, dmed) = _pose_depth_nn(kpts1, kpts2, depth1, T_rel, camera, threshold)
    c, v, s, med = torch.stack([cnt.to(torch.float64), valid.to(torch.float64), dsum, dmed]).reshape(4).tolist()      # one read-back
    repeatable, v = np.int64(c), np.int64(v)
    return {"repeatability": repeatable / v if v > 0 else 0.0, "repeatable_count": repeatable, "total_keypoints": n,
            "valid_keypoints": v, "mean_nn_distance": np.float64(s) / v if v > 0 else 0.0, "median_nn_distance": np.float64(med)}


def compute_ground_truth_matches_depth(kpts1, kpts2, depth1, T_rel, camera, threshold: float = 3.0):
    """compute_ground_truth_matches against the depth ground truth (arguments as compute_repeatability_depth): (K, 2) int64
    [idx1, idx2].  numpy for numpy keypoints, a device tensor else."""
    _, (gt, cnt, _, _, _, _) = _pose_depth_nn(kpts1, kpts2, depth1, T_rel, camera, threshold)
    out = gt[0, :int(cnt.item())]
    return out if isinstance(kpts1, torch.Tensor) else out.cpu().numpy()


def _pair_on_device(who, kp1, kp2, depth1, depth2, matches, camera):
    """One pair as the pose entries take it: (bank (2, k, 2), kp_depth (2, k), first, count, matches (1, P, 2)) on the device, or
    None for an empty match list.  Everything is judged before any device work."""
    depths = []
    for name, d in (("depth1", depth1), ("depth2", depth2)):
        d = torch.from_numpy(np.ascontiguousarray(d)) if isinstance(d, np.ndarray) else d
        if not isinstance(d, torch.Tensor) or d.dtype != torch.uint16 or d.dim() != 2:
            raise ValueError(f"{name} (h, w) uint16 expected: the frame's raw depth image")
        check_depth_size(d.shape[1], d.shape[0], camera)
        depths.append(d)
    k1, k2 = np.asarray(kp1, dtype=np.float32), np.asarray(kp2, dtype=np.float32)
    if k1.ndim != 2 or k2.ndim != 2 or k1.shape[1] != 2 or k2.shape[1] != 2 or k1.shape[0] < 1 or k2.shape[0] < 1:
        raise ValueError(f"keypoints (N >= 1, 2) and (M >= 1, 2) expected, got {k1.shape} and {k2.shape}")
    mt = np.asarray(matches)
    if mt.size == 0:
        return None
    if mt.ndim != 2 or mt.shape[1] != 2 or mt.dtype.kind not in "iu":
        raise ValueError(f"matches (P, 2) of integer indices expected, got {mt.shape} {mt.dtype}")
    k, p = max(len(k1), len(k2), len(mt)), len(mt)
    if k > lib.EVAL_MAX_K:
        raise lib.SslamHipError(f"{who}: {k} keypoints or matches; at most {lib.EVAL_MAX_K} are handled on the device")
    bank = torch.zeros((2, k, 2), dtype=torch.float32, device="cuda")
    bank[0, :len(k1)], bank[1, :len(k2)] = _dev(k1, torch.float32), _dev(k2, torch.float32)
    kp_depth = torch.full((2, k), -1, dtype=torch.int32, device="cuda")         # the padding rows: no depth, never usable
    for f, (d, n) in enumerate(zip(depths, (len(k1), len(k2)))):
        kp_depth[f, :n] = lib.keypoint_depth(d.to("cuda").contiguous()[None], bank[f:f + 1, :n].contiguous())[0]      # pixel units: scale 1
    first = torch.zeros((1,), dtype=torch.int32, device="cuda")
    count = torch.full((1,), p, dtype=torch.int32, device="cuda")
    return bank, kp_depth, first, count, _dev(mt.astype(np.int64)[None], torch.int64)


def estimate_relative_pose(kp1, kp2, depth1, depth2, matches, camera=None, threshold: float = 3.0, hypotheses: int = 256, seed: int = 0):
    """The rigid motion from camera 1 to camera 2 that the matches agree on: kp1 (N, 2) and kp2 (M, 2) in the pixels of the raw
    depth images depth1, depth2 (h, w) uint16 of their frames (scale 1), matches (P, 2) [idx1, idx2] as a matcher returns them,
    camera an sslam_amd.evaluation.Camera (the default one if None).  RANSAC over 3-point samples of the matches with a depth on
    both sides, Horn's closed form, a refit over the inliers (sslam_pose_ransac_pairs, include/sslam_hip.h); threshold is the
    reprojection distance in pixels.  numpy in, numpy out; one pair.
    Returns (T (4, 4) float64 with X_2 = T X_1 - the identity when fewer than 3 matches have both depths -, inlier mask (P,) bool)."""
    from sslam_amd.evaluation import Camera
    camera = Camera() if camera is None else camera
    lib.check_camera(camera)
    t, n_hyp, seed = lib.check_threshold(threshold), lib.check_hypotheses(hypotheses), lib.check_seed(seed)
    pair = _pair_on_device("estimate_relative_pose", kp1, kp2, depth1, depth2, matches, camera)
    if pair is None:
        return np.eye(4), np.zeros(0, bool)
    bank, kp_depth, first, count, mt = pair
    out = lib.pose_ransac_pairs(bank, kp_depth, first, first + 1, mt, count, camera, 1.0, 1.0, t, n_hyp, seed)
    T = np.eye(4)
    T[:3] = out[0].cpu().numpy().reshape(3, 4)
    return T, out[5][0].cpu().numpy() == 1


def match_weights(conf1, conf2, matches, mode: str = "product", sigma0: float = 1.0) -> np.ndarray:
    """The weight of every match for refine_relative_pose(weights=), from the two frames' keypoint confidences conf1 (N,) and
    conf2 (M,) float32 (UncertaintyEstimator's output) and matches (P, 2) [idx1, idx2]: (P,) float32.  mode "product": c1 * c2;
    mode "expected_error": sigma0^2 / (sigma0^2 + e1^2 + e2^2) with e = 1 / (c + 1e-6) - 1 in float64, the error at which the
    reference's compute_expected_error_loss is least for that confidence (include/sslam_weight.h: sslu_match_weights' bits).  A
    match with an index outside its frame gets 0.  numpy in, numpy out; needs no GPU."""
    modes = {"product": lib.WEIGHT_PRODUCT, "expected_error": lib.WEIGHT_EXPECTED_ERROR}
    if mode not in modes:
        raise ValueError(f"mode must be one of {tuple(modes)}, got {mode!r}")
    _, s0 = lib.check_weights(modes[mode], sigma0)
    c1, c2 = np.asarray(conf1, dtype=np.float32), np.asarray(conf2, dtype=np.float32)
    mt = np.asarray(matches)
    if c1.ndim != 1 or c2.ndim != 1:
        raise ValueError(f"confidences (N,) and (M,) expected, got {c1.shape} and {c2.shape}")
    if mt.size == 0:
        return np.zeros(0, np.float32)
    if mt.ndim != 2 or mt.shape[1] != 2 or mt.dtype.kind not in "iu":
        raise ValueError(f"matches (P, 2) of integer indices expected, got {mt.shape} {mt.dtype}")
    from sslam_amd import weight_numpy
    return weight_numpy.match_weights(c1, c2, mt, modes[mode], s0)


def refine_relative_pose(kp1, kp2, depth1, depth2, matches, T, camera=None, threshold: float = 3.0, huber=None, iterations: int = 5,
                         weights=None):
    """The step behind estimate_relative_pose: the pose T (4, 4) or (3, 4) from camera 1 to camera 2 - that function's, or any other
    initial pose - refined by Gauss-Newton on the Huber cost of the reprojection error over the matches T agrees with at
    `threshold` (sslam_pose_refine_pairs, include/sslam_hip.h).  kp1 .. camera as estimate_relative_pose takes them; huber: the
    Huber delta in pixels, threshold / 3 if None; iterations: the most steps.  numpy in, numpy out; one pair.
    Returns (T (4, 4) float64 - the T given when no step lowers the cost or the result would lose inliers -, inlier mask (P,) bool,
    info (6, 6) float64: the information matrix of the returned pose in the parameters (vx, vy, vz, wx, wy, wz) of a left
    perturbation in camera 2; zero when the refinement was not attempted).
    weights: None, or a (P,) float32 array aligned with matches - match_weights' output, or any other: the weighted refinement
    runs (sslu_pose_refine_weighted_pairs' statement, include/sslam_weight.h): a match whose weight is not finite and > 0 takes no
    part, the others' terms are multiplied by their weights, and info is the weighted information matrix.  This form needs NO
    GPU: it runs the header's statement in numpy float64 (sslam_amd/weight_numpy.py) and gives the bits the device entry gives - a
    caller on the device uses SequencePipeline.refine_poses(weights=)."""
    from sslam_amd.evaluation import Camera
    camera = Camera() if camera is None else camera
    lib.check_camera(camera)
    t, n_iter = lib.check_threshold(threshold), lib.check_iterations(iterations)
    hub = lib.check_huber(t / 3.0 if huber is None else huber)
    T0 = np.asarray(T, dtype=np.float64)
    if T0.shape not in ((4, 4), (3, 4)):
        raise ValueError(f"T (4, 4) or (3, 4) expected, got {T0.shape}")
    if weights is not None:
        weights = np.asarray(weights)
        if weights.dtype != np.float32 or weights.shape != (len(np.asarray(matches)),):
            raise ValueError(f"weights must be None or a float32 array of shape ({len(np.asarray(matches))},), got {weights.dtype} {weights.shape}")
        return _refine_weighted_numpy(kp1, kp2, depth1, depth2, matches, T0, camera, t, hub, n_iter, weights)
    pair = _pair_on_device("refine_relative_pose", kp1, kp2, depth1, depth2, matches, camera)
    T4 = np.eye(4)
    T4[:3] = T0[:3]
    if pair is None:
        return T4, np.zeros(0, bool), np.zeros((6, 6))
    bank, kp_depth, first, count, mt = pair
    out = lib.pose_refine_pairs(bank, kp_depth, first, first + 1, mt, count, camera, _dev(np.ascontiguousarray(T0[:3]).reshape(1, 12), torch.float64),
                                1.0, 1.0, t, hub, n_iter)
    T4[:3] = out[0].cpu().numpy().reshape(3, 4)
    tri = out[11][0].cpu().numpy()
    iu = np.triu_indices(6)
    info = np.zeros((6, 6))
    info[iu], info[iu[1], iu[0]] = tri, tri
    return T4, out[7][0].cpu().numpy() == 1, info


def _refine_weighted_numpy(kp1, kp2, depth1, depth2, matches, T0, camera, t, hub, n_iter, weights):
    """refine_relative_pose's weighted form: what _pair_on_device judges, judged alike, then sslam_amd/weight_numpy.py.  No GPU."""
    from sslam_amd import weight_numpy
    depths = []
    for name, d in (("depth1", depth1), ("depth2", depth2)):
        d = d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else d
        if not isinstance(d, np.ndarray) or d.dtype != np.uint16 or d.ndim != 2:
            raise ValueError(f"{name} (h, w) uint16 expected: the frame's raw depth image")
        check_depth_size(d.shape[1], d.shape[0], camera)
        depths.append(d)
    k1, k2 = np.asarray(kp1, dtype=np.float32), np.asarray(kp2, dtype=np.float32)
    if k1.ndim != 2 or k2.ndim != 2 or k1.shape[1] != 2 or k2.shape[1] != 2 or k1.shape[0] < 1 or k2.shape[0] < 1:
        raise ValueError(f"keypoints (N >= 1, 2) and (M >= 1, 2) expected, got {k1.shape} and {k2.shape}")
    mt = np.asarray(matches)
    T4 = np.eye(4)
    T4[:3] = T0[:3]
    if mt.size == 0:
        return T4, np.zeros(0, bool), np.zeros((6, 6))
    if mt.ndim != 2 or mt.shape[1] != 2 or mt.dtype.kind not in "iu":
        raise ValueError(f"matches (P, 2) of integer indices expected, got {mt.shape} {mt.dtype}")
    if max(len(k1), len(k2), len(mt)) > lib.EVAL_MAX_K:
        raise lib.SslamHipError(f"refine_relative_pose: {max(len(k1), len(k2), len(mt))} keypoints or matches; at most {lib.EVAL_MAX_K} are handled")
    out = weight_numpy.refine_pair(k1, k2, weight_numpy.keypoint_depth(depths[0], k1), weight_numpy.keypoint_depth(depths[1], k2), mt,
                                   weights, camera, t, hub, n_iter, np.ascontiguousarray(T0[:3]).reshape(12))
    T4[:3] = out["T"].reshape(3, 4)
    iu = np.triu_indices(6)
    info = np.zeros((6, 6))
    info[iu], info[iu[1], iu[0]] = out["info"], out["info"]
    return T4, out["inlier_of_slot"] == 1, info


def optimize_pose_graph(first, second, T, info, n_nodes: int, C_init=None, band=None, huber_chi: float = 4.0, damping: float = 0.0,
                        iterations: int = 8):
    """The step behind refine_relative_pose: the poses of a sequence from the relative poses of its pairs and their information
    matrices (sslg_pose_graph, include/sslam_graph.h).  first, second: the frames a < b of every pair (integer sequences; -1 in
    first: a pair to leave out); T (E, 4, 4) or (E, 3, 4): camera a -> camera b, as refine_relative_pose returns it; info
    (E, 6, 6): that function's information matrices; C_init (n_nodes, 4, 4) or (n_nodes, 3, 4) world -> camera, or None: the chain
    of the pairs (i, i + 1), each of which must then be listed; band: the most b - a of a pair that is used, the largest listed
    if None.  numpy in, numpy out; one graph.
    Returns (C (n_nodes, 4, 4) float64 world -> camera - C_init when no step lowers the cost -, status (0 optimised, 1 no step
    accepted, 2 a node no pair determines, 3 not attempted), chi2 (E,) float64: every used pair's squared residual at C)."""
    first, second = [int(v) for v in np.asarray(first).reshape(-1)], [int(v) for v in np.asarray(second).reshape(-1)]
    T, info = np.asarray(T, dtype=np.float64), np.asarray(info, dtype=np.float64)
    if T.ndim != 3 or tuple(T.shape[1:]) not in ((4, 4), (3, 4)) or len(T) != len(first) or len(first) != len(second) or not first:
        raise ValueError(f"T (E, 4, 4) or (E, 3, 4) for E = {len(first)} >= 1 pairs expected, got {T.shape}")
    if info.shape != (len(first), 6, 6):
        raise ValueError(f"info ({len(first)}, 6, 6) expected, got {info.shape}")
    if C_init is not None:
        C_init = np.asarray(C_init, dtype=np.float64)
        if C_init.ndim != 3 or tuple(C_init.shape[1:]) not in ((4, 4), (3, 4)) or len(C_init) != n_nodes:
            raise ValueError(f"C_init ({n_nodes}, 4, 4) or ({n_nodes}, 3, 4) expected, got {C_init.shape}")
        C_init = _dev(np.ascontiguousarray(C_init[:, :3]).reshape(n_nodes, 12), torch.float64)
    from sslam_amd.pipeline import SequencePipeline
    iu = np.triu_indices(6)
    out = SequencePipeline.optimize_pose_graph(first, second, _dev(np.ascontiguousarray(T[:, :3]).reshape(-1, 12), torch.float64),
                                               _dev(np.ascontiguousarray(info[:, iu[0], iu[1]]), torch.float64), n_nodes, C_init, band,
                                               huber_chi, damping, iterations)
    C = np.tile(np.eye(4), (n_nodes, 1, 1))
    C[:, :3] = out["C"].cpu().numpy().reshape(n_nodes, 3, 4)
    return C, int(out["status"].cpu()), out["edge_chi2"].cpu().numpy()


class PoseWindow:
    """The online counterpart of optimize_pose_graph: a sliding window over the last `window` frames (sslw_window_step,
    include/sslam_window.h) fed one frame at a time with the relative poses refine_relative_pose returned for the pairs
    (t - s, t), s in `spacings`.  This one class needs NO GPU: it runs the header's statement in numpy float64
    (sslam_amd/window_numpy.py) and gives the bits the device entry gives - a caller on the device uses
    SequencePipeline.pose_window_step or online.WindowPoseFrameStepper.
    window: 2 .. 32 frames, max(spacings) + 1 if None; spacings: up to 8 distinct positive ints; capacity: the frames the
    trajectory keeps; min_inliers, huber_chi, damping, iterations: as pose_window_step takes them; C_start (4, 4) or (3, 4) world ->
    camera pose of frame 0, the identity if None."""

    def __init__(self, window=None, spacings=(1, 5, 10, 15, 20), capacity: int = 4096, min_inliers: int = 12, huber_chi: float = 4.0,
                 damping: float = 0.0, iterations: int = 2, C_start=None):
        from sslam_amd import window_numpy as wn
        from sslam_amd.online import _checked_spacings
        self.spacings = _checked_spacings(spacings, below=2 ** 31)
        self.window, _, self.capacity, _ = lib.check_window_sizes(max(self.spacings) + 1 if window is None else window, len(self.spacings), capacity)
        self.min_inliers = lib.check_int("min_inliers", min_inliers, 0, 2 ** 31 - 1)
        self.huber_chi, self.damping = lib.check_positive("huber_chi", huber_chi), lib.check_damping(damping)
        self.iterations = lib.check_graph_iterations(iterations)
        if C_start is not None:
            C_start = np.asarray(C_start, dtype=np.float64)
            if tuple(C_start.shape) not in ((4, 4), (3, 4)):
                raise ValueError(f"C_start (4, 4) or (3, 4) expected, got {C_start.shape}")
            C_start = np.ascontiguousarray(C_start[:3]).reshape(12)
        self.C_start, self._wn = C_start, wn
        self.reset()

    def reset(self) -> None:
        self.state = self._wn.fresh_state(self.window, len(self.spacings), self.capacity)

    def step(self, T, info, status, inlier_count) -> dict:
        """T (S, 4, 4) or (S, 3, 4): camera t - s -> camera t for every spacing, in their order; info (S, 6, 6): their information
        matrices; status, inlier_count (S,): the refinement's (a pair that does not exist yet: status 3).  Returns the entry's
        outputs by name (lib.WINDOW_OUT_KEYS) as numpy arrays: C_window (window, 12) world -> camera in node order, base, n_nodes,
        admitted (S,), predicted_from, lost, status, iterations, used_edges, dropped_edges, failed_row, cost_in, cost, edge_chi2."""
        S = len(self.spacings)
        T, info = np.asarray(T, dtype=np.float64), np.asarray(info, dtype=np.float64)
        status, inlier_count = np.asarray(status).reshape(-1), np.asarray(inlier_count).reshape(-1)
        if T.ndim != 3 or tuple(T.shape) not in ((S, 4, 4), (S, 3, 4)):
            raise ValueError(f"T ({S}, 4, 4) or ({S}, 3, 4) expected, got {T.shape}")
        if info.shape != (S, 6, 6):
            raise ValueError(f"info ({S}, 6, 6) expected, got {info.shape}")
        if len(status) != S or len(inlier_count) != S:
            raise ValueError(f"status and inlier_count ({S},) expected")
        iu = np.triu_indices(6)
        return self._wn.step(self.state, self.spacings, np.ascontiguousarray(T[:, :3]).reshape(S, 12), np.ascontiguousarray(info[:, iu[0], iu[1]]),
                             status, inlier_count, self.C_start, self.min_inliers, self.huber_chi, self.damping, self.iterations)

    def trajectory(self) -> np.ndarray:
        """Camera -> world poses (n, 4, 4) of the frames 0 .. min(frames stepped, capacity) - 1."""
        n = min(int(self.state["t"]), self.capacity)
        C = np.tile(np.eye(4), (n, 1, 1))
        C[:, :3] = self.state["trajectory"][:n].reshape(n, 3, 4)
        return np.stack([np.linalg.inv(c) for c in C]) if n else np.zeros((0, 4, 4))


class PlaceBank:
    """The online counterpart of find_loop_candidates: a place bank that grows by one frame per step (sslp_place_step,
    include/sslam_place.h) and answers, at every step, which older frames the new one resembles.  Like PoseWindow it needs NO GPU:
    it runs the header's statement in numpy float32 (sslam_amd/place_numpy.py) and gives the bits the device entry gives - a caller
    on the device uses SequencePipeline.place_step or online.LoopWindowPoseFrameStepper.
    capacity: 1 .. 4096 frames; d: the descriptor width, 128 or 256; min_gap, min_sim, per_frame, suppress: find_loop_candidates'."""

    def __init__(self, capacity: int = 1024, d: int = lib.D_OUT, min_gap: int = 30, min_sim: float = 0.3, per_frame: int = 2, suppress: int = 5):
        from sslam_amd import place_numpy as pn
        self.min_gap, self.min_sim, self.per_frame, self.suppress = lib.check_loop_arguments(min_gap, min_sim, per_frame, suppress)
        self.capacity, _, self.d = lib.check_place_sizes(capacity, 1, d)
        self._pn = pn
        self.reset()

    def reset(self) -> None:
        self.state = self._pn.fresh_place(self.capacity, self.d)

    def step(self, descriptors, scores) -> dict:
        """descriptors (K, d), scores (K,) float32 of one frame, K 1 .. 4096.  Returns the entry's outputs by name (lib.PLACE_OUT_KEYS)
        as numpy arrays: first, second (per_frame,) int32 - the older frame and this one, -1 in an empty slot -, sim, count (1,),
        status (1,): 0, or 4 once the bank is full, sig (d,): the frame's signature as of this step."""
        descriptors, scores = np.asarray(descriptors, dtype=np.float32), np.asarray(scores, dtype=np.float32)
        if descriptors.ndim != 2 or descriptors.shape[1] != self.d or scores.shape != descriptors.shape[:1]:
            raise ValueError(f"descriptors (K, {self.d}) and scores (K,) expected, got {descriptors.shape} and {scores.shape}")
        lib.check_place_sizes(self.capacity, int(descriptors.shape[0]), self.d)
        return self._pn.place_step(self.state, descriptors, scores, self.min_gap, self.min_sim, self.per_frame, self.suppress)


class EdgeLog:
    """The append-only list of verified edges optimize_pose_graph_sparse reads (sslp_edge_log_step, include/sslam_place.h), in numpy:
    per frame n_slots pairs, the first n_odometry of them odometry pairs held to min_inliers, the others loop candidates held to
    loop_min_inliers.  No GPU needed; the device entry's bits."""

    def __init__(self, capacity: int = 1024, n_slots: int = 7, n_odometry: int = 5, min_inliers: int = 12, loop_min_inliers: int = 12):
        from sslam_amd import place_numpy as pn
        self.capacity, self.n_slots = lib.check_edge_log_sizes(capacity, n_slots)
        self.n_odometry = lib.check_int("n_odometry", n_odometry, 0, self.n_slots)
        self.min_inliers = lib.check_int("min_inliers", min_inliers, 0, 2 ** 31 - 1)
        self.loop_min_inliers = lib.check_int("loop_min_inliers", loop_min_inliers, 0, 2 ** 31 - 1)
        self._pn = pn
        self.reset()

    def reset(self) -> None:
        self.state = self._pn.fresh_log(self.capacity, self.n_slots)

    def step(self, slot_first, T, info, status, inlier_count) -> dict:
        """slot_first (E,): the global index of every pair's older frame, -1 for none; T (E, 4, 4) or (E, 3, 4), info (E, 6, 6),
        status, inlier_count (E,): as refine_relative_pose returned them.  Returns logged (E,) int32 and status (1,)."""
        E = self.n_slots
        slot_first = np.asarray(slot_first).reshape(-1)
        T, info = np.asarray(T, dtype=np.float64), np.asarray(info, dtype=np.float64)
        status, inlier_count = np.asarray(status).reshape(-1), np.asarray(inlier_count).reshape(-1)
        if T.ndim != 3 or tuple(T.shape) not in ((E, 4, 4), (E, 3, 4)):
            raise ValueError(f"T ({E}, 4, 4) or ({E}, 3, 4) expected, got {T.shape}")
        if info.shape != (E, 6, 6):
            raise ValueError(f"info ({E}, 6, 6) expected, got {info.shape}")
        if len(slot_first) != E or len(status) != E or len(inlier_count) != E:
            raise ValueError(f"slot_first, status and inlier_count ({E},) expected")
        iu = np.triu_indices(6)
        return self._pn.log_step(self.state, slot_first, np.ascontiguousarray(T[:, :3]).reshape(E, 12), np.ascontiguousarray(info[:, iu[0], iu[1]]),
                                 status, inlier_count, self.n_odometry, self.min_inliers, self.loop_min_inliers)

    def edges(self) -> tuple:
        """(first, second, T (n E, 12), info (n E, 21)) of the n frames logged: optimize_pose_graph_sparse's edges in log order."""
        rows = min(int(self.state["t"]), self.capacity) * self.n_slots
        return tuple(self.state[k][:rows] for k in ("log_first", "log_second", "log_T", "log_info"))


def build_tracks(first, second, matches, count=None, mask=None, n_frames=None, k=None) -> dict:
    """Feature tracks from the match lists of a sequence's pairs, numpy in -> numpy out with NO GPU (sslam_amd/track_numpy.py: the
    statement of include/sslam_track.h, the bits sslt_link_pairs + sslt_track_ids give; a caller on the device uses
    SequencePipeline.link_matches / track_ids).  first, second (P,): the frames a < b of every row; matches (P, n1, 2) [idx1, idx2];
    count (P,): the listed slots of every row, all of them if None; mask (P, n1): where given only slots with mask == 1 count - the
    inlier_of_slot of estimate_relative_pose or refine_relative_pose.  Returns prev, next (n_frames, k), prev_frame, next_frame
    (n_frames,), track_id, age (n_frames, k), n_tracks (1,), root_frame, root_slot, length (n_frames * k,) int32: every keypoint has
    at most one predecessor and one successor, tracks are numbered by their first keypoint in (frame, slot) order, and a keypoint
    without a link is a track of length 1."""
    from sslam_amd import track_numpy as tn
    return tn.build_tracks(first, second, matches, count, mask, n_frames, k)


def track_landmarks(keypoints, kp_depth, C, tracks: dict, camera=None, threshold: float = 3.0, min_obs: int = 2, weights=None) -> dict:
    """The landmark map of build_tracks' tracks, numpy with NO GPU (the bits of sslt_landmarks): keypoints (N, K, 2) float32 pixels,
    kp_depth (N, K) int32 raw depths under them, C (N, 12) / (N, 3, 4) / (N, 4, 4) world -> camera poses, camera an
    sslam_amd.evaluation.Camera (TUM's if None), weights (N, K) float32 or None - UncertaintyEstimator's confidences as they are.
    Returns xyz (N K, 3), n_obs, n_kept, status, weight_sum, rms per track and residual, kept (N, K) per keypoint."""
    from sslam_amd import track_numpy as tn
    from sslam_amd.evaluation import Camera
    C = np.asarray(C, dtype=np.float64)
    if C.ndim == 3 and C.shape[1:] == (4, 4):
        C = C[:, :3]
    return tn.track_landmarks(keypoints, kp_depth, np.ascontiguousarray(C).reshape(len(C), 12), tracks, Camera() if camera is None else camera,
                              threshold, min_obs, weights)


class TrackBank:
    """The online counterpart of build_tracks: a track bank that grows by one frame per step (sslt_track_step,
    include/sslam_track.h).  Like PlaceBank it needs NO GPU: it runs the header's statement in numpy (sslam_amd/track_numpy.py) and
    gives the bits the device entry gives - a caller on the device uses SequencePipeline.track_step.  After n steps its rows equal
    build_tracks over the rows stepped so far.  capacity: the frames the bank keeps; k: keypoint slots per frame, 1 .. 4096."""

    def __init__(self, capacity: int = 1024, k: int = 500):
        from sslam_amd import track_numpy as tn
        self._bank = tn.TrackBank(capacity, k)
        self.capacity, self.k = self._bank.capacity, self._bank.k

    @property
    def state(self) -> dict:
        return self._bank.state

    def reset(self) -> None:
        self._bank.reset()

    def step(self, matches, *, first: int = -1, count=None, mask=None) -> dict:
        """matches (n1, 2) [idx1 in frame `first`, idx2 in this frame]; first: the bank frame the matches come from, -1 for none
        (the first frame); count: the listed slots, all if None; mask (n1,): only slots with mask == 1 count - all three by keyword: the
        numpy bank this wraps orders them otherwise.  Returns this frame's track_id, age (k,), n_new (1,) and status (1,): 0, or 4
        once the bank is full."""
        matches = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
        return self._bank.step(matches, len(matches) if count is None else int(count), None if mask is None else np.asarray(mask).reshape(-1),
                               int(first))

    def tracks(self) -> dict:
        return self._bank.tracks()


def find_loop_candidates(descriptors, scores, min_gap: int = 30, min_sim: float = 0.3, per_frame: int = 2, suppress: int = 5):
    """The step that proposes loop closures: descriptors (N, K, D) and scores (N, K) float32 of a sequence's frames, D 128 or 256.
    Every frame gets a place signature - the score-weighted sum of its descriptors, centred on the sequence's mean, normalised -
    and up to per_frame older frames j <= i - min_gap whose signature's similarity to its own is at least min_sim, best first, none
    within `suppress` frames of a better one (ssll_frame_signatures, ssll_loop_candidates; include/sslam_loop.h).
    numpy in, numpy out.  Returns (pairs (P, 2) int32 [older frame, frame], sim (P,) float32): the proposed pairs in frame order."""
    descriptors, scores = np.ascontiguousarray(descriptors, dtype=np.float32), np.ascontiguousarray(scores, dtype=np.float32)
    if descriptors.ndim != 3 or scores.shape != descriptors.shape[:2]:
        raise ValueError(f"descriptors (N, K, D) and scores (N, K) expected, got {descriptors.shape} and {scores.shape}")
    lib.check_width(int(descriptors.shape[2]))
    lib.check_loop_arguments(min_gap, min_sim, per_frame, suppress)
    sig = lib.frame_signatures(_dev(descriptors, torch.float32), _dev(scores, torch.float32))
    first, second, sim, _ = (t.cpu().numpy() for t in lib.loop_candidates(sig, min_gap, min_sim, per_frame, suppress))
    filled = first >= 0
    return np.stack([first[filled], second[filled]], axis=1), sim[filled]


def optimize_pose_graph_sparse(first, second, T, info, n_nodes: int, C_init, huber_chi: float = 4.0, damping: float = 0.0, iterations: int = 8,
                               cg_iterations: int = 512, cg_tol: float = 1e-3):
    """optimize_pose_graph with pairs anywhere - loop closures among them - solved by preconditioned conjugate gradients
    (ssll_pose_graph_sparse, include/sslam_loop.h).  first .. info: as optimize_pose_graph takes them; C_init (n_nodes, 4, 4) or
    (n_nodes, 3, 4) world -> camera is required (optimize_pose_graph's C, or a chain); cg_iterations: the most CG iterations of a
    step; cg_tol: their relative tolerance.  numpy in, numpy out; one graph.
    Returns (C (n_nodes, 4, 4), status, chi2 (E,), cg_steps (16,): the CG iterations every step took)."""
    first, second = [int(v) for v in np.asarray(first).reshape(-1)], [int(v) for v in np.asarray(second).reshape(-1)]
    T, info = np.asarray(T, dtype=np.float64), np.asarray(info, dtype=np.float64)
    if T.ndim != 3 or tuple(T.shape[1:]) not in ((4, 4), (3, 4)) or len(T) != len(first) or len(first) != len(second) or not first:
        raise ValueError(f"T (E, 4, 4) or (E, 3, 4) for E = {len(first)} >= 1 pairs expected, got {T.shape}")
    if info.shape != (len(first), 6, 6):
        raise ValueError(f"info ({len(first)}, 6, 6) expected, got {info.shape}")
    C_init = np.asarray(C_init, dtype=np.float64)
    if C_init.ndim != 3 or tuple(C_init.shape[1:]) not in ((4, 4), (3, 4)) or len(C_init) != n_nodes:
        raise ValueError(f"C_init ({n_nodes}, 4, 4) or ({n_nodes}, 3, 4) expected, got {C_init.shape}")
    lib.check_cg_iterations(cg_iterations), lib.check_cg_tol(cg_tol)
    from sslam_amd.pipeline import SequencePipeline
    iu = np.triu_indices(6)
    out = SequencePipeline.optimize_pose_graph_sparse(first, second, _dev(np.ascontiguousarray(T[:, :3]).reshape(-1, 12), torch.float64),
                                                      _dev(np.ascontiguousarray(info[:, iu[0], iu[1]]), torch.float64), n_nodes,
                                                      _dev(np.ascontiguousarray(C_init[:, :3]).reshape(n_nodes, 12), torch.float64), huber_chi,
                                                      damping, iterations, cg_iterations, cg_tol)
    C = np.tile(np.eye(4), (n_nodes, 1, 1))
    C[:, :3] = out["C"].cpu().numpy().reshape(n_nodes, 3, 4)
    return C, int(out["status"].cpu()), out["edge_chi2"].cpu().numpy(), out["cg_steps"].cpu().numpy()


def refine_keypoints_subcell(saliency, keypoints):
    """The step between the selector and everything geometric: saliency (G, G) fp32 - one frame's map - and keypoints (N, 2), the
    whole cells (x, y) in patch units that KeypointSelector.select_keypoints returned for it -> (N, 2) fp32 patch coordinates, each
    keypoint at the vertex of the per-axis parabola through its cell's saliency and the two neighbours' (sslx_subcell_keypoints,
    include/sslam_ext.h; DinoBackbone.patch_to_pixel takes the result to pixels as it takes the cells).  A border axis, a cell
    that is no maximum along an axis and a plateau keep the cell's coordinate.
    numpy in, numpy out: shapes and values are judged on the host before any device work, and a keypoint that is no whole cell
    of the grid is a ValueError.  Torch tensors in, a device tensor out: shapes are judged, nothing is read on the host and
    nothing but the result leaves the device - a keypoint that is no whole cell of the grid (outside it, fractional, NaN) then
    comes back as (0, 0), the entry's answer to an index out of range."""
    tensors = isinstance(saliency, torch.Tensor) or isinstance(keypoints, torch.Tensor)
    saliency = saliency if isinstance(saliency, torch.Tensor) else np.asarray(saliency)
    keypoints = keypoints if isinstance(keypoints, torch.Tensor) else np.asarray(keypoints)
    if tuple(saliency.shape) != (saliency.shape[0],) * 2 or saliency.shape[0] < 1:
        raise ValueError(f"saliency (G, G) expected, got {tuple(saliency.shape)}")
    if len(keypoints.shape) != 2 or keypoints.shape[1] != 2 or keypoints.shape[0] < 1:
        raise ValueError(f"keypoints (N >= 1, 2) expected, got {tuple(keypoints.shape)}")
    g = int(saliency.shape[0])
    if not tensors:
        kp = np.asarray(keypoints)
        cells = np.floor(kp)
        if not np.isfinite(kp).all() or (cells != kp).any() or (cells < 0).any() or (cells >= g).any():
            raise ValueError(f"keypoints must be whole cells of the {g} x {g} grid, as select_keypoints returns them")
    kp = _dev(keypoints, torch.float32)
    x, y = kp[:, 0], kp[:, 1]
    whole = (x >= 0) & (x < g) & (y >= 0) & (y < g) & (x == x.floor()) & (y == y.floor())       # false for a NaN
    cell = torch.where(whole, y, torch.zeros_like(y)).long() * g + torch.where(whole, x, torch.zeros_like(x)).long()
    idx = torch.where(whole, cell, torch.full_like(cell, -1)).to(torch.int32)
    out = lib.subcell_keypoints(_dev(saliency, torch.float32)[None], idx[None].contiguous())[0][0]
    return out if tensors else out.cpu().numpy()


def evaluate_matches(pred_matches, gt_matches, num_kpts1: int, num_kpts2: int) -> dict:
    """Predicted matches (P, 2) against ground-truth matches (G, 2).  Returns the original's dictionary: tp, fp, fn, precision,
    recall, f1, inlier_ratio, num_pred_matches, num_gt_matches.
    Both lists must hold every idx1 at most once, within [0, num_kpts1) - as every matcher here and
    compute_ground_truth_matches write them; the counts are then the sizes of the original's set intersection and differences."""
    n1 = int(num_kpts1)
    pm, gm = _dev(pred_matches, torch.int64).reshape(-1, 2), _dev(gt_matches, torch.int64).reshape(-1, 2)
    n_pred, n_gt = int(pm.shape[0]), int(gm.shape[0])
    if n1 < 1 or n_pred > n1 or n_gt > n1:
        raise ValueError(f"lists of {n_pred} and {n_gt} rows cannot hold every idx1 of {n1} keypoints at most once")
    dev = pm.device
    matches = torch.zeros((1, n1, 2), dtype=torch.int64, device=dev)
    matches[0, :n_pred] = pm
    gt_of_row = torch.full((1, n1), -1, dtype=torch.int32, device=dev)
    if n_gt:
        if int(gm[:, 0].min()) < 0 or int(gm[:, 0].max()) >= n1:
            raise ValueError(f"gt_matches names a keypoint outside [0, {n1})")
        gt_of_row[0, gm[:, 0]] = gm[:, 1].to(torch.int32)
    value = torch.zeros((1, n1), dtype=torch.float32, device=dev)
    count = torch.full((1,), n_pred, dtype=torch.int32, device=dev)
    gt_count = torch.full((1,), n_gt, dtype=torch.int32, device=dev)
    tp, fp, fn, _ = lib.match_score_pairs(matches, value, count, gt_of_row, gt_count)
    tp, fp, fn = torch.stack([tp, fp, fn]).reshape(3).tolist()
    return match_metrics(tp, fp, fn, n_pred, n_gt)
