#!/usr/bin/env python3
"""Generate tests/golden/pose_eval.npz by RUNNING the reference's own pose-based scoring code (authoring container only: needs
/root/reference).  The fixture holds arrays only - seeded inputs and what the reference returned; no reference source is stored.

What is driven, imported where it lies with the inert placeholders of make_golden.py (timm / torchvision / cv2 / wandb):
  * test_repeatability.RepeatabilityTester.compute_repeatability            (:79-128), called unbound
  * test_descriptor_quality.DescriptorQualityTester.compute_ground_truth_matches, .evaluate_matches and
    .find_mutual_nearest_neighbors                                          (:97-231), called unbound
  * both classes' test_sequence (:130-215, :233-305) on objects built without __init__ (which loads a checkpoint and the
    third-party ViT): the module's TUMDataset is replaced by a stand-in that yields rgb1 / rgb2 (a frame number each) and
    relative_pose = pose2 @ inv(pose1) as a float tensor (data/tum_dataset.py:191-195), and detect_keypoints / extract_features
    hand back the preset keypoints and descriptors of that frame - the technique of run_reference_scripts.py.

Inputs: keypoint banks from the CPU oracle's selector (G = 28 / 40 / 60: these hold duplicates), lattice samples at
K in {1, 2, 3, 63, 64, 65, 127, 129}, free float32 coordinates; homographies None, K I K^-1 as the product comes out, small rotations, one
half-cell rotation that leaves nothing within 3 px, one H whose third row is exactly 0 at one keypoint; thresholds 3, 0 and 1e9;
pair lists with an absent row, a repeated frame and a self pair; predicted lists from the reference's M4, an empty one and one
equal to the ground truth.

EVERY kept case satisfies, in float64: min |dist - threshold| >= 1e-6 px, and for rows inside the threshold the nearest point at
another location is >= 1e-6 px farther (pose_eval_ref.margins).  A seed that does not pass is replaced HERE (the loop in
`seeded`), never filtered in a test.

Usage:  python tests/golden/make_golden_pose_eval.py [OUT.npz]        (default: pose_eval.npz next to this file)
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [TESTS, ROOT]
sys.dont_write_bytecode = True
REF = "/root/reference/semantic-slam"
MARGIN = 1e-6

import torch  # noqa: E402

import pose_eval_ref as pr  # noqa: E402
import synth  # noqa: E402
from oracle import ora  # noqa: E402

TUM_K = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])


def import_reference():
    for name in ["timm", "torchvision", "torchvision.transforms", "cv2", "wandb"]:
        sys.modules.setdefault(name, types.ModuleType(name))
    tv = sys.modules["torchvision.transforms"]
    for attr in ["Compose", "Resize", "ToTensor", "Normalize", "ColorJitter", "GaussianBlur", "RandomApply", "functional"]:
        if not hasattr(tv, attr):
            setattr(tv, attr, object)
    sys.modules["torchvision"].transforms = tv
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "test"))
    import test_descriptor_quality as tdq
    import test_repeatability as trep
    for mod in (tdq, trep):
        assert os.path.realpath(mod.__file__).startswith("/root/reference/"), mod.__file__
    return trep, tdq


# ------------------------------------------------------------------------------------------------------------------ inputs
def rotation(rng, sigma) -> np.ndarray:
    """A float32 rotation (what a relative pose hands over) by a rotation vector of N(0, sigma) components."""
    v = rng.normal(0.0, sigma, 3) if np.isscalar(sigma) else np.asarray(sigma, dtype=np.float64)
    t = np.linalg.norm(v)
    k = v / t
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx).astype(np.float32)


def K_H(R):
    return TUM_K @ R @ np.linalg.inv(TUM_K)                       # test_repeatability.py:192


def selector_bank(grid: int, k: int, frames: int = 3):
    toks = synth.token_sequence(frames, grid)
    feat = ora.bn_tokens(toks)[0].reshape(frames, grid, grid, 384)
    sal = ora.selector_saliency(feat, synth.selector_state(0))
    kp, sc, _, _ = ora.select_keypoints(sal, k)
    desc = ora.refine(ora.gather(feat, kp), synth.refiner_state(0))
    return ora.patch_to_pixel(kp), desc, sc


def lattice_bank(rng, k: int):
    cells = rng.permutation(28 * 28)[:k]                          # frame 0: distinct cells
    other = np.where(rng.random(k) < 0.6, cells, rng.integers(0, 28 * 28, k))      # frame 1: most of them again, some twice
    other = rng.permutation(other)
    to_px = lambda c: np.stack([16.0 * (c % 28) + 8.0, 16.0 * (c // 28) + 8.0], axis=1).astype(np.float32)
    return np.stack([to_px(cells), to_px(other)])


def ok(bank, first, second, H, thr) -> bool:
    for p, (a, b) in enumerate(zip(first, second)):
        if a < 0 or b < 0:
            continue
        edge, gap = pr.margins(bank[a], bank[b], None if H is None else H[p], thr)
        if not (edge >= MARGIN and gap >= MARGIN):
            return False
    return True


def seeded(make, base_seed: int):
    """make(rng) -> (case, passes): the first seed from base_seed on whose case passes the margin condition."""
    for seed in range(base_seed, base_seed + 100):
        case, passes = make(np.random.default_rng(seed))
        if passes:
            if seed != base_seed:
                print(f"  seed {base_seed} replaced by {seed}")
            return case
    raise RuntimeError(f"no passing seed from {base_seed}")


# --------------------------------------------------------------------------------------------------------------- reference
def reference_group(trep, tdq, out, name, bank_name, bank, first, second, H, thr, lists=None):
    """Run the reference per pair and store the group.  lists: per pair None | (pred (c, 2), values (c,)) | 'gt' | 'empty'."""
    P, k = len(first), bank.shape[1]
    cnt, mean, med, rep = np.zeros(P, np.int32), np.zeros(P), np.zeros(P), np.zeros(P)
    gt = np.zeros((P, k, 2), np.int16)
    pred, pc, pv, metrics = np.zeros((P, k, 2), np.int16), np.zeros(P, np.int32), np.zeros((P, k), np.float32), np.zeros((P, 9))
    for p, (a, b) in enumerate(zip(first, second)):
        if a < 0 or b < 0:
            continue
        h = None if H is None else H[p].reshape(3, 3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                        # the W = 0 case divides by zero, as it must
            r = trep.RepeatabilityTester.compute_repeatability(None, bank[a], bank[b], h, thr)
            g = None if h is None else tdq.DescriptorQualityTester.compute_ground_truth_matches(None, bank[a], bank[b], h, thr)
        cnt[p], mean[p], med[p], rep[p] = r["repeatable_count"], r["mean_nn_distance"], r["median_nn_distance"], r["repeatability"]
        assert r["total_keypoints"] == k
        if g is not None:
            assert len(g) == cnt[p]
            gt[p, :len(g)] = g
        if lists is not None and lists[p] is not None:
            assert g is not None
            if isinstance(lists[p], str):
                pm = g if lists[p] == "gt" else np.zeros((0, 2), np.int64)
                vals = np.zeros(len(pm), np.float32)
            else:
                pm, vals = lists[p]
            m = tdq.DescriptorQualityTester.evaluate_matches(None, pm, g, k, k)
            pred[p, :len(pm)], pc[p], pv[p, :len(pm)] = pm, len(pm), vals
            metrics[p] = [m[key] for key in pr.METRIC_KEYS]
    out[name + "_bank"] = np.array(bank_name)
    out[name + "_first"], out[name + "_second"] = np.asarray(first, np.int32), np.asarray(second, np.int32)
    out[name + "_H"] = np.zeros(0) if H is None else np.asarray(H, np.float64).reshape(P, 9)
    out[name + "_thr"] = np.float64(thr)
    out[name + "_count"], out[name + "_mean"], out[name + "_median"], out[name + "_rep"] = cnt, mean, med, rep
    if H is not None:
        out[name + "_gt"] = gt
    if lists is not None:
        out[name + "_pred"], out[name + "_pred_count"], out[name + "_pred_value"], out[name + "_metrics"] = pred, pc, pv, metrics
    out.setdefault("groups", []).append(name)
    print(f"  {name}: bank {bank_name}, {P} pairs, thr {thr:g}, counts {cnt.tolist()}")


def m4_lists(tdq, desc, first, second, kinds):
    """kinds[p]: 'm4' -> the reference's M4 on the pair's descriptors; 'gt' / 'empty' / None pass through."""
    out = []
    for a, b, kind in zip(first, second, kinds):
        if kind == "m4":
            pm, dist = tdq.DescriptorQualityTester.find_mutual_nearest_neighbors(None, desc[a], desc[b])
            mine, _ = ora.find_mnn_m4(desc[a], desc[b])
            assert np.array_equal(pm, mine), "the reference's M4 and the canonical-order M4 differ on this seed: choose another"
            out.append((pm, dist.astype(np.float32)))
        else:
            out.append(kind)
    return out


class PresetDataset:
    """Stand-in for data.tum_dataset.TUMDataset inside the two test modules: frame numbers for images, the relative pose as the
    loader forms it (tum_dataset.py:191, :195)."""
    poses, n_frames = None, 0

    def __init__(self, dataset_root=None, sequence=None, input_size=None, frame_spacing=1, max_frames=None, augmentation=None,
                 is_train=False):
        self.sp = frame_spacing
        self.n = PresetDataset.n_frames if max_frames is None else min(PresetDataset.n_frames, max_frames)

    def __len__(self):
        return max(0, self.n - self.sp)

    def __getitem__(self, idx):
        out = {"rgb1": torch.tensor([float(idx)]), "rgb2": torch.tensor([float(idx + self.sp)])}
        if PresetDataset.poses is not None:
            pose1, pose2 = PresetDataset.poses[idx], PresetDataset.poses[idx + self.sp]
            out["relative_pose"] = torch.from_numpy(pose2 @ np.linalg.inv(pose1)).float()
        return out


def reference_sequences(trep, tdq, out):
    kp, desc, sc = selector_bank(pr.SEQ_GRID, pr.SEQ_K, pr.SEQ_FRAMES)
    cfg = {"dataset": {"root": ""}, "model": {"input_size": 16 * pr.SEQ_GRID, "num_keypoints": pr.SEQ_K}}
    frame = lambda image: int(image.flatten()[0])
    rt = trep.RepeatabilityTester.__new__(trep.RepeatabilityTester)
    rt.device, rt.config = torch.device("cpu"), cfg
    rt.detect_keypoints = lambda image: (kp[frame(image)], sc[frame(image)])
    dq = tdq.DescriptorQualityTester.__new__(tdq.DescriptorQualityTester)
    dq.device, dq.config = torch.device("cpu"), cfg
    dq.extract_features = lambda image: (kp[frame(image)], desc[frame(image)], sc[frame(image)])
    trep.TUMDataset = tdq.TUMDataset = PresetDataset
    PresetDataset.n_frames = pr.SEQ_FRAMES
    runs = [("seq_s1", 1, 50, True), ("seq_s5", 5, 50, True), ("seq_s5_n4", 5, 4, True), ("seq_s1_raw", 1, 50, False)]

    def make(rng):
        poses = np.zeros((pr.SEQ_FRAMES, 4, 4))
        R = np.eye(3)
        for i in range(pr.SEQ_FRAMES):
            R = rotation(rng, 0.004).astype(np.float64) @ R
            poses[i, :3, :3], poses[i, :3, 3], poses[i, 3, 3] = R, rng.normal(0, 0.05, 3), 1.0
        passes = True
        for sp in (1, 5):
            first = list(range(pr.SEQ_FRAMES - sp))
            H = np.stack([K_H((poses[i + sp] @ np.linalg.inv(poses[i])).astype(np.float32)[:3, :3]) for i in first])
            passes = passes and ok(kp, first, [i + sp for i in first], H, 3.0) and ok(kp, first, [i + sp for i in first], None, 3.0)
            for i in first:                                        # the end-to-end tests match on the device in canonical order
                pm, _ = tdq.DescriptorQualityTester.find_mutual_nearest_neighbors(None, desc[i], desc[i + sp])
                passes = passes and np.array_equal(pm, ora.find_mnn_m4(desc[i], desc[i + sp])[0])
        return poses, passes

    poses = seeded(make, 700)
    out["seq_poses"] = poses
    for name, sp, num_pairs, use_pose in runs:
        PresetDataset.poses = poses
        r = rt.test_sequence("synthetic", num_pairs=num_pairs, frame_spacing=sp, use_pose=use_pose)
        out[name + "_spacing"], out[name + "_num_pairs"], out[name + "_use_pose"] = np.int64(sp), np.int64(num_pairs), np.bool_(use_pose)
        out[name + "_rep_summary"], out[name + "_rep_results"] = pr.summary_rows(r, pr.REP_SUMMARY_KEYS, pr.REP_RESULT_KEYS)
        if use_pose:
            q = dq.test_sequence("synthetic", num_pairs=num_pairs, frame_spacing=sp)
            out[name + "_dq_summary"], out[name + "_dq_results"] = pr.summary_rows(q, pr.DQ_SUMMARY_KEYS, pr.DQ_RESULT_KEYS)
        out.setdefault("sequences", []).append(name)
        print(f"  {name}: {r['num_pairs']} pairs, mean repeatability {r['mean_repeatability']:.4f}" +
              (f", mean precision {q['mean_precision']:.4f}, mean matches {q['mean_num_matches']:.1f}" if use_pose else ""))


def reference_dropins(trep, tdq, out):
    def free(rng, n, m, with_h):
        k1 = rng.uniform(0, 448, (n, 2)).astype(np.float32)
        H = K_H(rotation(rng, 0.02)) if with_h else None
        w = pr.warp(k1, None if H is None else H.reshape(9))
        take = rng.permutation(n)[:m] if m <= n else rng.integers(0, n, m)
        k2 = (w[take] + np.where(rng.random((m, 1)) < 0.6, rng.normal(0, 1.2, (m, 2)), rng.normal(0, 30, (m, 2)))).astype(np.float32)
        edge, gap = pr.margins(k1, k2, None if H is None else H.reshape(9), 3.0)
        return (k1, k2, H), edge >= MARGIN and gap >= MARGIN

    for name, seed, n, m, with_h in (("drop65", 900, 65, 50, True), ("drop65_raw", 910, 65, 65, False), ("drop500", 920, 500, 437, True),
                                     ("drop50_65", 930, 50, 65, True)):
        k1, k2, H = seeded(lambda rng: free(rng, n, m, with_h), seed)
        r = trep.RepeatabilityTester.compute_repeatability(None, k1, k2, H, 3.0)
        out[name + "_kp1"], out[name + "_kp2"], out[name + "_thr"] = k1, k2, np.float64(3.0)
        out[name + "_H"] = np.zeros(0) if H is None else H.reshape(9)
        out[name + "_rep"] = np.array([r[key] for key in pr.REP_RESULT_KEYS], dtype=np.float64)
        if H is not None:
            out[name + "_gt"] = tdq.DescriptorQualityTester.compute_ground_truth_matches(None, k1, k2, H, 3.0).astype(np.int16)
        out.setdefault("dropins", []).append(name)
        print(f"  {name}: {n} x {m}, repeatable {r['repeatable_count']}")


def main():
    if not os.path.isdir(REF):
        print("make_golden_pose_eval.py: /root/reference is absent (the fixtures are generated in the authoring container only)")
        return 77
    trep, tdq = import_reference()
    out = {}
    lists3 = ["m4", "m4", None, "empty", "gt", "m4"]
    first, second = [0, 1, -1, 0, 2, 1], [1, 2, 1, 1, 2, 0]          # an absent row, frame 1 four times, a repeated pair, a self pair
    for grid, k in ((28, 500), (40, 1024), (60, 2048)):
        kp, desc, _ = selector_bank(grid, k)
        bn = f"g{grid}"
        out["bank_" + bn] = kp
        f, s, kinds = (first, second, lists3) if grid != 60 else (first[:3], second[:3], lists3[:3])
        P = len(f)
        ident = np.stack([K_H(np.eye(3, dtype=np.float32))] * P)
        assert ok(kp, f, s, None, 3.0) and ok(kp, f, s, ident, 3.0)
        reference_group(trep, tdq, out, f"{bn}_raw", bn, kp, f, s, None, 3.0)
        reference_group(trep, tdq, out, f"{bn}_ident", bn, kp, f, s, ident, 3.0, m4_lists(tdq, desc, f, s, kinds))

        def rot_case(rng, thr=3.0, sig=(0.002, 0.02, 0.05)):
            H = np.stack([K_H(rotation(rng, sig[p % len(sig)])) for p in range(P)])
            return H, ok(kp, f, s, H, thr)
        H = seeded(rot_case, 100 + grid)
        reference_group(trep, tdq, out, f"{bn}_rot", bn, kp, f, s, H, 3.0, m4_lists(tdq, desc, f, s, kinds))
        if grid == 28:
            for tag, thr, seed in (("thr0", 0.0, 200), ("thrbig", 1e9, 210)):
                H = seeded(lambda rng: rot_case(rng, thr, (0.002, 0.02)), seed)
                reference_group(trep, tdq, out, f"{bn}_{tag}", bn, kp, f, s, H, thr, m4_lists(tdq, desc, f, s, kinds))
            # half a cell (8 px = 525 * 0.01524 rad) along both axes: every warped point lies between the lattice points
            far = np.stack([K_H(rotation(None, (0.01524, -0.01524, 0.0)))] * P)
            assert ok(kp, f, s, far, 3.0)
            reference_group(trep, tdq, out, f"{bn}_far", bn, kp, f, s, far, 3.0, m4_lists(tdq, desc, f, s, kinds))
            assert not out[f"{bn}_far_count"].any(), "the large rotation must leave no point within the threshold"

    lf, ls = [0, 1, 0, -1], [1, 0, 0, 0]
    for k in (1, 2, 3, 63, 64, 65, 127, 129):
        def lat_case(rng):
            bank = lattice_bank(rng, k)
            H = np.stack([K_H(rotation(rng, 0.004)) for _ in lf])
            return (bank, H), ok(bank, lf, ls, H, 3.0) and ok(bank, lf, ls, None, 3.0)
        bank, H = seeded(lat_case, 300 + k)
        bn = f"lat{k}"
        out["bank_" + bn] = bank
        lists = None
        if k >= 2:
            d = np.stack([synth.unit_descriptors(k, k), synth.descriptor_pair(k, k, k, 0)[1]])
            lists = m4_lists(tdq, d, lf, ls, ["m4", "gt", "empty", None])
        reference_group(trep, tdq, out, f"{bn}_rot", bn, bank, lf, ls, H, 3.0, lists)
        reference_group(trep, tdq, out, f"{bn}_raw", bn, bank, lf, ls, None, 3.0)

    # W = 0 at exactly one keypoint of frame 0 (distinct cells): h6 = 2^-10, h7 = 2^-17, h8 = -(h6 x0 + h7 y0), all exact
    bank = out["bank_lat65"]
    x0, y0 = (float(v) for v in bank[0, 7])
    H = K_H(rotation(np.random.default_rng(400), 0.02))
    H[2] = [2.0 ** -10, 2.0 ** -17, -(2.0 ** -10 * x0 + 2.0 ** -17 * y0)]
    w = (H[2, 0] * bank[0, :, 0].astype(np.float64) + H[2, 1] * bank[0, :, 1]) + H[2, 2]
    assert (w == 0).sum() == 1 and w[7] == 0
    Hs = np.stack([H, H])
    assert ok(bank, [0, 0], [1, 0], Hs, 3.0)
    reference_group(trep, tdq, out, "lat65_w0", "lat65", bank, [0, 0], [1, 0], Hs, 3.0, ["gt", "empty"])
    assert np.isinf(out["lat65_w0_mean"]).all()

    reference_dropins(trep, tdq, out)
    reference_sequences(trep, tdq, out)
    for key in ("groups", "dropins", "sequences"):
        out[key] = np.array(out[key])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pose_eval.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out['groups'])} groups, {len(out['dropins'])} drop-in cases, "
          f"{len(out['sequences'])} sequence runs")
    return 0


if __name__ == "__main__":
    sys.exit(main())
