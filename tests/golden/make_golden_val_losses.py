#!/usr/bin/env python3
"""Generate tests/golden/val_losses.npz by RUNNING the reference's own loss modules (losses.self_supervised) and the
trainer's matcher (train.SemanticSLAMTrainer._find_matches) the way _forward_pass wires them (train.py:331-406).

Runs only where the reference lies (like make_golden.py, whose importer it uses).  Arrays only: seeded inputs and the
reference's outputs, in fp32 as the trainer runs them and with the same modules cast to float64.

Cases (K = 37 descriptors per frame):
  g4  G = 4, B = 4, temperature 0.01, the second frame's descriptors are noisy copies of the first's: similarities above
      0.5, so the +-50 clamp of the logits is active
  g5  G = 5, B = 4, temperature 0.10, unrelated descriptors; the match counts of the four pairs differ, so the zero-padding of
      the match lists is exercised; two flat saliency maps (the variation branch of the sparsity term active)
For each case the outputs are stored for the batch of four AND for each pair alone (B = 1).
Every descriptor pair is tie-free in both arg-max directions; the smallest top-1 / top-2 gap is recorded.
The generator asserts that the reference's own fp32 result lies within a quarter of the tests' floor 2^-20 max(1, |value|) of
its float64 result for every stored scalar, and takes the next seed otherwise.

Usage:  python tests/golden/make_golden_val_losses.py
"""
from __future__ import annotations

import os

import numpy as np

import make_golden as mg

import torch  # noqa: E402

TERMS = ("desc", "variance", "repeat", "peakiness", "activation", "edge", "sparsity")
METRICS = ("num_matches", "mean_saliency", "max_saliency", "saliency_variance", "descriptor_variance")
ORDER = TERMS + ("total",) + METRICS
WEIGHTS = dict(desc=8.0, repeat=0.3, variance=0.5, peakiness=0.1, activation=0.05, edge=0.3, sparsity=0.3)   # train_config.yaml:53-60
K, D = 37, 128
FLOOR = 2.0 ** -20
MEAN = np.array([0.485, 0.456, 0.406], np.float32).reshape(1, 3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], np.float32).reshape(1, 3, 1, 1)


def normalise(u8: np.ndarray) -> np.ndarray:
    """(B, 3, S, S) uint8 -> the fp32 normalised image, one fp32 operation at a time (tests restate this line)."""
    return ((u8.astype(np.float32) / np.float32(255.0)) - MEAN) / STD


def unit(a):
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def inputs(seed: int, g: int, related: bool, flat: tuple = ()):
    rng = np.random.default_rng(seed)
    B, S = 4, 16 * g
    sal1 = rng.uniform(0.02, 0.98, (B, g, g)).astype(np.float32)
    sal2 = np.clip(sal1 + rng.normal(0, 0.1, (B, g, g)), 0.01, 0.99).astype(np.float32)
    for b in flat:
        sal1[b] = (0.3 + 0.05 * rng.uniform(0, 1, (g, g))).astype(np.float32)
    coarse = rng.uniform(0, 255, (B, 3, S // 8, S // 8))
    u8 = np.clip(np.kron(coarse, np.ones((8, 8))) + rng.normal(0, 12, (B, 3, S, S)), 0, 255).astype(np.uint8)
    d1 = unit(rng.normal(0, 1, (B, K, D)))
    if related:
        perm = np.stack([rng.permutation(K) for _ in range(B)])
        d2 = unit(np.take_along_axis(d1, perm[:, :, None], 1) + rng.normal(0, 0.035, (B, K, D)))
        for b in range(B):      # a few rows without a partner, so that the counts stay below K
            d2[b, : 2 + b] = unit(rng.normal(0, 1, (2 + b, D)))
    else:
        d2 = unit(rng.normal(0, 1, (B, K, D)))
    return sal1, sal2, u8, d1, d2


def min_gap(d1, d2) -> float:
    gap = np.inf
    for b in range(len(d1)):
        s = d1[b].astype(np.float64) @ d2[b].astype(np.float64).T
        for m in (s, s.T):
            top = np.sort(m, axis=1)
            gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
    return gap


def forward(M, sal1, sal2, img, d1, d2, temperature, dtype):
    """_forward_pass from the losses on (train.py:333-406), at `dtype`."""
    L = M["losses"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)      # noqa: E731
    s1, s2, im, a, b = t(sal1)[..., None], t(sal2)[..., None], t(img), t(d1), t(d2)
    matches = M["train"].SemanticSLAMTrainer._find_matches(None, a, b)
    out = dict(desc=L.DescriptorMatchingLoss(temperature=temperature)(a, b, matches), variance=L.DescriptorVarianceLoss(min_variance=0.005)(a),
               repeat=L.RepeatabilityLoss(2.0)(s1, s2), peakiness=L.PeakinessLoss(target_variance=0.22)(s1),
               activation=L.ActivationLoss(target_mean=0.35)(s1), edge=L.EdgeAwarenessLoss(0.1).to(dtype)(s1, im),
               sparsity=L.SpatialSparsityLoss(sparsity_target=0.35, penalty_weight=2.0)(s1))
    total = sum(WEIGHTS[k] * out[k] for k in ("desc", "variance", "repeat", "peakiness", "activation", "edge", "sparsity"))
    res = {k: float(v) for k, v in out.items()}
    res["total"] = float(total)
    sal_np, desc_np = s1.numpy(), a.numpy()
    res.update(num_matches=float(matches.shape[1]), mean_saliency=float(np.mean(sal_np)), max_saliency=float(np.max(sal_np)),
               saliency_variance=float(np.var(sal_np)), descriptor_variance=float(np.var(desc_np)))
    return np.array([res[k] for k in ORDER], np.float64), matches.numpy()


def counts(M, d1, d2):
    return [int(M["train"].SemanticSLAMTrainer._find_matches(None, torch.from_numpy(d1[b:b + 1]), torch.from_numpy(d2[b:b + 1])).shape[1])
            for b in range(len(d1))]


def case(M, name, g, temperature, related, flat, want_uneven, seed0):
    for seed in range(seed0, seed0 + 200):
        sal1, sal2, u8, d1, d2 = inputs(seed, g, related, flat)
        img = normalise(u8)
        gap = min_gap(d1, d2)
        n = counts(M, d1, d2)
        if gap < 1e-4 or (want_uneven and len(set(n)) < 3):
            continue
        r32, m32 = forward(M, sal1, sal2, img, d1, d2, temperature, torch.float32)
        r64, m64 = forward(M, sal1, sal2, img, d1, d2, temperature, torch.float64)
        one32, one64 = [], []
        same = np.array_equal(m32, m64)
        for b in range(4):
            sl = slice(b, b + 1)
            a32, ma = forward(M, sal1[sl], sal2[sl], img[sl], d1[sl], d2[sl], temperature, torch.float32)
            a64, mb = forward(M, sal1[sl], sal2[sl], img[sl], d1[sl], d2[sl], temperature, torch.float64)
            same = same and np.array_equal(ma, mb)
            one32.append(a32)
            one64.append(a64)
        one32, one64 = np.stack(one32), np.stack(one64)
        worst = max(float(np.max(np.abs(r32 - r64) / (FLOOR * np.maximum(1, np.abs(r64))))),
                    float(np.max(np.abs(one32 - one64) / (FLOOR * np.maximum(1, np.abs(one64))))))
        if not same or worst > 0.25:
            print(f"{name}: seed {seed} refused (matches agree: {same}, reference gap {worst:.3f} of the floor)")
            continue
        if related:
            x = np.einsum("bid,bjd->bij", d1.astype(np.float64), d2.astype(np.float64)) / temperature
            assert (x > 50).any(), "the clamp is meant to be active"
        print(f"{name}: seed {seed}, G {g}, T {temperature}, match counts {n}, min top-1/top-2 gap {gap:.3e}")
        for k, v32, v64 in zip(ORDER, r32, r64):
            print(f"    B=4 {k:20s} fp32 {v32:+.9e}  f64 {v64:+.9e}  gap {abs(v32 - v64):.2e}")
        print(f"    largest gap over B=4 and the four B=1 rows: {worst:.3f} of the floor")
        return {f"{name}_sal1": sal1, f"{name}_sal2": sal2, f"{name}_u8": u8, f"{name}_d1": d1, f"{name}_d2": d2,
                f"{name}_temperature": np.float64(temperature), f"{name}_counts": np.array(n, np.int32),
                f"{name}_ref32_b4": r32, f"{name}_ref64_b4": r64, f"{name}_ref32_b1": one32, f"{name}_ref64_b1": one64,
                f"{name}_gap_b4": np.abs(r32 - r64), f"{name}_gap_b1": np.abs(one32 - one64), f"{name}_min_gap": np.float64(gap),
                f"{name}_seed": np.int64(seed)}
    raise SystemExit(f"{name}: no seed passed")


def main():
    M = mg._import_reference()
    import losses.self_supervised as L
    M["losses"] = L
    out = {"order": np.array(ORDER)}
    out.update(case(M, "g4", 4, 0.01, True, (), False, 100))
    out.update(case(M, "g5", 5, 0.10, False, (1, 3), True, 200))
    path = os.path.join(mg.HERE, "val_losses.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
