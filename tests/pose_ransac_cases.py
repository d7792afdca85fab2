"""Seeded case lists for sslam_pose_ransac_pairs (tests/test_pose_ransac_cpu.py, tests/test_gpu_pose_ransac.py).

Planted geometry: frame a's keypoints are fp32, its raw depths integers (0.5 - 5 m); a rigid motion takes the back-projected points
to camera b; frame b's keypoints are the projections rounded to fp32 and its depths Z' rounded to the depth quantum (1 / 5000 m),
stored under a permutation that the match list follows; a stated share of the rows is then replaced by outliers (a random keypoint
and depth in frame b).  Every pair has its own two frames of the bank.

Every case is built so that the restatement of tests/pose_ransac_ref.py stays MARGIN = 1e-6 (px, or m for Z') clear of each
decision it takes - no distance of any hypothesis or of the refit within MARGIN of the threshold, no |Z'| under MARGIN - and a
seed that does not is replaced by the next one (check_margins() is what the builders hold a draw to and what the CPU test asserts
again).  Cases are built once per process (lru_cache) and never modified by a test.

Recovery of the planted motion by the RESTATEMENT (tests/test_pose_ransac_cpu.py measures it on the CPU over every pair flagged
`recover`: at most 30 % outliers, 40 usable rows at least): the largest rotation error is 0.00060 degrees and the largest
translation error 4.3e-5 m - what the depth quantum and the fp32 rounding of frame b's keypoints leave; the test asserts twice
those figures, RECOVER_DEG and RECOVER_M.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import pose_ransac_ref as rr

MARGIN = 1e-6
CAM = rr.Cam()
SCALE_448 = (640 / 448, 480 / 448)      # a 448-pixel pipeline's keypoints on a 640 x 480 depth image
RECOVER_DEG, RECOVER_M = 2 * 0.00060, 2 * 4.3e-5
SEEDS = (0, 0xdeadbeefcafef00d)         # the sampler's seeds: the second has its high bits set

IDENT = rr.rigid(np.eye(3), [0.0, 0.0, 0.0])


def _motion(rng, kind):
    if kind == "translation":
        return rr.rigid(np.eye(3), [0.08, -0.03, 0.05])
    if kind == "rotation":
        return rr.rigid(rr.rotation([0.3, 1.0, -0.2], np.deg2rad(4.0)), [0.0, 0.0, 0.0])
    return rr.rigid(rr.rotation(rng.normal(size=3), np.deg2rad(rng.uniform(1.0, 5.0))), rng.uniform(-0.08, 0.08, 3))


def _pair(rng, k, n1, scale, kind="general", outliers=0.3, count=None, dup=False, bad_idx=False, usable=None, holes=False):
    """One pair's two frames, its list and its planted motion."""
    sx, sy = scale
    cam = CAM
    a = np.stack([rng.uniform(30, cam.width - 30, k) / sx, rng.uniform(30, cam.height - 30, k) / sy], axis=1).astype(np.float32)
    da = rng.integers(2500, 25000, k).astype(np.int32)
    if dup:                                              # coincident points: a sample of three of them is degenerate
        a[k // 2:], da[k // 2:] = a[0], da[0]
    T = _motion(rng, kind)
    m = T.reshape(3, 4)
    Xb = rr.back_project(a, da, cam, sx, sy) @ m[:, :3].T + m[:, 3]
    kb = np.stack([(cam.fx * Xb[:, 0] / Xb[:, 2] + cam.cx) / sx, (cam.fy * Xb[:, 1] / Xb[:, 2] + cam.cy) / sy], axis=1).astype(np.float32)
    db = np.rint(Xb[:, 2] * cam.depth_scale).astype(np.int32)
    out = rng.random(k) < outliers
    kb[out] = np.stack([rng.uniform(0, cam.width, k) / sx, rng.uniform(0, cam.height, k) / sy], axis=1).astype(np.float32)[out]
    db[out] = rng.integers(2500, 25000, k)[out]
    if holes and k >= 64:                                # no measurement, outside the depth image
        da[5], db[9], da[17] = 0, -1, -1
    perm = rng.permutation(k)
    b, depth_b = np.empty_like(kb), np.empty_like(db)
    b[perm], depth_b[perm] = kb, db
    idx1 = np.sort(rng.permutation(k)[:n1])
    matches = np.stack([idx1, perm[idx1]], axis=1).astype(np.int64)
    if bad_idx and n1 >= 8:
        matches[1, 0], matches[2, 1], matches[4, 0], matches[6, 1] = -1, k, 1 << 40, -(1 << 35)
    count = n1 if count is None else count
    if usable is not None:                               # exactly `usable` usable rows among the listed ones
        listed = idx1[:max(0, min(count, n1))]
        da[listed[usable:]] = 0
    return dict(a=a, b=b, da=da, db=depth_b, matches=matches, count=count, T=T,
                recover=outliers <= 0.3 and not dup and not bad_idx and usable is None and min(count, n1) >= 40)


def _case(name, k, n1, specs, n_hyp, scale, rng_seed, threshold=3.0):
    """specs: per pair None (an ABSENT pair) or the keyword arguments of _pair."""
    rng = np.random.default_rng(rng_seed)
    bank, depth_bank, first, second, matches, count, planted, recover = [], [], [], [], [], [], [], []
    for spec in specs:
        if spec is None:
            first.append(-1 if len(first) % 2 else len(specs) * 2 + 5)      # -1 and an index past the bank
            second.append(0)
            matches.append(rng.integers(0, k, (n1, 2)).astype(np.int64))    # a list is there all the same: it must not be read as a pose
            count.append(n1)
            planted.append(IDENT)
            recover.append(False)
            continue
        p = _pair(rng, k, n1, scale, **spec)
        first.append(len(bank))
        second.append(len(bank) + 1)
        bank += [p["a"], p["b"]]
        depth_bank += [p["da"], p["db"]]
        matches.append(p["matches"])
        count.append(p["count"])
        planted.append(p["T"])
        recover.append(p["recover"])
    return dict(name=name, bank=np.stack(bank), depth_bank=np.stack(depth_bank), first=np.array(first, np.int32),
                second=np.array(second, np.int32), matches=np.stack(matches), count=np.array(count, np.int32), cam=CAM,
                scale_x=scale[0], scale_y=scale[1], threshold=threshold, n_hyp=n_hyp, planted=np.stack(planted), recover=recover, n1=n1)


def _specs_70(k):
    """70 pairs of K = 64: every kind of list."""
    s = []
    for p in range(70):
        if p in (1, 30, 68):
            s.append(None)                               # absent pairs between present ones
        elif p == 2:
            s.append(dict(outliers=1.0))                 # all outliers
        elif p == 3:
            s.append(dict(count=0))
        elif p == 4:
            s.append(dict(count=-7))
        elif p == 5:
            s.append(dict(count=k + 9))                  # clamped to n1
        elif p == 6:
            s.append(dict(bad_idx=True, holes=True))
        elif p == 7:
            s.append(dict(usable=2))
        elif p == 8:
            s.append(dict(usable=3))
        elif p == 9:
            s.append(dict(dup=True, outliers=0.2))
        elif p == 10:
            s.append(dict(kind="translation", outliers=0.0))
        elif p == 11:
            s.append(dict(kind="rotation", outliers=0.0))
        else:
            s.append(dict(outliers=(0.0, 0.3, 0.6, 0.9)[p % 4], count=(k, 41, k, 50)[p % 4], holes=p % 3 == 0))
    return s


# name -> (K, n1, specs, n_hyp, scale[, threshold = 3.0]).  n1 = K except in k300_n257.
CASES = {
    "k3": (3, 3, [dict(outliers=0.0), dict(usable=2, outliers=0.0), None, dict(outliers=1.0)], 1, (1.0, 1.0)),
    "k5_dup": (5, 5, [dict(dup=True, outliers=0.0), dict(outliers=0.0), dict(count=4, outliers=0.2)], 63, SCALE_448),
    "k64_p70": (64, 64, _specs_70(64), 64, (1.0, 1.0)),
    "k257": (257, 257, [dict(), None, dict(outliers=0.6, holes=True, bad_idx=True)], 65, SCALE_448),
    "k300_n257": (300, 257, [dict(kind="translation"), dict(kind="rotation"), dict(count=200, holes=True)], 256, (1.0, 1.0)),
    "k1024": (1024, 1024, [dict(outliers=0.5, holes=True)], 256, SCALE_448),
    "k1025": (1025, 1025, [dict(outliers=0.02), dict(count=1024, holes=True), dict(outliers=0.8)], 1024, (1.0, 1.0)),
    "k4096": (4096, 4096, [dict(outliers=0.05, holes=True)], 256, SCALE_448),
    # nothing but outliers under a loose threshold: hypotheses with a handful of chance inliers, whose refit may lose some of them
    "k64_loose": (64, 64, [dict(outliers=1.0)] * 6, 256, (1.0, 1.0), 40.0),
}
NAMES = tuple(CASES)


def present(c, p) -> bool:
    return 0 <= c["first"][p] < len(c["bank"]) and 0 <= c["second"][p] < len(c["bank"])


def check_margins(c, seed=SEEDS[0]) -> dict:
    """The least margins over the present pairs of a case (keys of pose_ransac_ref.margins)."""
    least = dict(edge=np.inf, z=np.inf)
    for p in range(len(c["first"])):
        if not present(c, p):
            continue
        a, b = c["first"][p], c["second"][p]
        m = rr.margins(c["bank"][a], c["bank"][b], c["depth_bank"][a], c["depth_bank"][b], c["matches"][p], c["count"][p], c["cam"],
                       c["threshold"], c["n_hyp"], seed, c["scale_x"], c["scale_y"])
        least = {key: min(least[key], m[key]) for key in least}
    return least


def margins_ok(m) -> bool:
    return all(v >= MARGIN for v in m.values())


def seeds_of(name) -> tuple:
    """The sampler's seeds a case is run under: both for the 70-pair case, the first elsewhere."""
    return SEEDS if name == "k64_p70" else SEEDS[:1]


@lru_cache(maxsize=None)
def case(name: str):
    k, n1, specs, n_hyp, scale = CASES[name][:5]
    rng_seed = 5000 + NAMES.index(name)
    while True:
        c = _case(name, k, n1, specs, n_hyp, scale, rng_seed, *CASES[name][5:])
        if all(margins_ok(check_margins(c, s)) for s in seeds_of(name)):
            return c
        rng_seed += 100


@lru_cache(maxsize=None)
def expected(name: str, seed: int):
    """The restatement's outputs for a case under a sampler seed, as the arrays the device writes (computed once per process)."""
    c = case(name)
    return rr.stacked(rr.ransac_pairs(c["bank"], c["depth_bank"], c["first"], c["second"], c["matches"], c["count"], c["cam"], c["threshold"],
                                      c["n_hyp"], seed, c["scale_x"], c["scale_y"]))
