"""Seeded case lists for the depth ground truth of the scoring stage (tests/test_pose_depth_cpu.py, tests/test_gpu_pose_depth.py).

Every case is built so that the restatement of tests/pose_depth_ref.py itself stays clear of each decision it takes - MARGIN =
1e-6 (px, or m for Z') - and a seed that does not is replaced by the next one:
  no nearest / second-nearest gap under MARGIN except exact duplicates;   no distance within MARGIN of the threshold;
  no u + 0.5 within MARGIN of an integer except the deliberately exact cases (their rows are listed in `exact`);
  no |Z'| under MARGIN;   no projection within MARGIN of a view edge.
check_margins() is what the builders hold a draw to and what the CPU test asserts again for every case.  Cases are built once per
process (lru_cache) and never modified by a test.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import pose_depth_ref as dr
import pose_eval_ref as pr

MARGIN = 1e-6
CAM = dr.Cam()
SCALE_448 = (640 / 448, 480 / 448)      # a 448-pixel pipeline's keypoints on a 640 x 480 depth image
WARP_SIZES = (1, 5, 64, 257, 1024, 1025, 4096, (300, 257, 131))      # n1 = n2 = K, and one (K, n1, n2)


# ------------------------------------------------------------------------------------------------------------- depth gather
def _gather_case(h, w, k, n, scale, seed):
    rng = np.random.default_rng(seed)
    depth = rng.integers(1, 65535, (n, h, w)).astype(np.uint16)
    depth[:, 0, 0], depth[:, h - 1, w - 1], depth[:, 2, 3] = 0, 65535, 65535
    depth[0, 1, 1] = 0
    sx, sy = scale
    kp = np.stack([rng.uniform(-0.2 * w, 1.2 * w, (n, k)) / sx, rng.uniform(-0.2 * h, 1.2 * h, (n, k)) / sy], axis=2).astype(np.float32)
    exact = np.zeros((n, k), bool)
    special = [(2.5, 1.5), (-0.75, 1.0), (w - 0.5, 2.0), (np.nan, 1.0), (0.25, 0.25)]      # -> (2, 3) = 65535; left; right; NaN; (0, 0) = 0
    if k >= 12:
        special += [(1.0, np.nan), (1e30, 1.0), (-1e30, 1.0), (1.0, h - 0.5), (-0.5, 1.0), (w - 1.0, h - 1.0), (1.25, 0.75)]
    if sx == 1.0 and sy == 1.0:
        for f in range(n):
            kp[f, :len(special)] = np.array(special, np.float32)
            exact[f, :len(special)] = True
    else:                                                   # units that are no depth pixels: NaN and the far outside only
        kp[:, 0], kp[:, 1], kp[:, 2] = (np.nan, 1.0), (-1e30, 5.0), (0.25 / sx, 0.25 / sy)      # the last: pixel (0, 0), a raw 0
        exact[:, :2] = True
    return dict(name=f"{h}x{w}_k{k}_n{n}_s{sx:.3f}", depth=depth, kp=kp, scale_x=sx, scale_y=sy, exact=exact)


@lru_cache(maxsize=None)
def gather_cases():
    out = []
    for h, w, k, n, scale in ((6, 8, 5, 1, (1.0, 1.0)), (6, 8, 70, 3, (1.0, 1.0)), (480, 640, 5, 3, (1.0, 1.0)), (480, 640, 70, 1, (1.0, 1.0)),
                              (480, 640, 70, 3, SCALE_448), (480, 640, 5, 1, SCALE_448), (6, 8, 70, 1, (8 / 448, 6 / 448))):
        seed = 1000 * h + 10 * k + n
        while True:
            c = _gather_case(h, w, k, n, scale, seed)
            if dr.gather_margin(c["kp"][~c["exact"]], c["scale_x"], c["scale_y"]) >= MARGIN:
                break
            seed += 100_000
        out.append(c)
    return out


# -------------------------------------------------------------------------------------------------------- warp and search
def check_margins(c) -> dict:
    """The least margins over the present pairs of a warp case (keys of pose_depth_ref.margins)."""
    k, n1, n2 = c["bank"].shape[1], c["n1"], c["n2"]
    least = dict(edge=np.inf, gap=np.inf, z=np.inf, view=np.inf)
    for p, (a, b) in enumerate(zip(c["first"], c["second"])):
        if not (0 <= a < len(c["bank"]) and 0 <= b < len(c["bank"])):
            continue
        m = dr.margins(c["bank"][a, :n1], c["bank"][b, :n2], c["depth_bank"][a, :n1], c["T"][p], c["cam"], c["threshold"], c["scale_x"],
                       c["scale_y"])
        least = {key: min(least[key], m[key]) for key in least}
    return least


def _pose(rng, angle_deg, shift):
    R = dr.rotation(rng.normal(size=3), np.deg2rad(angle_deg))
    return dr.rigid(R, rng.uniform(-shift, shift, 3))


def _warp_case(size, scale, seed):
    k, n1, n2 = (size, size, size) if isinstance(size, int) else size
    rng = np.random.default_rng(seed)
    sx, sy = scale
    cam = CAM

    def frame():
        return np.stack([rng.uniform(0, cam.width, k) / sx, rng.uniform(0, cam.height, k) / sy], axis=1).astype(np.float32)
    bank = np.stack([frame() for _ in range(3)])
    depth_bank = rng.integers(2500, 25000, (3, k)).astype(np.int32)           # 0.5 m .. 5 m
    T01, T12 = _pose(rng, 2.0, 0.05), _pose(rng, 3.0, 0.08)
    turn = dr.rigid(dr.rotation([0.0, 1.0, 0.0], np.pi), [0.0, 0.0, 0.0])      # 180 degrees about y: Z' = -z in every row
    ident = dr.rigid(np.eye(3), [0.0, 0.0, 0.0])
    # half of frame 1 (frame 2) are frame 0's (frame 1's) points seen from there, 1.5 px of noise on them
    for a, b, T in ((0, 1, T01), (1, 2, T12)):
        pj = dr.project(bank[a], depth_bank[a], T, cam, sx, sy)
        rows = rng.permutation(k)[: k // 2]
        rows = rows[pj["valid"][rows]]
        bank[b, rows] = (pj["warped"][rows] + rng.normal(0, 1.5, (len(rows), 2))).astype(np.float32)
    if k >= 6:
        bank[0, -2:], bank[1, -3:] = bank[0, :2], bank[1, :3]                  # exact duplicates: ties, the lowest index wins
    if k >= 5:
        depth_bank[0, 1], depth_bank[0, 2] = 0, -1                             # no measurement; outside the depth image
        depth_bank[0, 3] = 2500                                                # a near corner point that T01 takes out of frame 1's view
        for cu, cv in ((1.0, 1.0), (cam.width - 2.0, 1.0), (1.0, cam.height - 2.0), (cam.width - 2.0, cam.height - 2.0)):
            bank[0, 3] = (cu / sx, cv / sy)
            if not dr.project(bank[0, 3:4], depth_bank[0, 3:4], T01, cam, sx, sy)["valid"][0]:
                break
        else:
            return None                                                        # this pose keeps all four corners: another seed
    if isinstance(size, int) and size >= 1024:                                 # the large shapes: two pairs
        first, second, T = [0, 1], [1, 2], np.stack([T01, T12])
    else:                                                                      # every kind of pair
        first, second = [0, -1, 0, 0, 1, 0, 2, 1], [1, 0, 0, 1, 2, 2, 7, 0]
        T = np.stack([T01, T01, ident, T01, T12, turn, ident, _pose(rng, 1.0, 0.03)])
    return dict(name=f"k{k}_n{n1}_m{n2}_s{sx:.3f}", bank=bank, depth_bank=depth_bank, first=np.array(first, np.int32),
                second=np.array(second, np.int32), T=T, cam=cam, scale_x=sx, scale_y=sy, threshold=3.0, n1=n1, n2=n2)


def margins_ok(m) -> bool:
    return all(v >= MARGIN for v in m.values())


@lru_cache(maxsize=None)
def warp_case(index: int):
    """The case of WARP_SIZES[index]; sizes alternate between scale 1 and the 448-pixel pipeline's scale."""
    size = WARP_SIZES[index]
    seed = 7000 + index
    while True:
        c = _warp_case(size, (1.0, 1.0) if index % 2 else SCALE_448, seed)
        if c is not None and margins_ok(check_margins(c)):
            return c
        seed += 100


# ------------------------------------------------------------------------------------------- t = 0: the homography's cases
HOMOGRAPHY_K = 200


def _homography_case(scale, seed):
    rng = np.random.default_rng(seed)
    sx, sy = scale
    cam, k = CAM, HOMOGRAPHY_K
    angles = (0.5, 5.0, 12.0, 20.0)
    Rs = [dr.rotation(rng.normal(size=3), np.deg2rad(a)) for a in angles]
    T = np.stack([dr.rigid(R, [0.0, 0.0, 0.0]) for R in Rs])
    bank = np.zeros((1 + len(Rs), k, 2), np.float32)
    depth_bank = rng.integers(1, 65536, (1 + len(Rs), k)).astype(np.int32)     # any depth: a rotation does not look at it
    filled = 0
    while filled < k:                                                           # frame 0: points every rotation keeps in view
        q = np.stack([rng.uniform(0, cam.width, 4 * k) / sx, rng.uniform(0, cam.height, 4 * k) / sy], axis=1).astype(np.float32)
        d = np.full(len(q), 5000, np.int32)
        ok = np.ones(len(q), bool)
        for t in T:
            pj = dr.project(q, d, t, cam, sx, sy)
            ok &= pj["valid"] & (pj["Z2"] / pj["z"] >= 0.55)
        q = q[ok][: k - filled]
        bank[0, filled:filled + len(q)] = q
        filled += len(q)
    for p, t in enumerate(T):                                                   # frame 1 + p: frame 0 seen after rotation p, noise on half
        pj = dr.project(bank[0], depth_bank[0], t, cam, sx, sy)
        noise = rng.normal(0, 1.5, (k, 2)) * (rng.random((k, 1)) < 0.5) + rng.normal(0, 40.0, (k, 2)) * (rng.random((k, 1)) < 0.3)
        bank[1 + p] = (pj["warped"] + noise).astype(np.float32)
    H = np.stack([dr.homography_for(R, cam, sx, sy) for R in Rs])
    return dict(name=f"t0_s{sx:.3f}", bank=bank, depth_bank=depth_bank, first=np.zeros(len(Rs), np.int32),
                second=np.arange(1, 1 + len(Rs), dtype=np.int32), T=T, H=H, cam=cam, scale_x=sx, scale_y=sy, threshold=3.0, n1=k, n2=k)


def homography_conditions(c) -> dict:
    """What the t = 0 comparison rests on, per case: every projection inside the view (all rows valid), the least Z' / z, and the
    margins of BOTH searches (the depth warp's and the homography's)."""
    inside, ratio, hom = True, np.inf, np.inf
    for p, (a, b) in enumerate(zip(c["first"], c["second"])):
        pj = dr.project(c["bank"][a], c["depth_bank"][a], c["T"][p], c["cam"], c["scale_x"], c["scale_y"])
        inside &= bool(pj["valid"].all())
        ratio = min(ratio, float((pj["Z2"] / pj["z"]).min()))
        hom = min(hom, *pr.margins(c["bank"][a], c["bank"][b], c["H"][p], c["threshold"]))
    return dict(inside=inside, ratio=ratio, hom=hom, depth=check_margins(c))


@lru_cache(maxsize=None)
def homography_cases():
    out = []
    for i, scale in enumerate(((1.0, 1.0), SCALE_448)):
        seed = 9100 + i
        while True:
            c = _homography_case(scale, seed)
            cond = homography_conditions(c)
            if cond["inside"] and cond["ratio"] >= 0.5 and cond["hom"] >= MARGIN and margins_ok(cond["depth"]):
                break
            seed += 100
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------ translation is seen
TRANSLATION_K = 300


@lru_cache(maxsize=None)
def translation_case():
    """A scene 0.5 - 5 m in front of camera a, camera b 0.1 m to the side and turned by 1 degree.  Raw depths are drawn first, so
    z = d / 5000 is what the entry computes; frame b's keypoints are the projections of the moved points rounded to fp32 (a
    row that leaves the view gets a far-off point instead)."""
    seed = 4242
    while True:
        rng = np.random.default_rng(seed)
        cam, k = CAM, TRANSLATION_K
        a = np.stack([rng.uniform(0, cam.width, k), rng.uniform(0, cam.height, k)], axis=1).astype(np.float32)
        d = rng.integers(2500, 25000, k).astype(np.int32)
        R = dr.rotation([0.2, 1.0, 0.1], np.deg2rad(1.0))
        T = dr.rigid(R, [0.1, 0.0, 0.0])
        pj = dr.project(a, d, T, cam)
        b = np.where(pj["valid"][:, None], pj["warped"], rng.uniform(2000, 3000, (k, 2))).astype(np.float32)
        c = dict(name="translation", bank=np.stack([a, b]), depth_bank=np.stack([d, d]), first=np.zeros(1, np.int32),
                 second=np.ones(1, np.int32), T=T[None], H=dr.homography_for(R, cam)[None], cam=cam, scale_x=1.0, scale_y=1.0,
                 threshold=1e-2, n1=k, n2=k)
        hom = min(pr.margins(a, b, c["H"][0], 3.0))
        if margins_ok(check_margins(c)) and margins_ok(check_margins(dict(c, threshold=3.0))) and hom >= MARGIN:
            return c
        seed += 1


# --------------------------------------------------------------------------------------------------------------- score entry
@lru_cache(maxsize=None)
def score_case():
    """Five pairs of n1 = 70 rows: lists with rows on -2, -1 and matched rows, an idx1 out of range, counts above n1 and below 0,
    an empty list, an absent pair (every row -1, gt_count 0).  `plain` is the same with every -2 turned into -1."""
    rng = np.random.default_rng(515)
    P, n1 = 5, 70
    gt_of_row = rng.integers(0, n1, (P, n1)).astype(np.int32)
    kind = rng.random((P, n1))
    gt_of_row[kind < 0.3] = -2
    gt_of_row[(kind >= 0.3) & (kind < 0.5)] = -1
    gt_of_row[4] = -1                                                          # the absent pair's rows
    gt_count = (gt_of_row >= 0).sum(axis=1).astype(np.int32)
    matches = np.zeros((P, n1, 2), np.int64)
    for p in range(P):
        idx1 = rng.permutation(n1)
        matches[p, :, 0] = idx1
        right = rng.random(n1) < 0.6
        matches[p, :, 1] = np.where(right & (gt_of_row[p, idx1] >= 0), gt_of_row[p, idx1], rng.integers(0, n1, n1))
    matches[0, 3, 0], matches[0, 5, 0], matches[1, 0, 0] = n1, -1, 1 << 40     # idx1 outside [0, n1)
    value = rng.random((P, n1)).astype(np.float32)
    count = np.array([n1, n1 + 9, 0, 41, 17], np.int32)                        # full; above n1 (clamped); empty; part; the absent pair
    count_neg = np.array([-3, 5, 1, n1, 0], np.int32)
    plain = np.where(gt_of_row == -2, -1, gt_of_row).astype(np.int32)
    return dict(matches=matches, value=value, count=count, count_neg=count_neg, gt_of_row=gt_of_row, gt_count=gt_count, plain=plain, n1=n1)


# ---------------------------------------------------------------------------------------------------------------- end to end
def sequence_depth(n: int = pr.SEQ_FRAMES, h: int = 480, w: int = 640) -> np.ndarray:
    """(n, h, w) uint16 raw depth for the 12-frame synthetic sequence of pose_eval_ref.sequence_inputs: a tilted plane 1.5 - 3 m away
    with 32 x 32-pixel steps, and a band without measurement."""
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w), np.uint16)
    for f in range(n):
        plane = 7500 + 10 * f + 8.0 * xx + 4.0 * yy
        steps = rng.integers(0, 1500, (h // 32 + 1, w // 32 + 1))[yy // 32, xx // 32]
        out[f] = (plane + steps).astype(np.uint16)
        out[f, 100 + 5 * f:120 + 5 * f] = 0
    return out
