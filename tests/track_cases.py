"""Seeded cases for the four entries of libsslam_track.so (tests/test_tracks_cpu.py, tests/test_gpu_tracks.py): link rows with every
way a row or a slot can fail its rule, banks at the sizes where a kernel takes another path, planted scenes for the landmarks with
every way a member can fail to be an observation, and the planted study's scenes.  numpy only; a case is made once and shared.
"""
from __future__ import annotations

import functools
import types

import numpy as np

CAMERA = types.SimpleNamespace(fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_scale=5000.0, width=640, height=480)

# name -> (n_bank, K, n1, rows): the sizes are the smallest at which each kernel can go wrong - 0, 1, 3, 4, 5 and 6 pointer-jumping
# rounds (a non-power-of-two n_bank rounds up), K past a wave (70) and past a workgroup (257), n_bank * K exactly at and just past one
# tile of the numbering scan (1024, 1025)
def _consecutive(n):
    return [(i, i + 1) for i in range(n - 1)]


LINK_CASES = {
    "n1_k1": (1, 1, 1, [(0, 0)]),
    "n2_k8": (2, 8, 8, _consecutive(2)),
    "n5_k70": (5, 70, 70, _consecutive(5)),
    "n9_k257": (9, 257, 200, _consecutive(9)),
    "n17_k8": (17, 8, 6, _consecutive(17)),
    "n33_k70": (33, 70, 70, _consecutive(33)),
    "scan_at_1024": (128, 8, 8, _consecutive(128)),
    "scan_past_1025": (205, 5, 5, _consecutive(205)),
    "bridged_gap": (6, 8, 8, [(0, 1), (1, 3), (3, 4), (4, 5)]),
    # two rows for one second (0,2),(1,2); two for one first (3,4),(3,5); an invalid row (5,99); first >= second (4,4),(6,2); -1 rows;
    # and (5,6), which stays a link row: the row (5,99) before it is not valid, so it is still the lowest VALID row naming 5 first
    "row_rules": (8, 8, 8, [(0, 2), (1, 2), (3, 4), (3, 5), (5, 99), (4, 4), (6, 2), (-1, 3), (2, -1), (5, 6), (6, 7), (2, 3)]),
}
LINK_NAMES = tuple(LINK_CASES)
ONE_TRACK = "one_track_33"


@functools.lru_cache(maxsize=None)
def links(name: str, clean: bool = False) -> dict:
    """first, second (P,) int32; matches (P, n1, 2) int64; count (P,) int32; mask (P, n1) int32; n_bank, K.  Unless `clean`, every row
    carries slots that break the slot rule: an idx1 named twice, an idx2 named twice, indices -1, K and 2^40, mask values 0 and -1,
    and some rows a count above n1 or below 0."""
    if name == ONE_TRACK:                                      # slot 3 of every frame is one scene point: a track through all 33 frames
        n_bank, k, n1 = 33, 8, 2
        rows = _consecutive(n_bank)
        m = np.zeros((len(rows), n1, 2), np.int64)
        m[:, 0] = (3, 3)
        m[:, 1] = (5, 6)
        return _frozen(dict(first=np.array([a for a, _ in rows], np.int32), second=np.array([b for _, b in rows], np.int32), matches=m,
                            count=np.full(len(rows), n1, np.int32), mask=np.ones((len(rows), n1), np.int32), n_bank=n_bank, K=k))
    n_bank, k, n1, rows = LINK_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    P = len(rows)
    m = np.zeros((P, n1, 2), np.int64)
    for p in range(P):
        m[p, :, 0] = rng.permutation(max(k, n1))[:n1] % k if n1 <= k else rng.integers(0, k, n1)
        m[p, :, 1] = rng.permutation(max(k, n1))[:n1] % k if n1 <= k else rng.integers(0, k, n1)
    count = rng.integers(max(n1 - 3, 0), n1 + 1, P).astype(np.int32)
    mask = np.ones((P, n1), np.int32)
    if not clean and n1 >= 6:
        for p in range(P):
            j = rng.permutation(n1)
            m[p, j[0], 0] = m[p, j[1], 0]                      # one idx1 named twice
            m[p, j[2], 1] = m[p, j[3], 1]                      # one idx2 named twice
            m[p, j[4], rng.integers(0, 2)] = (-1, k, 2 ** 40)[p % 3]
            mask[p, j[5]] = (0, -1)[p % 2]
        count[0::5] = n1 + 7
        count[3::5] = -2
    return _frozen(dict(first=np.array([a for a, _ in rows], np.int32), second=np.array([b for _, b in rows], np.int32), matches=m, count=count,
                        mask=mask, n_bank=n_bank, K=k))


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def steps_of(name: str):
    """A link case with rows (a_i, i) only, as the online bank steps them: frame i -> (first, row index) or (-1, None)."""
    c = links(name)
    by_second = {}
    for p, (a, b) in enumerate(zip(c["first"], c["second"])):
        by_second.setdefault(int(b), (int(a), p))
    return [by_second.get(i, (-1, None)) for i in range(c["n_bank"])]


# ------------------------------------------------------------------------------------------------------------------ planted scenes
def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def poses(seed: int, n: int, rotate: bool = True) -> np.ndarray:
    """(n, 12) world -> camera rows of a smooth planted trajectory; frame 0 is the identity."""
    rng = np.random.default_rng(1000 + seed)
    C = np.zeros((n, 3, 4))
    for f in range(n):
        R = _rot(rng.normal(size=3), 0.01 * f) if rotate and f else np.eye(3)
        C[f, :, :3], C[f, :, 3] = R, (np.array([0.02 * f, -0.01 * f, 0.005 * f]) if f else 0.0)
    return C.reshape(n, 12)


def project(C, Pw, cam=CAMERA):
    """World points (k, 3) into the frame with row C (12,): pixels (k, 2) and depths in metres (k,), float64."""
    c = C.reshape(3, 4)
    X = Pw @ c[:, :3].T + c[:, 3]
    return np.stack([cam.fx * X[:, 0] / X[:, 2] + cam.cx, cam.fy * X[:, 1] / X[:, 2] + cam.cy], axis=1), X[:, 2]


@functools.lru_cache(maxsize=None)
def scene(seed: int = 0, n_bank: int = 7, k: int = 40, sigma_mix=(0.0, 0.0), dirty: bool = True) -> dict:
    """A planted scene: k world points seen by n_bank frames, frame f holding point j in slot perm_f[j]; the links are the true
    correspondences of consecutive frames (a few points drop out and come back as new tracks).  sigma_mix (small, large): the
    per-keypoint noise, 3 in 4 keypoints the small sigma; confidence = 1 / (1 + sigma).  dirty: every way a member can fail to be an
    observation and an observation to be kept is planted (the keys `planted` say where)."""
    rng = np.random.default_rng(77 + seed)
    cam = CAMERA
    Pw = np.stack([rng.uniform(-1.0, 1.0, k), rng.uniform(-0.7, 0.7, k), rng.uniform(1.5, 4.0, k)], axis=1)
    C = poses(seed, n_bank)
    perm = np.stack([rng.permutation(k) for _ in range(n_bank)])
    kp, depth = np.zeros((n_bank, k, 2), np.float32), np.zeros((n_bank, k), np.int32)
    sigma = np.where(rng.random((n_bank, k)) < 0.75, sigma_mix[0], sigma_mix[1])
    for f in range(n_bank):
        px, z = project(C[f], Pw, cam)
        kp[f, perm[f]] = (px + rng.normal(size=px.shape) * sigma[f, perm[f]][:, None]).astype(np.float32)
        depth[f, perm[f]] = np.rint(z * cam.depth_scale).astype(np.int32)
    seen = rng.random((n_bank - 1, k)) < 0.9                     # the link (f, f + 1) of point j exists
    first, second = np.arange(n_bank - 1, dtype=np.int32), np.arange(1, n_bank, dtype=np.int32)
    m = np.full((max(n_bank - 1, 1), k, 2), -1, np.int64)
    count = np.zeros(max(n_bank - 1, 1), np.int32)
    for f in range(n_bank - 1):
        j = np.flatnonzero(seen[f])
        m[f, :len(j), 0], m[f, :len(j), 1], count[f] = perm[f, j], perm[f + 1, j], len(j)
    weight = (1.0 / (1.0 + sigma)).astype(np.float32)
    planted = {}
    if dirty:
        assert n_bank >= 7 and k >= 24
        slot = lambda f, j: perm[f, j]
        seen[:, :12] = True                                      # points 0 .. 11 are whole tracks: their fates are planted below
        for f in range(n_bank - 1):
            j = np.flatnonzero(seen[f])
            m[f], count[f] = -1, len(j)
            m[f, :len(j), 0], m[f, :len(j), 1] = perm[f, j], perm[f + 1, j]
        for f in range(n_bank):
            depth[f, slot(f, 1)] = 0                              # point 1: no depth anywhere -> no observation, status 2
        for f in range(1, n_bank):
            depth[f, slot(f, 2)] = -1                             # point 2: one observation -> n_kept 1 < min_obs, status 1
        for f in range(2, n_bank):
            depth[f, slot(f, 3)] = 0                              # point 3: two observations, both good: min_obs 2 keeps it, 3 does not
        kp[3, slot(3, 6)] += np.float32(12.0)                     # point 6: one observation far off, the others kept: L is not L0
        for f in range(n_bank):
            kp[f, slot(f, 4), 0] += np.float32(25.0 * f)          # point 4: every observation far from the mean's reprojection
        wkinds = (0.0, np.nan, np.inf, -1.0, 1e-40)               # point 5: zero, NaN, infinite, negative and subnormal weights
        for f, w in enumerate(wkinds):
            weight[f, slot(f, 5)] = w
        planted = dict(clean=0, no_obs=1, one_obs=2, two_obs=3, none_kept=4, weights=5, one_outlier=6, bad_frame=n_bank - 1)
        C = C.copy()
        C[n_bank - 1, 7] = np.inf                                # the last frame's C row is not finite: none of its members observes
    return _frozen(dict(kp=kp, depth=depth, C=np.ascontiguousarray(C), first=first, second=second, matches=m, count=count, weight=weight,
                        sigma=sigma, Pw=Pw, perm=perm, n_bank=n_bank, K=k, planted=planted))


@functools.lru_cache(maxsize=None)
def behind_scene() -> dict:
    """Two frames, one track: frame 1's camera looks the other way, its keypoint carries a positive depth all the same.  With weight
    1000 on frame 0 the first mean lies at frame 0's point, behind camera 1: Z' <= 0 there, that observation is not kept and its
    residual is +inf."""
    cam = CAMERA
    C = np.zeros((2, 3, 4))
    C[0, :, :3], C[1, :, :3] = np.eye(3), np.diag([-1.0, 1.0, -1.0])
    kp = np.array([[[300.0, 200.0], [10.0, 10.0]], [[320.0, 240.0], [20.0, 20.0]]], np.float32)
    depth = np.array([[10000, 0], [10000, 0]], np.int32)
    m = np.array([[[0, 0], [-1, -1]]], np.int64)
    return _frozen(dict(kp=kp, depth=depth, C=C.reshape(2, 12), first=np.array([0], np.int32), second=np.array([1], np.int32), matches=m,
                        count=np.array([1], np.int32), weight=np.array([[1000.0, 1.0], [1.0, 1.0]], np.float32), n_bank=2, K=2, camera=cam))


@functools.lru_cache(maxsize=None)
def exact_scene(seed: int = 0, n_bank: int = 6, k: int = 48) -> dict:
    """The exact planted case: poses that are translations parallel to the image plane by multiples of 4 / fx metres, points at depths
    0.5, 1 and 2 m - exact multiples of the depth quantum - and frame-0 keypoints on a quarter-pixel grid: every keypoint of every
    frame is a float32 exactly, every depth an integer exactly.  Pw is the planted point, the frame-0 back-projection."""
    rng = np.random.default_rng(500 + seed)
    cam = CAMERA
    z = rng.choice([0.5, 1.0, 2.0], k)
    x0 = rng.integers(4 * 200, 4 * 440, k) / 4.0
    y0 = rng.integers(4 * 150, 4 * 330, k) / 4.0
    Pw = np.stack([(x0 - cam.cx) * z / cam.fx, (y0 - cam.cy) * z / cam.fy, z], axis=1)
    C = np.tile(np.eye(3, 4), (n_bank, 1, 1))
    kp, depth = np.zeros((n_bank, k, 2), np.float32), np.zeros((n_bank, k), np.int32)
    perm = np.stack([rng.permutation(k) for _ in range(n_bank)])
    for f in range(n_bank):
        nx, ny = 4 * f, -4 * (f % 3)                              # the shift in pixels at 1 m
        C[f, 0, 3], C[f, 1, 3] = nx / cam.fx, ny / cam.fy
        kp[f, perm[f], 0], kp[f, perm[f], 1] = x0 + nx / z, y0 + ny / z
        depth[f, perm[f]] = np.rint(z * cam.depth_scale)
        assert np.array_equal(kp[f, perm[f], 0].astype(np.float64), x0 + nx / z) and np.array_equal(depth[f, perm[f]] / cam.depth_scale, z)
    first, second = np.arange(n_bank - 1, dtype=np.int32), np.arange(1, n_bank, dtype=np.int32)
    m = np.stack([np.stack([perm[f], perm[f + 1]], axis=1) for f in range(n_bank - 1)]).astype(np.int64)
    return _frozen(dict(kp=kp, depth=depth, C=C.reshape(n_bank, 12), first=first, second=second, matches=m,
                        count=np.full(n_bank - 1, k, np.int32), Pw=Pw, perm=perm, n_bank=n_bank, K=k))
