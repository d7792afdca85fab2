"""A float64 numpy restatement of sslam_pose_ransac_pairs (csrc/pose_estimate.hip), written from the contract in
include/sslam_hip.h: the usable rows, the counter-based sampler, Horn's closed form with 8 cyclic Jacobi sweeps, the score, the
arg-max, the refit with its stated summation tree, the mask and the rms.  It is vectorised over hypotheses and rows, but every
elementwise operation is one numpy float64 operation in the header's order; nothing the device computes goes through np.dot, @
or np.sum, and the Jacobi skip is an np.where.

Tolerance: NONE.  Every step is the same sequence of IEEE-754 correctly rounded operations (+ - * / sqrt on float64, exact
int -> float64 and float32 -> float64 conversions, 64-bit integer arithmetic) on both sides, and both sides take them in one
order, so the device must equal this restatement bit for bit in every output, T and rms included.  numpy's float64 + - * / and
np.sqrt are the host's IEEE operations; the device's are the compiler's correctly rounded float64 division and square root with
contraction off.

margins() gives what the case lists hold themselves to: how far the restatement's own distances stay from the threshold and its
own Z' from 0, so that the integer outputs do not hang on a last bit.
"""
from __future__ import annotations

import numpy as np

from pose_depth_ref import Cam, rigid, rotation  # noqa: F401  (the case lists use them)

MAX_HYP = 1024
THREADS = 256           # the refit's sums: 256 partials, lanes by xor 32 .. 1, four waves in order
GOLD = np.uint64(0x9e3779b97f4a7c15)
KEYS = ("T", "inlier_count", "usable_count", "best_hypothesis", "refit_kept", "inlier_of_slot", "rms")


# ------------------------------------------------------------------------------------------------------------------ sampler
def mix(x):
    """splitmix64's finalizer on a uint64 array (arithmetic modulo 2^64)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94d049bb133111eb)
        x = x ^ (x >> np.uint64(31))
    return x


def draw(seed: int, h, k: int, n: int):
    """draw(h, k, n) of the header for an array of hypothesis indices h."""
    h = np.asarray(h, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = mix(np.uint64(seed) + GOLD * (np.uint64(3) * h + np.uint64(k + 1)))
        return (((x >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def sample(seed: int, n_hyp: int, n: int) -> np.ndarray:
    """(n_hyp, 3) int64: the three distinct usable rows of every hypothesis, n >= 3."""
    h = np.arange(n_hyp)
    i0 = draw(seed, h, 0, n)
    i1 = draw(seed, h, 1, n - 1)
    i1 = i1 + (i1 >= i0)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = draw(seed, h, 2, n - 2)
    i2 = i2 + (i2 >= lo)
    i2 = i2 + (i2 >= hi)
    return np.stack([i0, i1, i2], axis=1)


# --------------------------------------------------------------------------------------------------------------------- rows
def back_project(kp, d, cam, sx, sy):
    """(n, 3) float64 from keypoints kp (n, 2) fp32 and raw depths d (n,) int32, the formulas of sslam_pose_depth_nn_pairs."""
    fx, fy, cx, cy, ds = (np.float64(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.depth_scale))
    u, v = kp[:, 0].astype(np.float64) * np.float64(sx), kp[:, 1].astype(np.float64) * np.float64(sy)
    z = d.astype(np.float64) / ds
    return np.stack([((u - cx) * z) / fx, ((v - cy) * z) / fy, z], axis=1)


def usable_rows(kp_a, kp_b, d_a, d_b, matches, count, cam, sx, sy):
    """The usable rows of one pair in slot order: dict of slot (n,), Xa, Xb (n, 3) float64, kb (n, 2) fp32, listed (the clamped count)."""
    n1, k = len(matches), len(kp_a)
    c = int(np.clip(count, 0, n1))
    i1, i2 = matches[:c, 0], matches[:c, 1]
    ok = (i1 >= 0) & (i1 < k) & (i2 >= 0) & (i2 < k)
    j1, j2 = np.where(ok, i1, 0), np.where(ok, i2, 0)
    ok &= (d_a[j1] > 0) & (d_b[j2] > 0)
    slot = np.where(ok)[0]
    j1, j2 = j1[slot], j2[slot]
    return dict(slot=slot, Xa=back_project(kp_a[j1], d_a[j1], cam, sx, sy), Xb=back_project(kp_b[j2], d_b[j2], cam, sx, sy), kb=kp_b[j2],
                listed=c)


# ------------------------------------------------------------------------------------------------------------------- solver
def _rotate(a, v, p, q):
    apq = a[p][q]
    skip = apq == 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        theta = (a[q][q] - a[p][p]) / (2.0 * apq)
        t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        new = {(p, p): a[p][p] - h, (q, q): a[q][q] + h, (p, q): np.zeros_like(apq)}
        for r in range(4):
            if r in (p, q):
                continue
            rp, rq = (min(r, p), max(r, p)), (min(r, q), max(r, q))
            g, k = a[rp[0]][rp[1]], a[rq[0]][rq[1]]
            new[rp], new[rq] = c * g - s * k, s * g + c * k
        newv = {}
        for r in range(4):
            g, k = v[r][p], v[r][q]
            newv[(r, p)], newv[(r, q)] = c * g - s * k, s * g + c * k
    for (i, j), val in new.items():
        a[i][j] = np.where(skip, a[i][j], val)
    for (i, j), val in newv.items():
        v[i][j] = np.where(skip, v[i][j], val)


def horn(M, ca, cb):
    """[R | t] (H, 12) from the cross-covariances M (H, 3, 3), M[:, i, j] = sum (Xa - ca)_i (Xb - cb)_j, and the centroids (H, 3)."""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (M[:, i, j] for i in range(3) for j in range(3))
    a = [[None] * 4 for _ in range(4)]
    a[0][0], a[0][1], a[0][2], a[0][3] = (Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx
    a[1][1], a[1][2], a[1][3] = (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz
    a[2][2], a[2][3] = (Syy - Sxx) - Szz, Syz + Szy
    a[3][3] = (Szz - Sxx) - Syy
    one, zero = np.ones_like(Sxx), np.zeros_like(Sxx)
    v = [[one if r == c else zero for c in range(4)] for r in range(4)]
    for _ in range(8):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _rotate(a, v, p, q)
    best, quat = a[0][0], [v[r][0] for r in range(4)]
    for j in range(1, 4):
        better = a[j][j] > best
        best = np.where(better, a[j][j], best)
        quat = [np.where(better, v[r][j], quat[r]) for r in range(4)]
    w, x, y, z = quat
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
        neg = w < 0.0
        w, x, y, z = (np.where(neg, -e, e) for e in (w, x, y, z))
        ww, xx, yy, zz = w * w, x * x, y * y, z * z
        R = [((ww + xx) - yy) - zz, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
             2.0 * (x * y + w * z), ((ww - xx) + yy) - zz, 2.0 * (y * z - w * x),
             2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((ww - xx) - yy) + zz]
        T = np.empty((len(Sxx), 12))
        for i in range(3):
            T[:, 4 * i:4 * i + 3] = np.stack(R[3 * i:3 * i + 3], axis=1)
            T[:, 4 * i + 3] = cb[:, i] - ((R[3 * i] * ca[:, 0] + R[3 * i + 1] * ca[:, 1]) + R[3 * i + 2] * ca[:, 2])
    return T


def solve_samples(Xa, Xb):
    """Horn on (H, 3, 3) triples of points, [hypothesis, sample, xyz], summed in sample order from +0.0."""
    def total(t):                                        # ((0 + t0) + t1) + t2
        return ((0.0 + t[:, 0]) + t[:, 1]) + t[:, 2]
    ca, cb = total(Xa) / 3.0, total(Xb) / 3.0
    A, B = Xa - ca[:, None, :], Xb - cb[:, None, :]
    M = np.stack([np.stack([total(A[:, :, i] * B[:, :, j]) for j in range(3)], axis=1) for i in range(3)], axis=1)
    return horn(M, ca, cb)


def tree_sum(terms):
    """The refit's order: terms (n, ...) of the usable rows (+0.0 where a row is no inlier) -> (...)."""
    n = len(terms)
    k = -(-n // THREADS)
    pad = np.zeros((k * THREADS,) + terms.shape[1:])
    pad[:n] = terms
    pad = pad.reshape((k, THREADS) + terms.shape[1:])
    part = np.zeros((THREADS,) + terms.shape[1:])
    for j in range(k):                                   # thread t: rows t, t + 256, ... ascending
        part = part + pad[j]
    part = part.reshape((THREADS // 64, 64) + terms.shape[1:])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ o]
    w = part[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def solve_inliers(Xa, Xb, inl):
    """Horn over the rows flagged in inl (n,), the sums in the refit's order -> (12,)."""
    n = np.float64(int(inl.sum()))
    with np.errstate(divide="ignore", invalid="ignore"):
        ca = tree_sum(np.where(inl[:, None], Xa, 0.0)) / n
        cb = tree_sum(np.where(inl[:, None], Xb, 0.0)) / n
        A, B = Xa - ca, Xb - cb
        M = tree_sum(np.where(inl[:, None, None], A[:, :, None] * B[:, None, :], 0.0))
    return horn(M[None], ca[None], cb[None])[0]


# -------------------------------------------------------------------------------------------------------------------- score
def score(T, Xa, kb, cam, sx, sy, threshold):
    """Poses T (H, 12) on rows Xa (n, 3), kb (n, 2): dict of inlier (H, n) bool, s (H, n) squared distance, d (H, n), Z2 (H, n)."""
    fx, fy, cx, cy = (np.float64(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    sx, sy = np.float64(sx), np.float64(sy)
    m = [T[:, e][:, None] for e in range(12)]
    X, Y, Z = Xa[None, :, 0], Xa[None, :, 1], Xa[None, :, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        X2 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
        Y2 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
        Z2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
        u2, v2 = (fx * X2) / Z2 + cx, (fy * Y2) / Z2 + cy
        dx, dy = u2 / sx - kb[None, :, 0].astype(np.float64), v2 / sy - kb[None, :, 1].astype(np.float64)
        s = dx * dx + dy * dy
        d = np.sqrt(s)
        finite = np.isfinite(T).all(axis=1)[:, None]      # a pose with a non-finite entry has no inliers
        inlier = (Z2 > 0.0) & (d < np.float64(threshold)) & finite
    return dict(inlier=inlier, s=s, d=d, Z2=Z2)


# --------------------------------------------------------------------------------------------------------------------- pair
def no_pose(n1, listed=0, usable_slots=()):
    mask = np.zeros(n1, np.int32)
    mask[:listed] = -1
    mask[list(usable_slots)] = 0
    return dict(T=np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]), inlier_count=0, usable_count=len(usable_slots), best_hypothesis=-1,
                refit_kept=0, inlier_of_slot=mask, rms=0.0)


def ransac(kp_a, kp_b, d_a, d_b, matches, count, cam, threshold, n_hyp, seed, sx=1.0, sy=1.0, detail=False):
    """One present pair: dict of KEYS (T (12,), python ints, inlier_of_slot (n1,) int32, rms); with detail also the hypotheses,
    their inlier counts, the refit pose and the rows."""
    n1 = len(matches)
    rows = usable_rows(kp_a, kp_b, d_a, d_b, matches, count, cam, sx, sy)
    n = len(rows["slot"])
    if n < 3:
        return no_pose(n1, rows["listed"], rows["slot"])
    Xa, Xb, kb = rows["Xa"], rows["Xb"], rows["kb"]
    idx = sample(seed, n_hyp, n)
    hyp = solve_samples(Xa[idx], Xb[idx])
    counts = np.concatenate([score(hyp[h0:h0 + 256], Xa, kb, cam, sx, sy, threshold)["inlier"].sum(axis=1) for h0 in range(0, n_hyp, 256)])
    best = int(np.argmax(counts))                        # the lowest h among the most inliers
    best_n = int(counts[best])
    T, kept, refit = hyp[best], 0, None
    if best_n >= 3:
        inl = score(hyp[best:best + 1], Xa, kb, cam, sx, sy, threshold)["inlier"][0]
        refit = solve_inliers(Xa, Xb, inl)
        if int(score(refit[None], Xa, kb, cam, sx, sy, threshold)["inlier"].sum()) >= best_n:
            T, kept = refit, 1
    sc = score(T[None], Xa, kb, cam, sx, sy, threshold)
    inl = sc["inlier"][0]
    final_n = int(inl.sum())
    mask = np.zeros(n1, np.int32)
    mask[:rows["listed"]] = -1
    mask[rows["slot"]] = inl
    rms = float(np.sqrt(tree_sum(np.where(inl, sc["s"][0], 0.0)) / np.float64(final_n))) if final_n else 0.0
    out = dict(T=T, inlier_count=final_n, usable_count=n, best_hypothesis=best, refit_kept=kept, inlier_of_slot=mask, rms=rms)
    if detail:
        out.update(hypotheses=hyp, counts=counts, refit=refit, rows=rows, samples=idx)
    return out


def ransac_pairs(bank, depth_bank, first, second, matches, count, cam, threshold, n_hyp, seed, sx=1.0, sy=1.0, detail=False):
    """The listed pairs of a bank (n_bank, K, 2) fp32 with depths (n_bank, K) int32: a list of ransac() dicts."""
    out = []
    for p, (a, b) in enumerate(zip(first, second)):
        if not (0 <= a < len(bank) and 0 <= b < len(bank)):
            out.append(no_pose(matches.shape[1]))
        else:
            out.append(ransac(bank[a], bank[b], depth_bank[a], depth_bank[b], matches[p], count[p], cam, threshold, n_hyp, seed, sx, sy, detail))
    return out


def stacked(results) -> dict:
    """A list of ransac() dicts as the arrays the device writes."""
    dt = dict(T=np.float64, rms=np.float64)
    return {key: np.stack([np.asarray(r[key], dtype=dt.get(key, np.int32)) for r in results]) for key in KEYS}


def margins(kp_a, kp_b, d_a, d_b, matches, count, cam, threshold, n_hyp, seed, sx=1.0, sy=1.0) -> dict:
    """Over every finite pose the pair's run scores (all hypotheses and the refit) and every usable row:
    edge  the least |distance - threshold| over the rows with Z' > 0,   z  the least |Z'|   (inf without a pose)."""
    r = ransac(kp_a, kp_b, d_a, d_b, matches, count, cam, threshold, n_hyp, seed, sx, sy, detail=True)
    out = dict(edge=np.inf, z=np.inf)
    if r["best_hypothesis"] < 0:
        return out
    poses = r["hypotheses"] if r["refit"] is None else np.concatenate([r["hypotheses"], r["refit"][None]])
    poses = poses[np.isfinite(poses).all(axis=1)]
    for h0 in range(0, len(poses), 256):
        sc = score(poses[h0:h0 + 256], r["rows"]["Xa"], r["rows"]["kb"], cam, sx, sy, threshold)
        front = sc["Z2"] > 0
        if front.any():
            out["edge"] = min(out["edge"], float(np.min(np.abs(sc["d"][front] - threshold))))
        out["z"] = min(out["z"], float(np.min(np.abs(sc["Z2"]))))
    return out


# -------------------------------------------------------------------------------------------------------------- against truth
def pose_error(T, T_true):
    """(rotation error in degrees, translation error in metres) of [R | t] (12,) against the planted one."""
    A, B = np.asarray(T).reshape(3, 4), np.asarray(T_true).reshape(3, 4)
    E = A[:, :3] @ B[:, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(E) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(A[:, 3] - B[:, 3]))
