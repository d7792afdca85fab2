"""include/sslam_weight.h in numpy float64, for ONE pair: the arithmetic of sslu_match_weights and of
sslu_pose_refine_weighted_pairs (with the depth lookup of sslam_keypoint_depth in front) as the header states them, every
elementwise operation one numpy operation in the header's order, nothing through np.dot, @, np.sum or np.linalg.  It needs no GPU
and gives the bits the device entries give: evaluation.match_weights and evaluation.refine_relative_pose(weights=) run it, as
evaluation.PoseWindow runs window_numpy.  A caller on the device uses SequencePipeline.match_weights / refine_poses(weights=)."""
from __future__ import annotations

import numpy as np

PRODUCT, EXPECTED_ERROR = 0, 1
THREADS = 256
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]      # the 21 entries of H, row-major
_QUIET = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def weight_of(c1, c2, mode: int, sigma0: float = 1.0) -> np.ndarray:
    """The weight of confidences c1, c2 (fp32 arrays of one shape): c1 * c2, or s0^2 / ((s0^2 + e1^2) + e2^2) with
    e = 1 / (c + 1e-6) - 1 in float64, rounded once to fp32."""
    c1, c2 = np.asarray(c1, np.float32), np.asarray(c2, np.float32)
    with np.errstate(**_QUIET):
        if mode == PRODUCT:
            return (c1 * c2).astype(np.float32)
        s0 = np.float64(sigma0)
        s2 = s0 * s0
        e1 = np.float64(1.0) / (c1.astype(np.float64) + np.float64(1e-6)) - np.float64(1.0)
        e2 = np.float64(1.0) / (c2.astype(np.float64) + np.float64(1e-6)) - np.float64(1.0)
        return (s2 / ((s2 + e1 * e1) + e2 * e2)).astype(np.float32)


def match_weights(c1, c2, matches, mode: int, sigma0: float = 1.0) -> np.ndarray:
    """(P,) fp32: weight_of at every match (P, 2) [idx1, idx2] of the confidences c1 (N,), c2 (M,); +0.0 for an index outside."""
    i1, i2 = matches[:, 0].astype(np.int64), matches[:, 1].astype(np.int64)
    ok = (i1 >= 0) & (i1 < len(c1)) & (i2 >= 0) & (i2 < len(c2))
    out = np.zeros(len(matches), np.float32)
    out[ok] = weight_of(c1[i1[ok]], c2[i2[ok]], mode, sigma0)
    return out


def keypoint_depth(depth, kp) -> np.ndarray:
    """sslam_keypoint_depth at scale 1: depth (h, w) uint16, kp (n, 2) fp32 (x, y) -> (n,) int32, the raw value at the nearest
    pixel (floor(x + 0.5), floor(y + 0.5)), -1 outside the image - judged on the doubles -, a raw 0 staying 0."""
    h, w = depth.shape
    with np.errstate(invalid="ignore"):
        c, r = np.floor(kp[:, 0].astype(np.float64) + 0.5), np.floor(kp[:, 1].astype(np.float64) + 0.5)
        inside = (c >= 0) & (c < w) & (r >= 0) & (r < h)
    ci, ri = np.where(inside, c, 0).astype(np.int64), np.where(inside, r, 0).astype(np.int64)
    return np.where(inside, depth[ri, ci].astype(np.int32), np.int32(-1)).astype(np.int32)


def _back_project(kp, d, cam):
    fx, fy, cx, cy, ds = (np.float64(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.depth_scale))
    u, v = kp[:, 0].astype(np.float64) * np.float64(1.0), kp[:, 1].astype(np.float64) * np.float64(1.0)
    z = d.astype(np.float64) / ds
    return np.stack([((u - cx) * z) / fx, ((v - cy) * z) / fy, z], axis=1)


def _tree_sum(terms):
    """pose_block_sum's order: thread t of 256 adds the rows t, t + 256, ... ascending from +0.0; lanes by xor 32 .. 1; the four
    waves ((w0 + w1) + w2) + w3."""
    n = len(terms)
    k = -(-n // THREADS)
    pad = np.zeros((k * THREADS,) + terms.shape[1:])
    pad[:n] = terms
    pad = pad.reshape((k, THREADS) + terms.shape[1:])
    part = np.zeros((THREADS,) + terms.shape[1:])
    for j in range(k):
        part = part + pad[j]
    part = part.reshape((THREADS // 64, 64) + terms.shape[1:])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ o]
    w = part[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def _project(T, Xa, cam):
    fx, fy, cx, cy = (np.float64(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    m = [np.float64(v) for v in T]
    X, Y, Z = Xa[:, 0], Xa[:, 1], Xa[:, 2]
    X2 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
    Y2 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
    Z2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
    return X2, Y2, Z2, (fx * X2) / Z2 + cx, (fy * Y2) / Z2 + cy


def _score(T, Xa, kb, cam, threshold):
    """(inlier (n,) bool, s (n,)): Z' > 0 and sqrt(s) < threshold; a pose with a non-finite entry has no inliers."""
    with np.errstate(**_QUIET):
        _, _, Z2, u2, v2 = _project(T, Xa, cam)
        dx, dy = u2 / np.float64(1.0) - kb[:, 0].astype(np.float64), v2 / np.float64(1.0) - kb[:, 1].astype(np.float64)
        s = dx * dx + dy * dy
        return (Z2 > 0.0) & (np.sqrt(s) < np.float64(threshold)) & bool(np.isfinite(T).all()), s


def _pass(T, Xa, kb, g, sel, cam, huber):
    """The weighted pass at T over the selected rows: (cost, H (21,), grad (6,), behind)."""
    fx, fy, huber = np.float64(cam.fx), np.float64(cam.fy), np.float64(huber)
    with np.errstate(**_QUIET):
        kx, ky = fx / np.float64(1.0), fy / np.float64(1.0)
        X2, Y2, Z2, u2, v2 = _project(T, Xa, cam)
        rx, ry = u2 / np.float64(1.0) - kb[:, 0].astype(np.float64), v2 / np.float64(1.0) - kb[:, 1].astype(np.float64)
        s = rx * rx + ry * ry
        d = np.sqrt(s)
        quad = d <= huber
        w = np.where(quad, 1.0, huber / d)
        rho = np.where(quad, s, (2.0 * huber) * d - huber * huber)
        iz = 1.0 / Z2
        a, b = kx * iz, ky * iz
        c, e = -(a * (X2 * iz)), -(b * (Y2 * iz))
        zero = np.zeros_like(a)
        Ju = [a, zero, c, c * Y2, a * Z2 - c * X2, -(a * Y2)]
        Jv = [zero, b, e, e * Y2 - b * Z2, -(e * X2), b * X2]
        gd = g.astype(np.float64)
        gw = gd * w
        cols = [gd * rho] + [gw * (Ju[i] * Ju[j] + Jv[i] * Jv[j]) for i, j in TRIU] + [gw * (Ju[i] * rx + Jv[i] * ry) for i in range(6)]
        tot = _tree_sum(np.where(sel[:, None], np.stack(cols, axis=1), 0.0))
    return tot[0], tot[1:22], tot[22:28], int((sel & ~(Z2 > 0.0)).sum())


def _solve(H, grad):
    """H delta = -grad by the unpivoted LDL^T of include/sslam_hip.h: (delta (6,), ok)."""
    h = {}
    for (i, j), v in zip(TRIU, H):
        h[(i, j)] = h[(j, i)] = np.float64(v)
    L = [[None] * 6 for _ in range(6)]
    D, y, delta = [None] * 6, [None] * 6, [None] * 6
    ok = True
    with np.errstate(**_QUIET):
        for j in range(6):
            v = h[(j, j)]
            for k in range(j):
                v = v - (L[j][k] * L[j][k]) * D[k]
            D[j] = v
            ok = ok and bool(v > 0.0 and np.isfinite(v))
            for i in range(j + 1, 6):
                s = h[(i, j)]
                for k in range(j):
                    s = s - (L[i][k] * L[j][k]) * D[k]
                L[i][j] = s / v
        for i in range(6):
            v = -np.float64(grad[i])
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = v
        for i in range(5, -1, -1):
            v = y[i] / D[i]
            for k in range(i + 1, 6):
                v = v - L[k][i] * delta[k]
            delta[i] = v
    return np.array(delta, dtype=np.float64), ok


def _update(T, delta):
    m = [np.float64(v) for v in T]
    with np.errstate(**_QUIET):
        w, x, y, z = np.float64(1.0), np.float64(0.5) * delta[3], np.float64(0.5) * delta[4], np.float64(0.5) * delta[5]
        nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
        ww, xx, yy, zz = w * w, x * x, y * y, z * z
        R = [((ww + xx) - yy) - zz, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
             2.0 * (x * y + w * z), ((ww - xx) + yy) - zz, 2.0 * (y * z - w * x),
             2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((ww - xx) - yy) + zz]
        out = np.empty(12)
        for i in range(3):
            for j in range(3):
                out[4 * i + j] = (R[3 * i] * m[j] + R[3 * i + 1] * m[4 + j]) + R[3 * i + 2] * m[8 + j]
            out[4 * i + 3] = ((R[3 * i] * m[3] + R[3 * i + 1] * m[7]) + R[3 * i + 2] * m[11]) + delta[i]
    return out


def refine_pair(kp1, kp2, d1, d2, matches, weights, cam, threshold, huber, n_iter, T_in) -> dict:
    """One pair at scale 1: keypoints kp1 (N, 2), kp2 (M, 2) fp32 with their raw depths d1, d2 int32 (keypoint_depth), matches (P, 2),
    weights (P,) fp32, T_in (12,) -> dict of T (12,), status, iterations, selected_count, usable_count, inlier_count_in,
    inlier_count, inlier_of_slot (P,) int32, cost_in, cost, rms, info (21,), weight_sum."""
    T_in = np.asarray(T_in, dtype=np.float64).reshape(12)
    P = len(matches)
    i1, i2 = matches[:, 0].astype(np.int64), matches[:, 1].astype(np.int64)
    ok = (i1 >= 0) & (i1 < len(kp1)) & (i2 >= 0) & (i2 < len(kp2))
    j1, j2 = np.where(ok, i1, 0), np.where(ok, i2, 0)
    ok &= (d1[j1] > 0) & (d2[j2] > 0)
    slot = np.where(ok)[0]
    Xa, kb, g = _back_project(kp1[j1[slot]], d1[j1[slot]], cam), kp2[j2[slot]], np.asarray(weights, np.float32)[slot]
    mask = np.full(P, -1, np.int32)
    n = len(slot)
    geo = _score(T_in, Xa, kb, cam, threshold)[0] if n else np.zeros(0, bool)
    sel = geo & (g > 0) & np.isfinite(g)
    n_in, n_sel = int(geo.sum()), int(sel.sum())
    if n_sel < 3:
        mask[slot] = 0
        return dict(T=T_in.copy(), status=3, iterations=0, selected_count=0, usable_count=0, inlier_count_in=0, inlier_count=0, inlier_of_slot=mask,
                    cost_in=0.0, cost=0.0, rms=0.0, info=np.zeros(21), weight_sum=0.0)
    weight_sum = float(_tree_sum(np.where(sel, g.astype(np.float64), 0.0)))
    first = cur = _pass(T_in, Xa, kb, g, sel, cam, huber)
    T, accepted = T_in, 0
    for _ in range(n_iter):
        delta, fine = _solve(cur[1], cur[2])
        if not fine:
            break
        trial = _update(T, delta)
        tp = _pass(trial, Xa, kb, g, sel, cam, huber)
        if not (np.isfinite(tp[0]) and tp[3] == 0 and tp[0] < cur[0]):
            break
        T, cur, accepted = trial, tp, accepted + 1
    status = 0 if accepted else 1
    inl, s = _score(T, Xa, kb, cam, threshold)
    if accepted and int(inl.sum()) < n_in:
        status, T, cur = 2, T_in, first
        inl, s = _score(T, Xa, kb, cam, threshold)
    final_n = int(inl.sum())
    mask[slot] = inl
    rms = float(np.sqrt(_tree_sum(np.where(inl, s, 0.0)) / np.float64(final_n))) if final_n else 0.0
    return dict(T=np.array(T, dtype=np.float64), status=status, iterations=accepted, selected_count=n_sel, usable_count=n, inlier_count_in=n_in,
                inlier_count=final_n, inlier_of_slot=mask, cost_in=float(first[0]), cost=float(cur[0]), rms=rms, info=np.array(cur[1]),
                weight_sum=weight_sum)
