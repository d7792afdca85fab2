"""A float64 numpy restatement of sslam_pose_refine_pairs (csrc/pose_refine.hip), written from the contract in include/sslam_hip.h:
the usable rows and the selection (pose_ransac_ref's own usable_rows and score), a row's residual, Huber weight and Jacobian, the
pass with the refit's summation tree (pose_ransac_ref.tree_sum), the unpivoted LDL^T, the quaternion update, the acceptance and
the keep rule.  It is vectorised over rows, and every elementwise operation is one numpy float64 operation in the header's order;
nothing the device computes goes through np.dot, @, np.sum or np.linalg.  The 6 x 6 solve is scalar np.float64 arithmetic.

Tolerance: NONE, for the reason pose_ransac_ref gives: both sides take the same correctly rounded + - * / sqrt in one order.

plain_refine() is an INDEPENDENT implementation of the same mathematics - np.linalg.solve, np.sum, matrix products, its own
Jacobian from the chain rule - and finite_difference_gradient() differentiates the cost numerically; tests/test_pose_refine_cpu.py
holds the restatement to both.

margins() gives what tests/pose_refine_cases.py holds its cases to: how far the restatement stays from every decision it takes.
"""
from __future__ import annotations

import numpy as np

from pose_ransac_ref import Cam, pose_error, rigid, rotation, score, tree_sum, usable_rows  # noqa: F401  (the case lists use them)

MAX_ITER = 16
KEYS = ("T", "status", "iterations", "selected_count", "usable_count", "inlier_count_in", "inlier_count", "inlier_of_slot", "cost_in",
        "cost", "rms", "info")
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]      # the 21 entries of H, row-major


# ---------------------------------------------------------------------------------------------------------------------- a row
def row_terms(T, Xa, kb, cam, sx, sy, huber):
    """Rows Xa (n, 3), kb (n, 2) fp32 under the pose T (12,): dict of terms (n, 28) - rho, the 21 of H, the 6 of g - and r (n, 2), d,
    w, Z2, J (n, 2, 6)."""
    fx, fy, cx, cy = (np.float64(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    sx, sy, huber = np.float64(sx), np.float64(sy), np.float64(huber)
    m = [np.float64(v) for v in T]
    X, Y, Z = Xa[:, 0], Xa[:, 1], Xa[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        kx, ky = fx / sx, fy / sy
        X2 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
        Y2 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
        Z2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
        u2, v2 = (fx * X2) / Z2 + cx, (fy * Y2) / Z2 + cy
        rx, ry = u2 / sx - kb[:, 0].astype(np.float64), v2 / sy - kb[:, 1].astype(np.float64)
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
        cols = [rho] + [w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]) for i, j in TRIU] + [w * (Ju[i] * rx + Jv[i] * ry) for i in range(6)]
    return dict(terms=np.stack(cols, axis=1), r=np.stack([rx, ry], axis=1), d=d, w=w, Z2=Z2, J=np.stack([np.stack(Ju, axis=1), np.stack(Jv, axis=1)], axis=1))


def one_pass(T, Xa, kb, sel, cam, sx, sy, huber):
    """The pass at T over the selected rows sel (n,) bool of the usable rows: dict of cost, H (21,), g (6,), behind, and the rows' d, Z2."""
    rt = row_terms(T, Xa, kb, cam, sx, sy, huber)
    tot = tree_sum(np.where(sel[:, None], rt["terms"], 0.0))
    return dict(cost=tot[0], H=tot[1:22], g=tot[22:28], behind=int((sel & ~(rt["Z2"] > 0.0)).sum()), d=rt["d"][sel], Z2=rt["Z2"][sel])


# --------------------------------------------------------------------------------------------------------------------- a step
def solve(H, g):
    """H delta = -g by the header's unpivoted LDL^T: (delta (6,), ok, pivots (6,)); ok is False at a pivot that is not finite and > 0."""
    h = {}
    for (i, j), v in zip(TRIU, H):
        h[(i, j)] = h[(j, i)] = np.float64(v)
    L = [[None] * 6 for _ in range(6)]
    D, y, delta = [None] * 6, [None] * 6, [None] * 6
    ok = True
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
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
            v = -np.float64(g[i])
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = v
        for i in range(5, -1, -1):
            v = y[i] / D[i]
            for k in range(i + 1, 6):
                v = v - L[k][i] * delta[k]
            delta[i] = v
    return np.array(delta, dtype=np.float64), ok, np.array(D, dtype=np.float64)


def update(T, delta):
    """[R | t] <- [dR R | dR t + v], dR from the unit quaternion of (1, wx / 2, wy / 2, wz / 2): (12,)."""
    m = [np.float64(v) for v in T]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
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


# --------------------------------------------------------------------------------------------------------------------- a pair
def not_attempted(T_in, n1, listed=0, usable_slots=()):
    mask = np.zeros(n1, np.int32)
    mask[:listed] = -1
    mask[list(usable_slots)] = 0
    return dict(T=np.array(T_in, dtype=np.float64).copy(), status=3, iterations=0, selected_count=0, usable_count=0, inlier_count_in=0,
                inlier_count=0, inlier_of_slot=mask, cost_in=0.0, cost=0.0, rms=0.0, info=np.zeros(21))


def refine(kp_a, kp_b, d_a, d_b, matches, count, cam, threshold, huber, n_iter, T_in, sx=1.0, sy=1.0, detail=False):
    """One present pair: dict of KEYS; with detail also `log` - every quantity a decision was taken on (margins() reads it) - the
    rows and the selection."""
    n1 = len(matches)
    T_in = np.asarray(T_in, dtype=np.float64).reshape(12)
    rows = usable_rows(kp_a, kp_b, d_a, d_b, matches, count, cam, sx, sy)
    Xa, kb = rows["Xa"], rows["kb"]
    n = len(rows["slot"])
    log = dict(score_d=[], score_z=[], pass_d=[], pass_z=[], cost_gap=[], pivots=[])
    sel = np.zeros(n, bool)
    if n:
        sc = score(T_in[None], Xa, kb, cam, sx, sy, threshold)
        sel = sc["inlier"][0]
        if np.isfinite(T_in).all():
            log["score_d"].append(sc["d"][0])
            log["score_z"].append(sc["Z2"][0])
    n_sel = int(sel.sum())
    if n_sel < 3:
        out = not_attempted(T_in, n1, rows["listed"], rows["slot"])
        if detail:
            out.update(log=log, rows=rows, selected=sel)
        return out
    cur = one_pass(T_in, Xa, kb, sel, cam, sx, sy, huber)
    first = cur
    log["pass_d"].append(cur["d"])
    log["pass_z"].append(cur["Z2"])
    T, accepted = T_in, 0
    for _ in range(n_iter):
        delta, ok, piv = solve(cur["H"], cur["g"])
        log["pivots"].append(piv)
        if not ok:
            break
        trial = update(T, delta)
        tp = one_pass(trial, Xa, kb, sel, cam, sx, sy, huber)
        log["pass_d"].append(tp["d"])
        log["pass_z"].append(tp["Z2"])
        log["cost_gap"].append(tp["cost"] - cur["cost"])
        if not (np.isfinite(tp["cost"]) and tp["behind"] == 0 and tp["cost"] < cur["cost"]):
            break
        T, cur, accepted = trial, tp, accepted + 1
    status = 0 if accepted else 1
    sc = score(T[None], Xa, kb, cam, sx, sy, threshold)
    if accepted:
        if np.isfinite(T).all():
            log["score_d"].append(sc["d"][0])
            log["score_z"].append(sc["Z2"][0])
        if int(sc["inlier"].sum()) < n_sel:
            status, T, cur = 2, T_in, first
            sc = score(T[None], Xa, kb, cam, sx, sy, threshold)
    inl = sc["inlier"][0]
    final_n = int(inl.sum())
    mask = np.zeros(n1, np.int32)
    mask[:rows["listed"]] = -1
    mask[rows["slot"]] = inl
    rms = float(np.sqrt(tree_sum(np.where(inl, sc["s"][0], 0.0)) / np.float64(final_n))) if final_n else 0.0
    out = dict(T=T.copy(), status=status, iterations=accepted, selected_count=n_sel, usable_count=n, inlier_count_in=n_sel,
               inlier_count=final_n, inlier_of_slot=mask, cost_in=float(first["cost"]), cost=float(cur["cost"]), rms=rms, info=cur["H"].copy())
    if detail:
        out.update(log=log, rows=rows, selected=sel, g=cur["g"].copy())
    return out


def refine_pairs(bank, depth_bank, first, second, matches, count, cam, threshold, huber, n_iter, T_in, sx=1.0, sy=1.0, detail=False):
    """The listed pairs of a bank: a list of refine() dicts (an absent pair: not attempted, the whole mask 0)."""
    out = []
    for p, (a, b) in enumerate(zip(first, second)):
        if not (0 <= a < len(bank) and 0 <= b < len(bank)):
            out.append(not_attempted(T_in[p], matches.shape[1]))
            if detail:
                out[-1].update(log=None)
        else:
            out.append(refine(bank[a], bank[b], depth_bank[a], depth_bank[b], matches[p], count[p], cam, threshold, huber, n_iter, T_in[p],
                              sx, sy, detail))
    return out


def stacked(results) -> dict:
    """A list of refine() dicts as the arrays the device writes."""
    dt = dict(T=np.float64, cost_in=np.float64, cost=np.float64, rms=np.float64, info=np.float64)
    return {key: np.stack([np.asarray(r[key], dtype=dt.get(key, np.int32)) for r in results]) for key in KEYS}


def margins(log, threshold, huber) -> dict:
    """From a refine(detail=True) log, the least distance of the run from each decision it took (inf where none was taken):
    edge   |d - threshold| over the usable rows with Z' > 0, at the selection and at the final rescoring;
    huber  |d - huber| over the selected rows, every pass;
    z      |Z'| over the rows of the selection, the rescoring and every pass;
    cost   |cost_trial - cost| over the trials;
    pivot  the least pivot of every factorisation that went through, the distance from 0 of one that did not."""
    out = dict(edge=np.inf, huber=np.inf, z=np.inf, cost=np.inf, pivot=np.inf)
    if log is None:
        return out
    for d, z in zip(log["score_d"], log["score_z"]):
        front = z > 0
        if front.any():
            out["edge"] = min(out["edge"], float(np.min(np.abs(d[front] - threshold))))
        out["z"] = min(out["z"], float(np.min(np.abs(z))))
    for d, z in zip(log["pass_d"], log["pass_z"]):
        if np.isfinite(d).all():
            out["huber"] = min(out["huber"], float(np.min(np.abs(d - huber))))
            out["z"] = min(out["z"], float(np.min(np.abs(z))))
    for gap in log["cost_gap"]:
        if np.isfinite(gap):
            out["cost"] = min(out["cost"], float(abs(gap)))
    for piv in log["pivots"]:
        bad = np.where(~((piv > 0) & np.isfinite(piv)))[0]
        seen = piv if len(bad) == 0 else piv[:bad[0] + 1]
        seen = seen[np.isfinite(seen)]
        if len(seen):
            out["pivot"] = min(out["pivot"], float(np.min(np.abs(seen))))
    return out


# ------------------------------------------------------------------------------------------- the independent implementation
def _plain_residuals(T, Xa, kb, cam, sx, sy):
    m = np.asarray(T, dtype=np.float64).reshape(3, 4)
    Xc = Xa @ m[:, :3].T + m[:, 3]
    proj = np.stack([(cam.fx * Xc[:, 0] / Xc[:, 2] + cam.cx) / sx, (cam.fy * Xc[:, 1] / Xc[:, 2] + cam.cy) / sy], axis=1)
    return proj - kb.astype(np.float64), Xc


def plain_cost(T, Xa, kb, cam, sx, sy, huber) -> float:
    """sum rho over the rows, written the plain way."""
    r, _ = _plain_residuals(T, Xa, kb, cam, sx, sy)
    d = np.linalg.norm(r, axis=1)
    return float(np.sum(np.where(d <= huber, d * d, 2.0 * huber * d - huber * huber)))


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def plain_normal_equations(T, Xa, kb, cam, sx, sy, huber):
    """(cost, H (6, 6), g (6,)) from per-row matrix products: J = dproj/dX' (2 x 3) @ [I | -[X']x]."""
    r, Xc = _plain_residuals(T, Xa, kb, cam, sx, sy)
    d = np.linalg.norm(r, axis=1)
    w = np.where(d <= huber, 1.0, huber / np.maximum(d, 1e-300))
    H, g = np.zeros((6, 6)), np.zeros(6)
    for i in range(len(Xa)):
        x, y, z = Xc[i]
        P = np.array([[cam.fx / (sx * z), 0.0, -cam.fx * x / (sx * z * z)], [0.0, cam.fy / (sy * z), -cam.fy * y / (sy * z * z)]])
        J = P @ np.hstack([np.eye(3), -_skew(Xc[i])])
        H += w[i] * (J.T @ J)
        g += w[i] * (J.T @ r[i])
    return plain_cost(T, Xa, kb, cam, sx, sy, huber), H, g


def plain_update(T, delta):
    m = np.asarray(T, dtype=np.float64).reshape(3, 4)
    q = np.array([1.0, delta[3] / 2, delta[4] / 2, delta[5] / 2])
    w, x, y, z = q / np.linalg.norm(q)
    dR = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return np.hstack([dR @ m[:, :3], (dR @ m[:, 3] + delta[:3])[:, None]]).reshape(12)


def plain_refine(Xa, kb, cam, sx, sy, huber, n_iter, T_in):
    """Gauss-Newton with the restatement's acceptance on ALREADY SELECTED rows: (T, cost_in, cost, H (6, 6), accepted)."""
    T = np.asarray(T_in, dtype=np.float64).reshape(12)
    cost, H, g = plain_normal_equations(T, Xa, kb, cam, sx, sy, huber)
    cost_in, accepted = cost, 0
    for _ in range(n_iter):
        try:
            np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            break
        trial = plain_update(T, np.linalg.solve(H, -g))
        c2, H2, g2 = plain_normal_equations(trial, Xa, kb, cam, sx, sy, huber)
        if not (np.isfinite(c2) and (_plain_residuals(trial, Xa, kb, cam, sx, sy)[1][:, 2] > 0).all() and c2 < cost):
            break
        T, cost, H, g, accepted = trial, c2, H2, g2, accepted + 1
    return T, cost_in, cost, H, accepted


def finite_difference_gradient(T, Xa, kb, cam, sx, sy, huber, step=1e-6):
    """d(1/2 sum rho)/d(delta) at delta = 0 by central differences through plain_update: (6,)."""
    g = np.zeros(6)
    for i in range(6):
        e = np.zeros(6)
        e[i] = step
        g[i] = (plain_cost(plain_update(T, e), Xa, kb, cam, sx, sy, huber) - plain_cost(plain_update(T, -e), Xa, kb, cam, sx, sy, huber)) / (4 * step)
    return g


def full_info(info):
    """(6, 6) symmetric from the 21 upper-triangle entries."""
    H = np.zeros((6, 6))
    for (i, j), v in zip(TRIU, info):
        H[i, j] = H[j, i] = v
    return H
