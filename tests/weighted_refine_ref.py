"""A float64 numpy restatement of the two entries of libsslam_weight.so, written from the contract in include/sslam_weight.h:
sslu_match_weights (match_weights) and sslu_pose_refine_weighted_pairs (refine / refine_pairs).  The weighted refinement is
pose_refine_ref's restatement with the header's five differences: the row terms (pose_refine_ref.row_terms gives rho, w, the residual
and the Jacobian), the 6 x 6 solve, the update, the summation tree and the usable rows and the score are IMPORTED from
tests/pose_refine_ref.py and tests/pose_ransac_ref.py, not written again; what is written here is the selection by weight, the
product gw = g * w in front of every term, the weight sum and the keep rule against the geometric count.

Tolerance: NONE, for the reason pose_ransac_ref gives: both sides take the same correctly rounded + - * / sqrt in one order.

plain_weighted_refine() is an INDEPENDENT implementation of the same mathematics - np.linalg.solve, np.sum, matrix products -
and finite_difference_gradient() differentiates the weighted cost numerically; tests/test_weighted_refine_cpu.py holds the
restatement to both.
"""
from __future__ import annotations

import numpy as np

import pose_refine_ref as fr
from pose_ransac_ref import score, tree_sum, usable_rows
from pose_refine_ref import TRIU, row_terms, solve, update

PRODUCT, EXPECTED_ERROR = 0, 1
KEYS = fr.KEYS + ("weight_sum",)
SHARED = fr.KEYS
SCALED = ("cost_in", "cost", "info", "weight_sum")      # what a power-of-two scaling of the weights scales; the rest keeps its bytes


# ------------------------------------------------------------------------------------------------------------- match weights
def weight_of(c1, c2, mode, sigma0=1.0):
    """Confidences c1, c2 (fp32 arrays of one shape) -> the weight (fp32): the header's two forms."""
    c1, c2 = np.asarray(c1, np.float32), np.asarray(c2, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if mode == PRODUCT:
            return (c1 * c2).astype(np.float32)
        if mode != EXPECTED_ERROR:
            raise ValueError(mode)
        s0 = np.float64(sigma0)
        s2 = s0 * s0
        e1 = np.float64(1.0) / (c1.astype(np.float64) + np.float64(1e-6)) - np.float64(1.0)
        e2 = np.float64(1.0) / (c2.astype(np.float64) + np.float64(1e-6)) - np.float64(1.0)
        return (s2 / ((s2 + e1 * e1) + e2 * e2)).astype(np.float32)


def match_weights(conf_bank, first, second, matches, count, mode, sigma0=1.0):
    """conf_bank (n_bank, K) fp32, the pair lists, matches (P, n1, 2) int64, count (P,) -> weight (P, n1) fp32, every element set."""
    n_bank, K = conf_bank.shape
    P, n1 = matches.shape[:2]
    out = np.zeros((P, n1), np.float32)
    for p, (a, b) in enumerate(zip(first, second)):
        if not (0 <= a < n_bank and 0 <= b < n_bank):
            continue
        c = int(np.clip(count[p], 0, n1))
        i1, i2 = matches[p, :c, 0], matches[p, :c, 1]
        ok = (i1 >= 0) & (i1 < K) & (i2 >= 0) & (i2 < K)
        out[p, :c][ok] = weight_of(conf_bank[a][i1[ok]], conf_bank[b][i2[ok]], mode, sigma0)
    return out


def weight_ok(g):
    """g > 0 && g - g == 0 in fp32: finite and positive, subnormals included."""
    g = np.asarray(g, np.float32)
    return (g > 0) & np.isfinite(g)


# ------------------------------------------------------------------------------------------------------------------- a pass
def weighted_terms(T, Xa, kb, g, cam, sx, sy, huber):
    """The 28 terms (n, 28) of every row under T with the weights g (n,) fp32, and the row's d and Z2 (row_terms' own)."""
    rt = row_terms(T, Xa, kb, cam, sx, sy, huber)
    gd = g.astype(np.float64)
    Ju, Jv = [rt["J"][:, 0, i] for i in range(6)], [rt["J"][:, 1, i] for i in range(6)]
    rx, ry = rt["r"][:, 0], rt["r"][:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        gw = gd * rt["w"]
        cols = [gd * rt["terms"][:, 0]] + [gw * (Ju[i] * Ju[j] + Jv[i] * Jv[j]) for i, j in TRIU] + [gw * (Ju[i] * rx + Jv[i] * ry) for i in range(6)]
    return np.stack(cols, axis=1), rt


def one_pass(T, Xa, kb, g, sel, cam, sx, sy, huber):
    terms, rt = weighted_terms(T, Xa, kb, g, cam, sx, sy, huber)
    tot = tree_sum(np.where(sel[:, None], terms, 0.0))
    return dict(cost=tot[0], H=tot[1:22], g=tot[22:28], behind=int((sel & ~(rt["Z2"] > 0.0)).sum()), d=rt["d"][sel], Z2=rt["Z2"][sel])


# ------------------------------------------------------------------------------------------------------------------- a pair
def not_attempted(T_in, n1, listed=0, usable_slots=()):
    return dict(fr.not_attempted(T_in, n1, listed, usable_slots), weight_sum=0.0)


def refine(kp_a, kp_b, d_a, d_b, matches, count, weight, cam, threshold, huber, n_iter, T_in, sx=1.0, sy=1.0, detail=False):
    """One present pair with the weights `weight` (n1,) fp32 of its slots: dict of KEYS; with detail also pose_refine_ref's log."""
    n1 = len(matches)
    T_in = np.asarray(T_in, dtype=np.float64).reshape(12)
    rows = usable_rows(kp_a, kp_b, d_a, d_b, matches, count, cam, sx, sy)
    Xa, kb = rows["Xa"], rows["kb"]
    n = len(rows["slot"])
    g = np.asarray(weight, np.float32)[rows["slot"]] if n else np.zeros(0, np.float32)
    log = dict(score_d=[], score_z=[], pass_d=[], pass_z=[], cost_gap=[], pivots=[])
    geo = np.zeros(n, bool)
    if n:
        sc = score(T_in[None], Xa, kb, cam, sx, sy, threshold)
        geo = sc["inlier"][0]
        if np.isfinite(T_in).all():
            log["score_d"].append(sc["d"][0])
            log["score_z"].append(sc["Z2"][0])
    sel = geo & weight_ok(g)
    n_in, n_sel = int(geo.sum()), int(sel.sum())
    if n_sel < 3:
        out = not_attempted(T_in, n1, rows["listed"], rows["slot"])
        if detail:
            out.update(log=log, rows=rows, selected=sel)
        return out
    weight_sum = float(tree_sum(np.where(sel, g.astype(np.float64), 0.0)))
    cur = one_pass(T_in, Xa, kb, g, sel, cam, sx, sy, huber)
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
        tp = one_pass(trial, Xa, kb, g, sel, cam, sx, sy, huber)
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
        if int(sc["inlier"].sum()) < n_in:
            status, T, cur = 2, T_in, first
            sc = score(T[None], Xa, kb, cam, sx, sy, threshold)
    inl = sc["inlier"][0]
    final_n = int(inl.sum())
    mask = np.zeros(n1, np.int32)
    mask[:rows["listed"]] = -1
    mask[rows["slot"]] = inl
    rms = float(np.sqrt(tree_sum(np.where(inl, sc["s"][0], 0.0)) / np.float64(final_n))) if final_n else 0.0
    out = dict(T=T.copy(), status=status, iterations=accepted, selected_count=n_sel, usable_count=n, inlier_count_in=n_in,
               inlier_count=final_n, inlier_of_slot=mask, cost_in=float(first["cost"]), cost=float(cur["cost"]), rms=rms, info=cur["H"].copy(),
               weight_sum=weight_sum)
    if detail:
        out.update(log=log, rows=rows, selected=sel, g=cur["g"].copy(), row_weight=g)
    return out


def refine_pairs(bank, depth_bank, first, second, matches, count, weight, cam, threshold, huber, n_iter, T_in, sx=1.0, sy=1.0, detail=False):
    """The listed pairs of a bank with weight (P, n1) fp32: a list of refine() dicts (an absent pair: not attempted, the whole mask 0)."""
    out = []
    for p, (a, b) in enumerate(zip(first, second)):
        if not (0 <= a < len(bank) and 0 <= b < len(bank)):
            out.append(not_attempted(T_in[p], matches.shape[1]))
            if detail:
                out[-1].update(log=None)
        else:
            out.append(refine(bank[a], bank[b], depth_bank[a], depth_bank[b], matches[p], count[p], weight[p], cam, threshold, huber, n_iter,
                              T_in[p], sx, sy, detail))
    return out


def stacked(results) -> dict:
    """A list of refine() dicts as the arrays the device writes."""
    dt = dict(T=np.float64, cost_in=np.float64, cost=np.float64, rms=np.float64, info=np.float64, weight_sum=np.float64)
    return {key: np.stack([np.asarray(r[key], dtype=dt.get(key, np.int32)) for r in results]) for key in KEYS}


# ------------------------------------------------------------------------------------------- the independent implementation
def plain_weighted_cost(T, Xa, kb, g, cam, sx, sy, huber) -> float:
    """sum g * rho over the rows, written the plain way."""
    r, _ = fr._plain_residuals(T, Xa, kb, cam, sx, sy)
    d = np.linalg.norm(r, axis=1)
    return float(np.sum(g * np.where(d <= huber, d * d, 2.0 * huber * d - huber * huber)))


def plain_weighted_normal_equations(T, Xa, kb, g, cam, sx, sy, huber):
    """(cost, H (6, 6), g (6,)) from per-row matrix products, every row's J^T J and J^T r scaled by its weight times Huber's."""
    r, Xc = fr._plain_residuals(T, Xa, kb, cam, sx, sy)
    d = np.linalg.norm(r, axis=1)
    w = g * np.where(d <= huber, 1.0, huber / np.maximum(d, 1e-300))
    H, grad = np.zeros((6, 6)), np.zeros(6)
    for i in range(len(Xa)):
        x, y, z = Xc[i]
        P = np.array([[cam.fx / (sx * z), 0.0, -cam.fx * x / (sx * z * z)], [0.0, cam.fy / (sy * z), -cam.fy * y / (sy * z * z)]])
        J = P @ np.hstack([np.eye(3), -fr._skew(Xc[i])])
        H += w[i] * (J.T @ J)
        grad += w[i] * (J.T @ r[i])
    return plain_weighted_cost(T, Xa, kb, g, cam, sx, sy, huber), H, grad


def plain_weighted_refine(Xa, kb, g, cam, sx, sy, huber, n_iter, T_in):
    """Weighted Gauss-Newton with the restatement's acceptance on ALREADY SELECTED rows and their float64 weights g:
    (T, cost_in, cost, H (6, 6), accepted)."""
    T = np.asarray(T_in, dtype=np.float64).reshape(12)
    g = np.asarray(g, dtype=np.float64)
    cost, H, grad = plain_weighted_normal_equations(T, Xa, kb, g, cam, sx, sy, huber)
    cost_in, accepted = cost, 0
    for _ in range(n_iter):
        try:
            np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            break
        trial = fr.plain_update(T, np.linalg.solve(H, -grad))
        c2, H2, g2 = plain_weighted_normal_equations(trial, Xa, kb, g, cam, sx, sy, huber)
        if not (np.isfinite(c2) and (fr._plain_residuals(trial, Xa, kb, cam, sx, sy)[1][:, 2] > 0).all() and c2 < cost):
            break
        T, cost, H, grad, accepted = trial, c2, H2, g2, accepted + 1
    return T, cost_in, cost, H, accepted


def finite_difference_gradient(T, Xa, kb, g, cam, sx, sy, huber, step=1e-6):
    """d(1/2 sum g rho)/d(delta) at delta = 0 by central differences through pose_refine_ref.plain_update: (6,)."""
    out = np.zeros(6)
    for i in range(6):
        e = np.zeros(6)
        e[i] = step
        out[i] = (plain_weighted_cost(fr.plain_update(T, e), Xa, kb, g, cam, sx, sy, huber) -
                  plain_weighted_cost(fr.plain_update(T, -e), Xa, kb, g, cam, sx, sy, huber)) / (4 * step)
    return out
