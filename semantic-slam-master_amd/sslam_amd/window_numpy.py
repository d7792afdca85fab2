"""The sliding-window estimator of include/sslam_window.h in numpy float64, for a caller without the GPU: what evaluation.PoseWindow
runs.  It is written from the two headers (sslam_graph.h: poses, edges, the cost's summation tree, the normal equations, the
unpivoted LDL^T, the update, the iteration; sslam_window.h: the ring, the admission, the prediction, the write-back), one numpy
float64 operation per operation named there, in the order written - so a step gives the bits sslw_window_step gives
(tests/test_window_cpu.py holds it to the tests' own restatement, which the device is held to).  It is no fallback: nothing in the
package calls it in place of a kernel.  Edges are handled one at a time in Python: a window has at most 256 slots."""
from __future__ import annotations

import numpy as np

MAX_WINDOW, MAX_SPACINGS, MAX_FRAME, MAX_ITER = 32, 8, 2 ** 31 - 2, 16
OUT_KEYS = ("C_window", "base", "n_nodes", "admitted", "predicted_from", "lost", "status", "iterations", "used_edges", "dropped_edges",
            "failed_row", "cost_in", "cost", "edge_chi2")
IDENTITY = np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
_ERR = dict(divide="ignore", invalid="ignore", over="ignore")
_TRI = {}           # (i, j), either triangle -> the word of info's row-major upper triangle
for _k, (_i, _j) in enumerate((i, j) for i in range(6) for j in range(i, 6)):
    _TRI[(_i, _j)] = _TRI[(_j, _i)] = _k


def compose(A, B):
    """A o B (first B, then A) of two poses (12,)."""
    out = np.empty(12)
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]
        out[4 * i + 3] = ((A[4 * i] * B[3] + A[4 * i + 1] * B[7]) + A[4 * i + 2] * B[11]) + A[4 * i + 3]
    return out


def inverse(A):
    out = np.empty(12)
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = A[4 * j + i]
        out[4 * i + 3] = -((A[i] * A[3] + A[4 + i] * A[7]) + A[8 + i] * A[11])
    return out


def _sum6(x):
    return ((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]


def _edge(Ca, Cb, Tm, info, chi):
    """AN EDGE of sslam_graph.h at the poses: (T_p, H 6 x 6, Hr, s, w, rho)."""
    Tp = compose(Cb, inverse(Ca))
    D = compose(Tp, inverse(Tm))
    half = np.float64(0.5)
    r = [D[3], D[7], D[11], half * (D[9] - D[6]), half * (D[2] - D[8]), half * (D[4] - D[1])]
    H = [[info[_TRI[(i, j)]] for j in range(6)] for i in range(6)]
    Hr = [_sum6([H[i][k] * r[k] for k in range(6)]) for i in range(6)]
    s = _sum6([r[k] * Hr[k] for k in range(6)])
    if s <= chi * chi:
        return Tp, H, Hr, s, np.float64(1.0), s
    q = np.sqrt(s)
    return Tp, H, Hr, s, chi / q, (np.float64(2.0) * chi) * q - chi * chi


def _tree(rho):
    """The cost's sum over at most 256 slots: thread t holds slot t, lanes by xor 32 .. 1, the four waves ((w0 + w1) + w2) + w3."""
    v = np.zeros(256)
    v[:len(rho)] = rho
    v = v.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[:, :o] + v[:, o:2 * o]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def _cost(used, a, b, T, info, C, chi):
    rho, s = np.zeros(len(used)), np.zeros(len(used))
    for e in np.flatnonzero(used):
        _, _, _, s[e], _, rho[e] = _edge(C[a[e]], C[b[e]], T[e], info[e], chi)
    return _tree(rho), s


def _normal_equations(used, a, b, T, info, C, chi, damping):
    n = 6 * (len(C) - 1)
    A, g = np.zeros((n, n)), np.zeros(n)
    zero = np.float64(0.0)
    for e in np.flatnonzero(used):                               # ascending slot order
        m, H, Hr, _, w, _ = _edge(C[a[e]], C[b[e]], T[e], info[e], chi)
        Ad = [[zero] * 6 for _ in range(6)]
        for i in range(3):
            for j in range(3):
                Ad[i][j] = Ad[3 + i][3 + j] = m[4 * i + j]
        for j in range(3):
            Ad[0][3 + j] = m[7] * m[8 + j] - m[11] * m[4 + j]
            Ad[1][3 + j] = m[11] * m[j] - m[3] * m[8 + j]
            Ad[2][3 + j] = m[3] * m[4 + j] - m[7] * m[j]
        P = [[_sum6([H[i][k] * Ad[k][j] for k in range(6)]) for j in range(6)] for i in range(6)]
        rb, ra = 6 * (b[e] - 1), 6 * (a[e] - 1)
        for i in range(6):
            for j in range(i + 1):
                A[rb + i, rb + j] = A[rb + i, rb + j] + w * H[i][j]
            g[rb + i] = g[rb + i] + w * Hr[i]
        if a[e] >= 1:
            for i in range(6):
                for j in range(6):
                    A[rb + i, ra + j] = A[rb + i, ra + j] + (-(w * P[i][j]))
                for j in range(i + 1):
                    A[ra + i, ra + j] = A[ra + i, ra + j] + w * _sum6([Ad[k][i] * P[k][j] for k in range(6)])
                g[ra + i] = g[ra + i] + (-(w * _sum6([Ad[k][i] * Hr[k] for k in range(6)])))
    for i in range(n):
        A[i, i] = A[i, i] + damping
    return A, g


def _solve(A, g):
    """SOLVE of sslam_graph.h where the band holds every row: (delta, -1) or (None, the row of the failed pivot).  Right-looking on
    the lower triangle: an element takes the updates of the statement in the statement's ascending k."""
    n = len(g)
    L, y = A.copy(), -g
    for j in range(n):
        d = L[j, j]
        if not (d > 0.0 and np.isfinite(d)):
            return None, j
        col = L[j + 1:, j] / d
        L[j + 1:, j] = col
        L[j + 1:, j + 1:] -= (col[:, None] * col[None, :]) * d
        y[j + 1:] -= col * y[j]
    delta = np.zeros(n)
    for i in range(n - 1, -1, -1):
        v = y[i] / L[i, i]
        for p in L[i + 1:, i] * delta[i + 1:]:
            v = v - p
        delta[i] = v
    return delta, -1


def _update(m, delta):
    """UPDATE of sslam_graph.h: [R | t] <- [dR R | dR t + v], dR from the unit quaternion of (1, wx / 2, wy / 2, wz / 2)."""
    half, two = np.float64(0.5), np.float64(2.0)
    w, x, y, z = np.float64(1.0), half * delta[3], half * delta[4], half * delta[5]
    nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    R = [((ww + xx) - yy) - zz, two * (x * y - w * z), two * (x * z + w * y),
         two * (x * y + w * z), ((ww - xx) + yy) - zz, two * (y * z - w * x),
         two * (x * z - w * y), two * (y * z + w * x), ((ww - xx) - yy) + zz]
    out = np.empty(12)
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (R[3 * i] * m[j] + R[3 * i + 1] * m[4 + j]) + R[3 * i + 2] * m[8 + j]
        out[4 * i + 3] = ((R[3 * i] * m[3] + R[3 * i + 1] * m[7]) + R[3 * i + 2] * m[11]) + delta[i]
    return out


def optimize(first, second, T, info, C_in, band, chi, damping, n_iter) -> dict:
    """sslg_pose_graph's statement on one graph of at most 256 slots whose band holds every row."""
    a, b = np.asarray(first, np.int64), np.asarray(second, np.int64)
    n_nodes = len(C_in)
    assert len(a) <= 256 and band >= n_nodes - 1
    chi, damping = np.float64(chi), np.float64(damping)
    with np.errstate(**_ERR):
        used = (0 <= a) & (a < b) & (b < n_nodes) & (b - a <= band) & np.isfinite(T).all(axis=1) & np.isfinite(info).all(axis=1)
        out = dict(C=C_in.copy(), status=3, iterations=0, used_edges=int(used.sum()), skipped_edges=int((~used & (a != -1)).sum()), failed_row=-1,
                   cost_in=0.0, cost=0.0, edge_chi2=np.zeros(len(a)))
        if not used.any() or not np.isfinite(C_in).all():
            return out
        cur = C_in.copy()
        cost_in, _ = _cost(used, a, b, T, info, cur, chi)
        cost, accepted, failed, first_failed = cost_in, 0, -1, False
        for it in range(n_iter):
            delta, fail = _solve(*_normal_equations(used, a, b, T, info, cur, chi, damping))
            if fail >= 0:
                failed, first_failed = fail, it == 0
                break
            trial = np.stack([cur[0]] + [_update(cur[m], delta[6 * (m - 1):6 * m]) for m in range(1, n_nodes)])
            c_trial, _ = _cost(used, a, b, T, info, trial, chi)
            if not (np.isfinite(c_trial) and c_trial < cost):
                break
            cur, cost, accepted = trial, c_trial, accepted + 1
        _, s = _cost(used, a, b, T, info, cur, chi)
    out.update(C=cur, status=0 if accepted else (2 if first_failed else 1), iterations=accepted, failed_row=failed, cost_in=float(cost_in),
               cost=float(cost), edge_chi2=s)
    return out


def fresh_state(window: int, n_spacings: int, capacity: int) -> dict:
    ws = window * n_spacings
    return dict(t=np.zeros((), np.int32), ring_first=np.full(ws, -1, np.int32), ring_second=np.zeros(ws, np.int32), ring_T=np.zeros((ws, 12)),
                ring_info=np.zeros((ws, 21)), ring_C=np.zeros((window, 12)), trajectory=np.zeros((capacity, 12)))


def step(state, spacings, T, info, status, inliers, C_start, min_inliers, chi, damping, n_iter) -> dict:
    """THE STEP of sslam_window.h on one window: `state` is updated in place -> the outputs by name (status 4: `status` alone)."""
    t = int(state["t"])
    if not 0 <= t <= MAX_FRAME:
        return dict(status=np.int32(4))
    W, S = len(state["ring_C"]), len(spacings)
    base = max(0, t - W + 1)
    nn, row = t - base + 1, t % W
    admitted = np.zeros(S, np.int32)
    for k in range(S):
        a = t - int(spacings[k])
        ok = base <= a < t and int(status[k]) != 3 and int(inliers[k]) >= min_inliers and bool(np.isfinite(T[k]).all() and np.isfinite(info[k]).all())
        slot = row * S + k
        admitted[k] = ok
        state["ring_first"][slot], state["ring_second"][slot] = (a if ok else -1), t
        state["ring_T"][slot] = T[k] if ok else 0.0
        state["ring_info"][slot] = info[k] if ok else 0.0
    ring_C, ks = state["ring_C"], -1
    if t == 0:
        cur = IDENTITY.copy() if C_start is None else np.array(C_start, np.float64).reshape(12)
    else:
        for k in range(S):
            if admitted[k] and (ks < 0 or int(spacings[k]) < int(spacings[ks])):
                ks = k
        with np.errstate(**_ERR):
            cur = compose(T[ks], ring_C[(t - int(spacings[ks])) % W]) if ks >= 0 else ring_C[(t - 1) % W].copy()
    ring_C[row] = cur
    rf = state["ring_first"].astype(np.int64)
    first = np.where(rf == -1, -1, np.where(rf < base, -2, rf - base))
    rows = [(base + i) % W for i in range(nn)]
    r = optimize(first, state["ring_second"].astype(np.int64) - base, state["ring_T"], state["ring_info"], ring_C[rows], W - 1, chi, damping, n_iter)
    C_window = np.zeros((W, 12))
    C_window[:nn] = r["C"]
    ring_C[rows] = r["C"]
    for i in range(nn):
        if base + i < len(state["trajectory"]):
            state["trajectory"][base + i] = r["C"][i]
    state["t"][...] = t + 1
    out = dict(C_window=C_window, base=base, n_nodes=nn, admitted=admitted, predicted_from=ks, lost=int(t > 0 and ks < 0), status=r["status"],
               iterations=r["iterations"], used_edges=r["used_edges"], dropped_edges=r["skipped_edges"], failed_row=r["failed_row"],
               cost_in=r["cost_in"], cost=r["cost"], edge_chi2=r["edge_chi2"])
    real = ("C_window", "cost_in", "cost", "edge_chi2")
    return {k: np.asarray(out[k], dtype=np.float64 if k in real else np.int32) for k in OUT_KEYS}
