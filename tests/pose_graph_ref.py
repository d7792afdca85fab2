"""A float64 numpy restatement of libsslam_graph.so (csrc_graph/pose_graph.hip), written from the contract in include/sslam_graph.h:
the pose products, the used edges, an edge's residual, Huber weight and adjoint, the cost in the pass' summation tree
(pose_ransac_ref.tree_sum), the normal equations accumulated edge by edge in slot order, the banded unpivoted LDL^T, the
quaternion update (pose_refine_ref.update) and the acceptance.  It is vectorised over edges, and every elementwise operation is
one numpy float64 operation in the header's order; nothing the device computes goes through np.dot, @, np.sum or np.linalg.

The factorisation here is RIGHT-looking on a dense lower triangle (column j updates the window behind it), the device's is
left-looking on the band: every element takes the same updates in the same k order, so the bits agree - and an indexing error
in either shows as a difference.  The ordered subtractions of the back substitution go through np.add.accumulate, which is
strictly sequential.

Tolerance: NONE - both sides take the same correctly rounded + - * / sqrt in one order.

plain_normal_equations() is an INDEPENDENT implementation - matrix products, its own Jacobians - for tests/test_pose_graph_cpu.py.
"""
from __future__ import annotations

import numpy as np

from pose_ransac_ref import tree_sum
from pose_refine_ref import update as pose_update

MAX_BAND, MAX_NODES, MAX_EDGES, MAX_GRAPHS, MAX_ITER = 32, 4096, 1048576, 65535, 16
KEYS = ("C", "status", "iterations", "used_edges", "skipped_edges", "failed_row", "cost_in", "cost", "edge_chi2")
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]
_ERR = dict(divide="ignore", invalid="ignore", over="ignore")


# ------------------------------------------------------------------------------------------------------------------- poses
def compose(A, B):
    """A o B (first B, then A) for poses (..., 12)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.empty(np.broadcast(A, B).shape)
    with np.errstate(**_ERR):
        for i in range(3):
            for j in range(3):
                out[..., 4 * i + j] = (A[..., 4 * i] * B[..., j] + A[..., 4 * i + 1] * B[..., 4 + j]) + A[..., 4 * i + 2] * B[..., 8 + j]
            out[..., 4 * i + 3] = ((A[..., 4 * i] * B[..., 3] + A[..., 4 * i + 1] * B[..., 7]) + A[..., 4 * i + 2] * B[..., 11]) + A[..., 4 * i + 3]
    return out


def inverse(A):
    A = np.asarray(A, np.float64)
    out = np.empty(A.shape)
    with np.errstate(**_ERR):
        for i in range(3):
            for j in range(3):
                out[..., 4 * i + j] = A[..., 4 * j + i]
            out[..., 4 * i + 3] = -((A[..., i] * A[..., 3] + A[..., 4 + i] * A[..., 7]) + A[..., 8 + i] * A[..., 11])
    return out


def chain(T, start=None):
    """(n_nodes, 12) world -> camera poses from T (n_nodes - 1, 12): C_0 = start ([I | 0] if None), C_{i+1} = T_i o C_i."""
    T = np.asarray(T, np.float64).reshape(-1, 12)
    cur = np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]) if start is None else np.asarray(start, np.float64).reshape(12).copy()
    out = [cur]
    for t in T:
        out.append(compose(t, out[-1]))
    return np.stack(out)


def _sum6(x):
    return ((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]


# ------------------------------------------------------------------------------------------------------------------- edges
def used_mask(first, second, T, info, n_nodes, band):
    first, second = np.asarray(first, np.int64), np.asarray(second, np.int64)
    ok = (0 <= first) & (first < second) & (second < n_nodes) & (second - first <= band)
    return ok & np.isfinite(T).all(axis=1) & np.isfinite(info).all(axis=1)


def edge_eval(C, a, b, T, info, chi):
    """The edges (a, b (E,), T (E, 12), info (E, 21)) at the poses C (n_nodes, 12): dict of Tp (E, 12), H [6][6] of (E,), r, Hr
    [6] of (E,), s, w, rho (E,)."""
    chi = np.float64(chi)
    with np.errstate(**_ERR):
        Tp = compose(C[b], inverse(C[a]))
        D = compose(Tp, inverse(T))
        half = np.float64(0.5)
        r = [D[:, 3], D[:, 7], D[:, 11], half * (D[:, 9] - D[:, 6]), half * (D[:, 2] - D[:, 8]), half * (D[:, 4] - D[:, 1])]
        H = [[None] * 6 for _ in range(6)]
        for (i, j), col in zip(TRIU, info.T):
            H[i][j] = H[j][i] = col
        Hr = [_sum6([H[i][k] * r[k] for k in range(6)]) for i in range(6)]
        s = _sum6([r[k] * Hr[k] for k in range(6)])
        quad = s <= chi * chi
        q = np.sqrt(s)
        w = np.where(quad, 1.0, chi / q)
        rho = np.where(quad, s, (2.0 * chi) * q - chi * chi)
    return dict(Tp=Tp, H=H, r=r, Hr=Hr, s=s, w=w, rho=rho)


def edge_stage(ev):
    """The staged terms of evaluated edges: BB, BA, AA (E, 6, 6) and GB, GA (E, 6) - what is ADDED to block (b, b), block (b, a),
    block (a, a), g of b and g of a.  Of BB and AA only the lower triangle (i >= j) is the contract's."""
    m, H, Hr, w = ev["Tp"], ev["H"], ev["Hr"], ev["w"]
    E = len(w)
    zero = np.zeros(E)
    with np.errstate(**_ERR):
        Ad = [[None] * 6 for _ in range(6)]
        for i in range(3):
            for j in range(3):
                Ad[i][j] = Ad[3 + i][3 + j] = m[:, 4 * i + j]
                Ad[3 + i][j] = zero
        for j in range(3):
            Ad[0][3 + j] = m[:, 7] * m[:, 8 + j] - m[:, 11] * m[:, 4 + j]
            Ad[1][3 + j] = m[:, 11] * m[:, j] - m[:, 3] * m[:, 8 + j]
            Ad[2][3 + j] = m[:, 3] * m[:, 4 + j] - m[:, 7] * m[:, j]
        P = [[_sum6([H[i][k] * Ad[k][j] for k in range(6)]) for j in range(6)] for i in range(6)]
        BB, BA, AA = np.empty((E, 6, 6)), np.empty((E, 6, 6)), np.empty((E, 6, 6))
        GB, GA = np.empty((E, 6)), np.empty((E, 6))
        for i in range(6):
            for j in range(6):
                BA[:, i, j] = -(w * P[i][j])
                AA[:, i, j] = w * _sum6([Ad[k][i] * P[k][j] for k in range(6)])
                BB[:, i, j] = w * H[i][j]
            GA[:, i] = -(w * _sum6([Ad[k][i] * Hr[k] for k in range(6)]))
            GB[:, i] = w * Hr[i]
    return BB, BA, AA, GB, GA


class Graph:
    """One graph's operands, the used edges picked out once."""

    def __init__(self, first, second, T, info, n_nodes, band):
        self.first, self.second = np.asarray(first, np.int32), np.asarray(second, np.int32)
        self.T, self.info = np.asarray(T, np.float64).reshape(-1, 12), np.asarray(info, np.float64).reshape(-1, 21)
        self.n_nodes, self.band, self.n_edges = int(n_nodes), int(band), len(self.first)
        self.used = used_mask(self.first, self.second, self.T, self.info, n_nodes, band)
        self.slots = np.where(self.used)[0]
        self.a, self.b = self.first[self.slots].astype(np.int64), self.second[self.slots].astype(np.int64)
        self.skipped = int((~self.used & (self.first != -1)).sum())

    def eval(self, C, chi):
        return edge_eval(C, self.a, self.b, self.T[self.slots], self.info[self.slots], chi)

    def cost(self, C, chi, ev=None):
        """(cost, s per slot) at the poses C."""
        ev = self.eval(C, chi) if ev is None else ev
        rho, s = np.zeros(self.n_edges), np.zeros(self.n_edges)
        rho[self.slots], s[self.slots] = ev["rho"], ev["s"]
        return tree_sum(rho), s

    def assemble(self, C, chi, damping):
        """(A (n, n) with the lower triangle the contract's, g (n,)) at the poses C."""
        n = 6 * (self.n_nodes - 1)
        A, g = np.zeros((n, n)), np.zeros(n)
        BB, BA, AA, GB, GA = edge_stage(self.eval(C, chi))
        with np.errstate(**_ERR):
            for e, (a, b) in enumerate(zip(self.a, self.b)):          # ascending slot order
                rb, ra = 6 * (b - 1), 6 * (a - 1)
                A[rb:rb + 6, rb:rb + 6] += BB[e]
                g[rb:rb + 6] += GB[e]
                if a >= 1:
                    A[rb:rb + 6, ra:ra + 6] += BA[e]
                    A[ra:ra + 6, ra:ra + 6] += AA[e]
                    g[ra:ra + 6] += GA[e]
            A[np.arange(n), np.arange(n)] += np.float64(damping)
        return A, g


# ------------------------------------------------------------------------------------------------------------------- the solve
def solve_banded(A, g, bw):
    """A delta = -g by the header's banded unpivoted LDL^T on the lower triangle of A: (delta, failed_row, D); failed_row is -1, or
    the first pivot that is not finite and > 0 (delta is then None)."""
    n = len(g)
    L = np.array(A, dtype=np.float64)
    D = np.zeros(n)
    with np.errstate(**_ERR):
        for j in range(n):
            d = L[j, j]
            D[j] = d
            if not (d > 0.0 and np.isfinite(d)):
                return None, j, D
            hi = min(n, j + bw + 1)
            col = L[j + 1:hi, j] / d
            L[j + 1:hi, j] = col
            L[j + 1:hi, j + 1:hi] -= (col[:, None] * col[None, :]) * d
        y = -np.asarray(g, np.float64)
        for k in range(n):
            hi = min(n, k + bw + 1)
            y[k + 1:hi] -= L[k + 1:hi, k] * y[k]
        delta = np.zeros(n)
        for i in range(n - 1, -1, -1):
            hi = min(n, i + bw + 1)
            terms = np.concatenate([[y[i] / D[i]], -(L[i + 1:hi, i] * delta[i + 1:hi])])
            delta[i] = np.add.accumulate(terms)[-1]          # sequential: ((v - p0) - p1) - ...
    return delta, -1, D


def apply_update(C, delta):
    out = C.copy()
    for m in range(1, len(C)):
        out[m] = pose_update(C[m], delta[6 * (m - 1):6 * m])
    return out


# ------------------------------------------------------------------------------------------------------------------- a graph
def optimize(first, second, T, info, C_in, band, chi=4.0, damping=0.0, n_iter=8, detail=False):
    """One graph: dict of KEYS; with detail also `steps`: per solve attempted, dict(A, g, delta, failed_row, cost_trial, cost)."""
    C_in = np.asarray(C_in, np.float64).reshape(-1, 12)
    G = Graph(first, second, T, info, len(C_in), band)
    out = dict(C=C_in.copy(), status=3, iterations=0, used_edges=len(G.slots), skipped_edges=G.skipped, failed_row=-1, cost_in=0.0,
               cost=0.0, edge_chi2=np.zeros(G.n_edges))
    steps = []
    if detail:
        out["steps"] = steps
    if len(G.slots) == 0 or not np.isfinite(C_in).all():
        return out
    bw = 6 * band + 5
    cur = C_in.copy()
    cost_in, _ = G.cost(cur, chi)
    cost, accepted, failed, first_failed = cost_in, 0, -1, False
    for it in range(n_iter):
        A, g = G.assemble(cur, chi, damping)
        delta, fail, _ = solve_banded(A, g, bw)
        steps.append(dict(A=A, g=g, delta=delta, failed_row=fail, C=cur.copy()))
        if fail >= 0:
            failed, first_failed = fail, it == 0
            break
        trial = apply_update(cur, delta)
        c_trial, _ = G.cost(trial, chi)
        steps[-1].update(cost_trial=c_trial, cost=cost)
        if not (np.isfinite(c_trial) and c_trial < cost):
            break
        cur, cost, accepted = trial, c_trial, accepted + 1
    _, s = G.cost(cur, chi)
    out.update(C=cur, status=0 if accepted else (2 if first_failed else 1), iterations=accepted, failed_row=failed, cost_in=float(cost_in),
               cost=float(cost), edge_chi2=s)
    return out


def optimize_graphs(first, second, T, info, C_in, band, chi=4.0, damping=0.0, n_iter=8):
    """n_graphs graphs (leading axis of every operand) as the arrays the device writes."""
    res = [optimize(first[k], second[k], T[k], info[k], C_in[k], band, chi, damping, n_iter) for k in range(len(C_in))]
    dt = dict(C=np.float64, cost_in=np.float64, cost=np.float64, edge_chi2=np.float64)
    return {key: np.stack([np.asarray(r[key], dtype=dt.get(key, np.int32)) for r in res]) for key in KEYS}


# ------------------------------------------------------------------------------------------- the independent implementation
def _m44(p):
    return np.vstack([np.asarray(p, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def full_info(info):
    H = np.zeros((6, 6))
    for (i, j), v in zip(TRIU, info):
        H[i, j] = H[j, i] = v
    return H


def plain_normal_equations(first, second, T, info, C, band, chi, damping):
    """(cost, A (n, n) symmetric, g (n,)) of the reduced system, from per-edge matrix products."""
    C = np.asarray(C, np.float64).reshape(-1, 12)
    N = len(C)
    n = 6 * (N - 1)
    A, g, cost = np.zeros((n, n)), np.zeros(n), 0.0
    for e in np.where(used_mask(first, second, np.asarray(T).reshape(-1, 12), np.asarray(info).reshape(-1, 21), N, band))[0]:
        a, b = int(first[e]), int(second[e])
        Tp = _m44(C[b]) @ np.linalg.inv(_m44(C[a]))
        Dm = Tp @ np.linalg.inv(_m44(T[e]))
        R = Dm[:3, :3]
        r = np.concatenate([Dm[:3, 3], 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])])
        H = full_info(info[e])
        s = r @ H @ r
        w = 1.0 if s <= chi * chi else chi / np.sqrt(s)
        cost += s if s <= chi * chi else 2 * chi * np.sqrt(s) - chi * chi
        Rp, tp = Tp[:3, :3], Tp[:3, 3]
        J = np.zeros((6, n + 6))                                     # columns of node m at 6 m
        J[:, 6 * b:6 * b + 6] = np.eye(6)
        J[:, 6 * a:6 * a + 6] = -np.block([[Rp, _skew(tp) @ Rp], [np.zeros((3, 3)), Rp]])
        J = J[:, 6:]                                                 # the anchor's columns dropped
        A += w * (J.T @ H @ J)
        g += w * (J.T @ H @ r)
    return cost, A + damping * np.eye(n), g


def trajectory(C):
    """Camera-to-world (N, 4, 4) from world -> camera poses (N, 12)."""
    return np.stack([np.linalg.inv(_m44(c)) for c in np.asarray(C, np.float64).reshape(-1, 12)])
