"""A numpy restatement of libsslam_loop.so (csrc_loop/loop.hip), written from the contract in include/sslam_loop.h: the frame
signatures and the candidate lists in float32 - a fused multiply-add where the header writes fmaf, made here from float64
arithmetic (fmaf32) - and the sparse pose graph in float64.  The per-edge terms, the cost, the update and the used edges are
tests/pose_graph_ref.py's, imported, not copied: only the solve differs from libsslam_graph.so.

The device adds a node's terms by walking its incidence list; here the lists are laid out in ROUNDS - round r holds the r-th entry
of every node that has one - so that a round is one vectorised numpy operation per term and every node still takes its terms in
ascending slot order.  Nothing the device computes goes through np.dot, @, np.sum or np.linalg.

Tolerance: NONE - both sides take the same correctly rounded operations in one order.
"""
from __future__ import annotations

import numpy as np

import pose_graph_ref as pg
from pose_ransac_ref import tree_sum

MAX_FRAMES, MAX_K, MAX_PER_FRAME = 4096, 4096, 8
MAX_NODES, MAX_EDGES, MAX_GRAPHS, MAX_ITER, MAX_CG = 4096, 65536, 65535, 16, 4096
FRAMES_PER_GROUP = 32
KEYS = pg.KEYS + ("cg_steps",)
CANDIDATE_KEYS = ("first", "second", "sim", "count")
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


# ------------------------------------------------------------------------------------------------------------------- float32
def fmaf32(a, b, c):
    """fmaf(a, b, c) for float32 arrays: the exact a * b + c rounded ONCE to float32.  a * b is exact in float64; the sum is rounded
    to odd in float64 (the round-to-nearest sum, moved to its odd neighbour on the side of the rounding error when it is inexact
    and even), and a value rounded to odd at 53 bits rounds to 24 bits as the exact one does."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
    with np.errstate(**_ERR):
        t = p + c
        bp = t - p
        err = (p - (t - bp)) + (c - bp)
        even = (t.view(np.int64) & 1) == 0
        odd = np.nextafter(t, np.where(err > 0, np.inf, -np.inf))
        t = np.where((err != 0) & even & np.isfinite(t), odd, t)
        return t.astype(np.float32)


def wave_sum32(x):
    """(..., d) float32 -> (...): lanes of each wave of 64 by xor 32 .. 1, then the waves ascending."""
    x = np.asarray(x, np.float32)
    part = x.reshape(x.shape[:-1] + (x.shape[-1] // 64, 64))
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[..., lanes ^ o]
    w = part[..., 0]
    out = w[..., 0]
    for k in range(1, w.shape[-1]):
        out = out + w[..., k]
    return out


def raw_signatures(desc, scores):
    desc, scores = np.asarray(desc, np.float32), np.asarray(scores, np.float32)
    acc = np.zeros((desc.shape[0], desc.shape[2]), np.float32)
    for k in range(desc.shape[1]):
        acc = fmaf32(scores[:, k, None], desc[:, k], acc)
    return acc


def signatures(desc, scores):
    """sig (N, D) float32 of desc (N, K, D), scores (N, K)."""
    return finish_signatures(raw_signatures(desc, scores))


def finish_signatures(raw):
    """sig (N, D) float32 of the raw sums (N, D) of ALL the sequence's frames: the mean in frame order, the centring, the norm."""
    raw = np.asarray(raw, np.float32)
    n = len(raw)
    with np.errstate(**_ERR):
        mean = np.zeros(raw.shape[1], np.float32)
        for i in range(n):
            mean = mean + raw[i]
        mean = mean / np.float32(n)
        c = raw - mean
        ss = wave_sum32(c * c)
        return (c / np.fmax(np.sqrt(ss), np.float32(1e-12))[:, None]).astype(np.float32)


def similarity(sig):
    """S (N, N) float32: S_ij one fmaf chain over the columns ascending."""
    sig = np.asarray(sig, np.float32)
    S = np.zeros((len(sig), len(sig)), np.float32)
    for c in range(sig.shape[1]):
        S = fmaf32(sig[:, None, c], sig[None, :, c], S)
    return S


def candidates(sig, min_gap=30, min_sim=0.3, per_frame=2, suppress=5, S=None):
    """dict of CANDIDATE_KEYS as the device writes them."""
    S = similarity(sig) if S is None else S
    n, lo = len(S), np.float32(min_sim)
    first, second = np.full(n * per_frame, -1, np.int32), np.full(n * per_frame, -1, np.int32)
    sim, count = np.zeros(n * per_frame, np.float32), np.zeros(n, np.int32)
    for i in range(n):
        m = i - min_gap + 1
        if m <= 0:
            continue
        row = S[i, :m]
        live = row >= lo
        for s in range(per_frame):
            if not live.any():
                break
            best = np.where(live, row, -np.inf).max()
            j = int(np.flatnonzero(live & (row == best))[0])
            first[i * per_frame + s], second[i * per_frame + s], sim[i * per_frame + s] = j, i, row[j]
            count[i] += 1
            live[max(0, j - suppress):j + suppress + 1] = False
    return dict(first=first, second=second, sim=sim, count=count)


# ------------------------------------------------------------------------------------------------------------------- the graph
def _sum6(x):
    return ((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]


class SparseGraph(pg.Graph):
    """pose_graph_ref.Graph without a band, and the incidence lists in rounds."""

    def __init__(self, first, second, T, info, n_nodes):
        super().__init__(first, second, T, info, n_nodes, max(int(n_nodes), 1))
        k = np.arange(len(self.slots))
        node = np.stack([self.b, self.a], axis=1).reshape(-1)          # per used edge, in slot order: as its b, then as its a
        edge, side = np.repeat(k, 2), np.tile([0, 1], len(k))
        keep = node >= 1
        node, edge, side = node[keep], edge[keep], side[keep]
        order = np.argsort(node, kind="stable")                       # within a node the slot order stays
        node, edge, side = node[order], edge[order], side[order]
        start = np.searchsorted(node, node, side="left")
        pos = np.arange(len(node)) - start
        self.rounds = []
        for r in range(int(pos.max()) + 1 if len(pos) else 0):
            sel = pos == r
            self.rounds.append((node[sel] - 1, edge[sel], side[sel].astype(bool)))
        self.degree = np.bincount(node, minlength=self.n_nodes)

    def blocks(self, C, chi, damping):
        """(D (nn, 6, 6) with the lower triangle the contract's, g (nn, 6), BA (E_used, 6, 6)) at the poses C."""
        nn = self.n_nodes - 1
        BB, BA, AA, GB, GA = pg.edge_stage(self.eval(C, chi))
        D, g = np.zeros((nn, 6, 6)), np.zeros((nn, 6))
        with np.errstate(**_ERR):
            for mi, e, as_a in self.rounds:
                D[mi] = D[mi] + np.where(as_a[:, None, None], AA[e], BB[e])
                g[mi] = g[mi] + np.where(as_a[:, None], GA[e], GB[e])
            idx = np.arange(6)
            D[:, idx, idx] = D[:, idx, idx] + np.float64(damping)
        return D, g, BA


def block_ldl(D):
    """Every block's unpivoted LDL^T in sslam_hip.h's order: (f (nn, 6, 6): L below the diagonal, the pivots on it; failed_row or -1)."""
    f = np.array(D, dtype=np.float64)
    nn = len(f)
    bad = np.full(nn, -1)
    with np.errstate(**_ERR):
        for j in range(6):
            d = f[:, j, j].copy()
            for k in range(j):
                d = d - (f[:, j, k] * f[:, j, k]) * f[:, k, k]
            f[:, j, j] = d
            bad = np.where((bad < 0) & ~((d > 0.0) & np.isfinite(d)), j, bad)
            for i in range(j + 1, 6):
                l = f[:, i, j].copy()
                for k in range(j):
                    l = l - (f[:, i, k] * f[:, j, k]) * f[:, k, k]
                f[:, i, j] = l / d
    rows = np.where(bad >= 0, 6 * np.arange(nn) + bad, np.iinfo(np.int64).max)
    return f, (int(rows.min()) if (bad >= 0).any() else -1)


def block_solve(f, v):
    """z = M^-1 v per node."""
    y, z = np.array(v, dtype=np.float64), np.empty(v.shape)
    with np.errstate(**_ERR):
        for i in range(6):
            for k in range(i):
                y[:, i] = y[:, i] - f[:, i, k] * y[:, k]
        for i in range(5, -1, -1):
            z[:, i] = y[:, i] / f[:, i, i]
            for k in range(i + 1, 6):
                z[:, i] = z[:, i] - f[:, k, i] * z[:, k]
    return z


def dot(u, v):
    with np.errstate(**_ERR):
        return tree_sum(u.reshape(-1) * v.reshape(-1))


def matvec(G, D, BA, p):
    """q = A p: the diagonal blocks, then every node's off-diagonal blocks in its list's order."""
    sym = np.where(np.tri(6, dtype=bool), D, np.swapaxes(D, 1, 2))   # D_ik read from the lower triangle, either way round
    with np.errstate(**_ERR):
        q = np.stack([_sum6([sym[:, i, k] * p[:, k] for k in range(6)]) for i in range(6)], axis=1)
        for mi, e, as_a in G.rounds:
            has = G.a[e] >= 1
            mi, e, as_a = mi[has], e[has], as_a[has]
            po = p[np.where(as_a, G.b[e], G.a[e]) - 1]
            B = np.where(as_a[:, None, None], np.swapaxes(BA[e], 1, 2), BA[e])
            q[mi] = q[mi] + np.stack([_sum6([B[:, i, k] * po[:, k] for k in range(6)]) for i in range(6)], axis=1)
    return q


def pcg(G, D, g, BA, f, cg_iterations, cg_tol):
    """(x (nn, 6), steps) of A x = -g from x = 0."""
    return pcg_trace(G, D, g, BA, f, cg_iterations, cg_tol)[:2]


def pcg_trace(G, D, g, BA, f, cg_iterations, cg_tol):
    """pcg, and how its loop ended: "count" (cg_iterations taken), "pq" (p . A p not positive and finite) or "tol"."""
    tol2 = np.float64(cg_tol) * np.float64(cg_tol)
    ended = "count"
    with np.errstate(**_ERR):
        x, r = np.zeros(g.shape), -g
        z = block_solve(f, r)
        p = z.copy()
        rz = dot(r, z)
        rz0, steps = rz, 0
        for _ in range(cg_iterations):
            q = matvec(G, D, BA, p)
            pq = dot(p, q)
            if not (pq > 0.0 and np.isfinite(pq)):
                ended = "pq"
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            z = block_solve(f, r)
            rz1 = dot(r, z)
            steps += 1
            if rz1 <= tol2 * rz0:
                ended = "tol"
                break
            beta = rz1 / rz
            p = z + beta * p
            rz = rz1
    return x, steps, ended


def optimize(first, second, T, info, C_in, chi=4.0, damping=0.0, n_iter=8, cg_iterations=512, cg_tol=1e-3, detail=False):
    """One graph: dict of KEYS; with detail also `steps`: per solve attempted, dict(C, D, g, BA, delta, failed_row, cg)."""
    C_in = np.asarray(C_in, np.float64).reshape(-1, 12)
    G = SparseGraph(first, second, T, info, len(C_in))
    out = dict(C=C_in.copy(), status=3, iterations=0, used_edges=len(G.slots), skipped_edges=G.skipped, failed_row=-1, cost_in=0.0,
               cost=0.0, edge_chi2=np.zeros(G.n_edges), cg_steps=np.zeros(MAX_ITER, np.int32))
    steps = []
    if detail:
        out["steps"] = steps
    if len(G.slots) == 0 or not np.isfinite(C_in).all():
        return out
    cur = C_in.copy()
    cost_in, _ = G.cost(cur, chi)
    cost, accepted, failed, first_failed = cost_in, 0, -1, False
    for it in range(n_iter):
        D, g, BA = G.blocks(cur, chi, damping)
        f, fail = block_ldl(D)
        steps.append(dict(C=cur.copy(), D=D, g=g, BA=BA, delta=None, failed_row=fail, cg=0))
        if fail >= 0:
            failed, first_failed = fail, it == 0
            break
        x, n_cg = pcg(G, D, g, BA, f, cg_iterations, cg_tol)
        out["cg_steps"][it] = n_cg
        steps[-1].update(delta=x.reshape(-1), cg=n_cg)
        trial = pg.apply_update(cur, x.reshape(-1))
        c_trial, _ = G.cost(trial, chi)
        if not (np.isfinite(c_trial) and c_trial < cost):
            break
        cur, cost, accepted = trial, c_trial, accepted + 1
    _, s = G.cost(cur, chi)
    out.update(C=cur, status=0 if accepted else (2 if first_failed else 1), iterations=accepted, failed_row=failed, cost_in=float(cost_in),
               cost=float(cost), edge_chi2=s)
    return out


def optimize_graphs(first, second, T, info, C_in, chi=4.0, damping=0.0, n_iter=8, cg_iterations=512, cg_tol=1e-3):
    """n_graphs graphs (leading axis of every operand) as the arrays the device writes."""
    res = [optimize(first[k], second[k], T[k], info[k], C_in[k], chi, damping, n_iter, cg_iterations, cg_tol) for k in range(len(C_in))]
    dt = dict(C=np.float64, cost_in=np.float64, cost=np.float64, edge_chi2=np.float64)
    return {key: np.stack([np.asarray(r[key], dtype=dt.get(key, np.int32)) for r in res]) for key in KEYS}
