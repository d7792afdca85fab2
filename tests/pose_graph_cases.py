"""Planted pose graphs for the restatement (tests/pose_graph_ref.py) and the device (tests/test_gpu_pose_graph.py): a smooth
camera path, edges (i, i + s) at the given spacings measured with noise drawn from each edge's own covariance (the information
matrix handed over is that covariance's inverse), a share of gross outliers, and the chained spacing-1 poses as the initial guess.
Everything is seeded.  Case generation uses sines and np.linalg freely: nothing here is what the device computes.
No torch, no GPU: importable anywhere."""
from __future__ import annotations

import numpy as np

import pose_graph_ref as ref

SPACINGS = (1, 5, 10, 15, 20)


def so3(w):
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    K = ref._skew(w)
    if t < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * (K @ K)


def pose12(R, t):
    return np.hstack([R, np.asarray(t, np.float64).reshape(3, 1)]).reshape(12)


def perturb(T12, xi):
    """exp(xi) o T, xi = (v, w): the left perturbation the information matrices are stated in (first order in v)."""
    return ref.compose(pose12(so3(xi[3:]), xi[:3]), T12)


def path(n_nodes, seed):
    """World -> camera poses (n_nodes, 12) of a curved walk: about 5 cm and 1 degree per frame."""
    rng = np.random.default_rng(seed)
    C = [pose12(np.eye(3), np.zeros(3))]
    for i in range(n_nodes - 1):
        step = pose12(so3([0.004 * np.sin(0.11 * i), 0.017 + 0.004 * rng.standard_normal(), 0.003 * np.cos(0.07 * i)]),
                      [0.05 + 0.01 * rng.standard_normal(), 0.01 * np.sin(0.2 * i), 0.02 * rng.standard_normal()])
        C.append(ref.compose(step, C[-1]))
    return np.stack(C)


def edge_list(n_nodes, spacings):
    return [(i, i + s) for s in spacings for i in range(n_nodes - s)]


def planted(n_nodes, spacings=SPACINGS, seed=0, outliers=0.0, sigma_t=0.01, sigma_r=0.004):
    """dict(first, second int32 (E,), T (E, 12), info (E, 21), truth (n_nodes, 12), C_chain (n_nodes, 12), outlier (E,) bool)."""
    rng = np.random.default_rng(1000 + seed)
    truth = path(n_nodes, seed)
    edges = edge_list(n_nodes, spacings)
    E = len(edges)
    first, second = np.array([a for a, _ in edges], np.int32), np.array([b for _, b in edges], np.int32)
    T, info, outlier = np.empty((E, 12)), np.empty((E, 21)), rng.random(E) < outliers
    iu = np.triu_indices(6)
    for e, (a, b) in enumerate(edges):
        sig = np.concatenate([np.full(3, sigma_t), np.full(3, sigma_r)]) * rng.uniform(0.7, 1.5, 6) * np.sqrt(1.0 + 0.2 * (b - a))
        M = np.eye(6) + 0.15 * rng.standard_normal((6, 6))
        cov = M @ np.diag(sig * sig) @ M.T
        xi = np.linalg.cholesky(cov) @ rng.standard_normal(6)
        if outlier[e]:
            xi = xi + np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.2, 0.2, 3)])
        T[e] = perturb(ref.compose(truth[b], ref.inverse(truth[a])), xi)
        H = np.linalg.inv(cov)
        info[e] = (0.5 * (H + H.T))[iu]
    n1 = n_nodes - 1 if 1 in spacings else 0
    chain = ref.chain(T[:n1]) if n1 == n_nodes - 1 else truth.copy()
    return dict(first=first, second=second, T=T, info=info, truth=truth, C_chain=chain, outlier=outlier)


def exact_graph():
    """Poses of quarter turns and dyadic translations, the edges their exact relative poses with unit information: every residual is
    +-0.0 exactly.  band 2, 5 nodes."""
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    Rs = [np.eye(3), Rz, Rz @ Rx, Rx, Rx @ Rz]
    C = np.stack([pose12(R, [0.5 * i, -0.25 * i, 2.0 - 0.125 * i]) for i, R in enumerate(Rs)])
    edges = edge_list(5, (1, 2))
    first, second = np.array([a for a, _ in edges], np.int32), np.array([b for _, b in edges], np.int32)
    T = np.stack([ref.compose(C[b], ref.inverse(C[a])) for a, b in edges])
    info = np.tile(np.eye(6)[np.triu_indices(6)], (len(edges), 1))
    return dict(first=first, second=second, T=T, info=info, C_in=C, band=2)


def graph_case(name, n_nodes, spacings, band, seed, chi=4.0, damping=0.0, n_iter=8, **kw):
    p = planted(n_nodes, spacings, seed, **kw)
    return dict(name=name, first=p["first"], second=p["second"], T=p["T"], info=p["info"], C_in=p["C_chain"], band=band, chi=chi,
                damping=damping, n_iter=n_iter, truth=p["truth"])


def shape_cases():
    """The smallest shapes at which the band indexing can go wrong."""
    return [
        graph_case("two_nodes_one_edge", 2, (1,), 1, 1),
        graph_case("three_nodes_band_2", 3, (1, 2), 2, 2),
        graph_case("band_plus_1", 4, (1, 2, 3), 3, 3),
        graph_case("band_plus_2_window_slides", 5, (1, 2, 3), 3, 4),
        graph_case("band_plus_5", 8, (1, 3), 3, 5),
        graph_case("forty_nodes_five_spacings", 40, SPACINGS, 20, 6, outliers=0.03),
        graph_case("thirty_four_nodes_band_32", 34, (1, 16, 32), 32, 7),
        graph_case("forty_nodes_band_32_window_slides", 40, (1, 16, 32), 32, 10),      # 234 rows: the 198-row window slides 36 times
        graph_case("huber_branch", 12, (1, 2, 4), 4, 8, chi=1.0, outliers=0.15),
        graph_case("damped", 9, (1, 3), 3, 9, damping=0.5),
    ]


def _with_edges(case, name, **changes):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    out["name"] = name
    for key, (slot, value) in changes.items():
        out[key][slot] = value
    return out


def contract_cases():
    """The contract's rows: exact edges, no iterations, absent and skipped slots, a disconnected node, duplicates."""
    base = graph_case("base", 7, (1, 2, 3), 3, 11)
    ex = exact_graph()
    cases = [dict(name="exact_edges", chi=4.0, damping=0.0, n_iter=8, **ex),
             dict(base, name="no_iterations", n_iter=0),
             _with_edges(base, "absent_slot", first=(4, -1)),
             _with_edges(base, "second_before_first", first=(7, 5), second=(7, 2)),
             _with_edges(base, "equal_nodes", second=(8, base["first"][8])),
             _with_edges(base, "node_out_of_range", second=(9, 7)),
             _with_edges(base, "negative_node", first=(9, -3)),
             _with_edges(base, "nan_in_T", T=((3, 5), np.nan)),
             _with_edges(base, "inf_in_info", info=((10, 20), np.inf)),
             _with_edges(base, "nan_in_info", info=((2, 0), np.nan))]
    wide = graph_case("past_the_band", 7, (1, 2, 3), 2, 11)           # the spacing-3 edges lie past band 2
    cases.append(wide)
    # node 4 disconnected: every edge that names it absent
    lone = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    touch = (lone["first"] == 4) | (lone["second"] == 4)
    lone["first"][touch] = -1
    cases.append(dict(lone, name="disconnected_node"))
    cases.append(dict(lone, name="disconnected_node_damped", damping=1.0))
    dup = {k: (np.concatenate([v, v[:5]]) if isinstance(v, np.ndarray) and k in ("first", "second", "T", "info") else v) for k, v in base.items()}
    dup["T"][-5:] = planted(7, (1, 2, 3), 12)["T"][:5]                # the duplicates measure something else
    cases.append(dict(dup, name="duplicate_edges"))
    bad = dict(base, name="nan_in_C_in", C_in=base["C_in"].copy())
    bad["C_in"][3, 7] = np.nan
    cases.append(bad)
    cases.append(dict(base, name="no_used_edge", first=np.full_like(base["first"], -1)))
    return cases


def run(case, detail=False):
    return ref.optimize(case["first"], case["second"], case["T"], case["info"], case["C_in"], case["band"], case["chi"], case["damping"],
                        case["n_iter"], detail=detail)


def ate_rmse(C, truth):
    """Position rmse after rigid alignment without scale of the camera centres of world -> camera poses."""
    est, gt = ref.trajectory(C)[:, :3, 3], ref.trajectory(truth)[:, :3, 3]
    cs, cd = est.mean(axis=0), gt.mean(axis=0)
    U, _, Vt = np.linalg.svd((gt - cd).T @ (est - cs))
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ S @ Vt
    return float(np.sqrt(np.mean(np.sum((est @ R.T + (cd - R @ cs) - gt) ** 2, axis=1))))


def stacked_graphs(cases):
    """Cases of equal n_nodes padded with absent slots to one edge count: the operands of one n_graphs call."""
    E = max(len(c["first"]) for c in cases)

    def pad(v, fill):
        out = np.full((E,) + v.shape[1:], fill, dtype=v.dtype)
        out[:len(v)] = v
        return out
    return dict(first=np.stack([pad(c["first"], -1) for c in cases]), second=np.stack([pad(c["second"], -1) for c in cases]),
                T=np.stack([pad(c["T"], 0.0) for c in cases]), info=np.stack([pad(c["info"], 0.0) for c in cases]),
                C_in=np.stack([c["C_in"] for c in cases]))
