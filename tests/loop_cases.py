"""Seeded cases for the restatement (tests/loop_ref.py) and the device (tests/test_gpu_loop.py) of libsslam_loop.so: descriptor
banks for the signatures, signature sets that revisit places for the candidates, and pose graphs with edges past any band for the
sparse solve - tests/pose_graph_cases.py's planted graphs with loop edges measured the same way.  Case generation uses np.linalg
freely: nothing here is what the device computes.
No torch, no GPU: importable anywhere."""
from __future__ import annotations

import numpy as np

import pose_graph_cases as pc
import pose_graph_ref as pg

IU = np.triu_indices(6)


# ------------------------------------------------------------------------------------------------------------- signatures
def bank(n, k, d, seed, zero_frame=None):
    """(desc (n, k, d), scores (n, k)) float32: unit-ish descriptors that share a strong common part, scores in (0, 1)."""
    rng = np.random.default_rng(2000 + seed)
    common = rng.standard_normal(d)
    desc = (common + 0.3 * rng.standard_normal((n, k, d))).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=2, keepdims=True).astype(np.float32)
    scores = rng.random((n, k)).astype(np.float32)
    if zero_frame is not None:
        scores[zero_frame] = 0.0
    return np.ascontiguousarray(desc), scores


def place_signatures(n, d, seed, period, noise=0.25):
    """(n, d) float32 unit rows: frame i shows place i % period, so frames a multiple of `period` apart resemble each other."""
    rng = np.random.default_rng(3000 + seed)
    places = rng.standard_normal((period, d))
    sig = places[np.arange(n) % period] + noise * rng.standard_normal((n, d))
    return np.ascontiguousarray((sig / np.linalg.norm(sig, axis=1, keepdims=True)).astype(np.float32))


def candidate_case(name, sig, min_gap, min_sim, per_frame, suppress):
    return dict(name=name, sig=sig, min_gap=min_gap, min_sim=min_sim, per_frame=per_frame, suppress=suppress)


def candidate_cases():
    """The rows of the contract: ties, the gap, suppression at frame 0, per_frame 1 and 8, fewer eligible frames than slots."""
    dup = place_signatures(14, 128, 1, 14)
    dup[1:5] = dup[0]                                              # five identical frames: equal sims, the lower j first
    dup[12] = dup[0]
    near0 = place_signatures(40, 128, 2, 40)
    near0[30] = near0[1]                                           # the best match of frame 30 is frame 1: suppression reaches below 0
    near0[31] = near0[1]
    few = place_signatures(20, 256, 3, 7)
    return [
        candidate_case("duplicate_frames", dup, 3, 0.5, 4, 0),
        candidate_case("duplicate_frames_suppressed", dup, 3, 0.5, 4, 1),
        candidate_case("gap_at_least_n", place_signatures(9, 128, 4, 3), 9, -1.0, 2, 0),
        candidate_case("gap_past_n", place_signatures(9, 128, 4, 3), 1000, -1.0, 2, 0),
        candidate_case("suppression_clipped_at_frame_0", near0, 5, -1.0, 3, 5),
        candidate_case("per_frame_1", place_signatures(50, 128, 5, 11), 8, 0.3, 1, 2),
        candidate_case("per_frame_8", place_signatures(50, 128, 5, 11), 8, 0.0, 8, 1),
        candidate_case("fewer_eligible_than_slots", few, 6, 0.6, 8, 0),
        candidate_case("everything_suppressed_after_one", few, 2, -1.0, 8, 1000000),
        candidate_case("width_256", place_signatures(33, 256, 6, 10), 5, 0.2, 2, 3),
    ]


def candidate_size_cases():
    """N in {1, 2, 64, 65, 300}: below, at and past one stride of the 256 threads, and more than one stride."""
    return [candidate_case(f"n_{n}", place_signatures(n, 128, 10 + n, max(1, min(n, 23))), 1 if n <= 2 else 20, -1.0 if n <= 2 else 0.3, 2, 5) for n in (1, 2, 64, 65, 300)]


# ------------------------------------------------------------------------------------------------------------------ graphs
def measure(truth, edges, rng, sigma_t=0.01, sigma_r=0.004, gap_scaled=True):
    """(T (E, 12), info (E, 21)) of the edges measured on `truth` as pose_graph_cases.planted measures: noise drawn from each edge's
    own covariance.  gap_scaled False: the noise of a spacing-1 edge whatever b - a is - two views of ONE place."""
    T, info = np.empty((len(edges), 12)), np.empty((len(edges), 21))
    for e, (a, b) in enumerate(edges):
        sig = np.concatenate([np.full(3, sigma_t), np.full(3, sigma_r)]) * rng.uniform(0.7, 1.5, 6) * np.sqrt(1.0 + 0.2 * ((b - a) if gap_scaled else 1))
        M = np.eye(6) + 0.15 * rng.standard_normal((6, 6))
        cov = M @ np.diag(sig * sig) @ M.T
        T[e] = pc.perturb(pg.compose(truth[b], pg.inverse(truth[a])), np.linalg.cholesky(cov) @ rng.standard_normal(6))
        H = np.linalg.inv(cov)
        info[e] = (0.5 * (H + H.T))[IU]
    return T, info


def with_loops(n_nodes, spacings, seed, loops, name=None, chi=4.0, damping=0.0, n_iter=8, cg_iterations=512, cg_tol=1e-3, **kw):
    """A planted graph (pose_graph_cases.planted) followed by the loop edges `loops` [(a, b), ...], measured at a spacing-1 edge's
    noise; the start is the spacing-1 chain."""
    p = pc.planted(n_nodes, spacings, seed, **kw)
    rng = np.random.default_rng(5000 + seed)
    sig = {k: kw[k] for k in ("sigma_t", "sigma_r") if k in kw}
    Tl, il = measure(p["truth"], loops, rng, gap_scaled=False, **sig) if loops else (np.empty((0, 12)), np.empty((0, 21)))
    first = np.concatenate([p["first"], np.array([a for a, _ in loops], np.int32)]).astype(np.int32)
    second = np.concatenate([p["second"], np.array([b for _, b in loops], np.int32)]).astype(np.int32)
    return dict(name=name or f"loops_{n_nodes}_{seed}", first=first, second=second, T=np.concatenate([p["T"], Tl]), info=np.concatenate([p["info"], il]),
                C_in=p["C_chain"], truth=p["truth"], n_odometry=len(p["first"]), chi=chi, damping=damping, n_iter=n_iter,
                cg_iterations=cg_iterations, cg_tol=cg_tol)


def from_banded(c, **kw):
    """A case of pose_graph_cases as a sparse case."""
    out = dict(name=c["name"], first=c["first"], second=c["second"], T=c["T"], info=c["info"], C_in=c["C_in"], chi=c["chi"], damping=c["damping"],
               n_iter=c["n_iter"], cg_iterations=512, cg_tol=1e-3)
    out.update(kw)
    return out


def exact_with_far_edge():
    ex = pc.exact_graph()
    C = ex["C_in"]
    return dict(name="exact_graph_plus_0_4", first=np.append(ex["first"], 0).astype(np.int32), second=np.append(ex["second"], 4).astype(np.int32),
                T=np.concatenate([ex["T"], pg.compose(C[4], pg.inverse(C[0]))[None]]), info=np.concatenate([ex["info"], np.eye(6)[IU][None]]),
                C_in=C, chi=4.0, damping=0.0, n_iter=8, cg_iterations=512, cg_tol=1e-3)


def forty_nodes_many_slots():
    """40 nodes, 149 planted edges and 12 loop edges, then every slot again measuring something else (duplicates), and among the
    322 slots an absent one, a non-finite T, a non-finite info, a == b, a > b and a node out of range."""
    c = with_loops(40, pc.SPACINGS, 6, [(a, a + 30) for a in range(0, 10)] + [(0, 39), (3, 37)], name="forty_nodes_322_slots", outliers=0.03)
    other = with_loops(40, pc.SPACINGS, 6, [(a, a + 30) for a in range(0, 10)] + [(0, 39), (3, 37)])
    rng = np.random.default_rng(77)
    edges = list(zip(c["first"], c["second"]))
    T2, i2 = measure(other["truth"], edges, rng)
    for key, extra in (("first", c["first"]), ("second", c["second"]), ("T", T2), ("info", i2)):
        c[key] = np.concatenate([c[key], extra])
    c["first"][7] = -1
    c["T"][20, 3] = np.nan
    c["info"][200, 5] = np.inf
    c["second"][41] = c["first"][41]
    c["first"][170], c["second"][170] = 9, 4
    c["second"][300] = 40
    assert len(c["first"]) > 256
    return c


def hub_case():
    """76 nodes in a chain and node 5 joined to every node 6 .. 75: 70 edges at the hub besides its two chain edges."""
    return with_loops(76, (1,), 21, [(5, b) for b in range(6, 76)], name="hub_of_70", n_iter=3)


def unreachable_case():
    """Six nodes, none of the edges names node 3: its block is zero, the first pivot fails at row 6 * (3 - 1)."""
    c = with_loops(6, (1, 2), 22, [], name="unreachable_node")
    gone = (c["first"] == 3) | (c["second"] == 3)
    c["first"] = np.where(gone, -1, c["first"]).astype(np.int32)
    return c


def sparse_cases():
    small = with_loops(12, (1, 2), 23, [(0, 11), (2, 9)], name="twelve_nodes_two_loops")
    return [
        from_banded(pc.shape_cases()[0]),                                                   # two nodes, one edge
        exact_with_far_edge(),
        forty_nodes_many_slots(),
        hub_case(),
        unreachable_case(),
        with_loops(44, (1, 2), 24, [(0, 43), (5, 40)], name="rows_258_past_one_stride", n_iter=2),       # 6 * 43 = 258 rows
        with_loops(258, (1, 3), 25, [(0, 257), (10, 250)], name="nodes_257_past_one_stride", n_iter=2, cg_iterations=60),
        dict(small, name="no_iterations", n_iter=0),
        dict(small, name="one_cg_iteration", cg_iterations=1),
        dict(small, name="cg_tol_zero", cg_tol=0.0, cg_iterations=40, n_iter=3),
        dict(small, name="huber_and_damping", chi=1.0, damping=0.5),
    ]


def stacked(cases):
    """Cases of equal n_nodes padded with absent slots to one edge count: the operands of one n_graphs call."""
    return pc.stacked_graphs(cases)


def run(c, detail=False):
    import loop_ref as ref
    return ref.optimize(c["first"], c["second"], c["T"], c["info"], c["C_in"], c["chi"], c["damping"], c["n_iter"], c["cg_iterations"], c["cg_tol"],
                        detail=detail)


def study_case(seed):
    """The planted loop study: 420 nodes (the path turns a full circle in about 370 frames), the five spacings, 3 % gross outliers,
    noise x 3, and 30 loop edges (a, a + 370), a = 0 .. 29."""
    return with_loops(420, pc.SPACINGS, seed, [(a, a + 370) for a in range(30)], outliers=0.03, sigma_t=0.03, sigma_r=0.012)
