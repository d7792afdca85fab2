"""The host halves of odometry, odometry_result, odometry_graph, odometry_result_graph and odometry_result_loop_graph without a GPU:
a stub pipeline hands out CPU tensors of the real shapes and dtypes whose every value occurs nowhere else, so a value that lands under
the wrong key, in the wrong row or in the wrong dtype shows.  Each call's dictionary is compared with one put together here from the
stub's tensors BY NAME - key order, Python types, dtypes, shapes and values - and each call makes exactly one device-to-host read."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sslam_amd import lib
from sslam_amd import odometry as od
from sslam_amd.evaluation import Camera
from sslam_amd.pipeline import PoseWeights
from sslam_amd.track_numpy import length_statistics

N, K, D, SPACINGS, PER_FRAME = 5, 7, 4, (1, 2), 2
LISTS = {s: od.consecutive_pairs(N, s) for s in SPACINGS}
PAIRS = [pr for s in SPACINGS for pr in LISTS[s]]
P, L = len(PAIRS), N * PER_FRAME
CAMERA = Camera(width=8, height=6)
# the candidate slots, two per frame: frame 3 names frame 0, frame 4 names frames 0 and 1; the others are empty
CAND_FIRST = [-1, -1, -1, -1, -1, -1, 0, -1, 0, 1]
CAND_SECOND = [-1, -1, -1, -1, -1, -1, 3, -1, 4, 4]
REFINED_INLIERS = 12000                         # the stub's refined inlier_count of row r is REFINED_INLIERS + r
MIN_INLIERS = REFINED_INLIERS + P + 7           # so slot 6 is filled and refused, slots 8 and 9 are filled and kept


def ints(base, *shape):
    return (base + torch.arange(int(np.prod(shape)))).reshape(shape).to(torch.int32)


def reals(base, *shape):
    return (base + torch.arange(int(np.prod(shape)), dtype=torch.float64) / 1024).reshape(shape)


def rigid(base, rows):
    """(rows, 12) float64 [R | t]: a small rotation about z and a small translation, no two rows alike."""
    out = np.zeros((rows, 3, 4))
    for r in range(rows):
        a = base + 0.001 * (r + 1)
        out[r, :3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
        out[r, :, 3] = [base + 0.01 * (r + 1), 0.02 * (r + 1), base + 0.03 * (r + 1)]
    return torch.from_numpy(out.reshape(rows, 12))


POSES = np.stack([np.linalg.inv(np.vstack([rigid(0.3, N)[i].numpy().reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])) for i in range(N)])


class StubPipeline:
    """The pipeline methods the odometry layer calls, each answering seeded tensors and keeping what it answered."""
    cfg = SimpleNamespace(confidence=True, num_keypoints=K)

    def __init__(self):
        self.graphs = []

    def tokens_from_images(self, images):
        raise AssertionError("tokens are given")

    def extract(self, tokens, images):
        n = int(tokens.shape[0])
        self.ex = {"descriptors": reals(70.0, n, K, D).float(), "scores": reals(71.0, n, K).float(),
                   "keypoints_pixel": reals(72.0, n, K, 2).float(), "confidence": reals(73.0, n, K).float()}
        return self.ex

    def keypoint_depth(self, depth, keypoints, out):
        out.copy_(ints(26000, *out.shape))

    def match_pairs(self, desc, scores, first, second, rule):
        rows = len(first)
        self.far = {"matches": ints(27000, rows, K, 2).long(), "match_count": ints(6900, rows)}
        return self.far

    def match_weights(self, confidence, first, second, matches, weights):
        return reals(74.0, len(first), K).float()

    def estimate_poses(self, kp, kp_depth, first, second, matches, camera, threshold, hypotheses, seed):
        rows = len(first)
        self.est = {"T": rigid(0.0, rows), "inlier_count": ints(1000, rows), "usable_count": ints(2000, rows),
                    "best_hypothesis": ints(3000, rows), "refit_kept": ints(4000, rows), "inlier_of_slot": ints(5000, rows, K),
                    "rms": reals(10.0, rows)}
        return self.est

    def refine_poses(self, kp, kp_depth, first, second, matches, camera, pose, threshold, huber, iterations, weights=None):
        rows = len(first)
        self.ref = {"T": rigid(0.1, rows), "status": ints(7000, rows), "iterations": ints(8000, rows), "selected_count": ints(9000, rows),
                    "usable_count": ints(10000, rows), "inlier_count_in": ints(11000, rows), "inlier_count": ints(REFINED_INLIERS, rows),
                    "inlier_of_slot": ints(13000, rows, K), "cost_in": reals(20.0, rows), "cost": reals(21.0, rows), "rms": reals(22.0, rows),
                    "info": reals(23.0, rows, 21)}
        if weights is not None:
            self.ref["weight_sum"] = reals(24.0, rows)
        return self.ref

    def _graph(self, n, edges, sparse):
        c = len(self.graphs)
        g = {"C": rigid(0.2 + 0.1 * c, n)}
        g.update({key: ints(14000 + 1000 * i + 100 * c).reshape(()) for i, key in enumerate(lib.POSE_GRAPH_KEYS[1:6])})
        g.update(cost_in=reals(30.0 + 10 * c).reshape(()), cost=reals(31.0 + 10 * c).reshape(()), edge_chi2=reals(32.0 + 10 * c, edges))
        if sparse:
            g["cg_steps"] = ints(19000 + 100 * c, lib.SPARSE_MAX_ITER)
        self.graphs.append(g)
        return g

    def optimize_pose_graph(self, first, second, T, info, n, C_init=None, band=None, huber_chi=4.0, damping=0.0, iterations=8):
        return self._graph(n, len(first), False)

    def optimize_pose_graph_sparse(self, first, second, T, info, n, C_init, huber_chi, damping, iterations, cg_iterations, cg_tol):
        return self._graph(n, len(first), True)

    def find_loop_candidates(self, desc, scores, min_gap, min_sim, per_frame, suppress):
        assert per_frame == PER_FRAME
        self.cand = {"first": torch.tensor(CAND_FIRST, dtype=torch.int32), "second": torch.tensor(CAND_SECOND, dtype=torch.int32),
                     "sim": reals(40.0, L).float(), "count": ints(21000, N), "signatures": reals(41.0, N, D).float()}
        return self.cand

    def link_matches(self, first, second, matches, mask=None, n_frames=None, k=None):
        self.linked = {"matches": matches, "mask": mask}
        return {key: None for key in lib.LINK_KEYS}

    def track_ids(self, links):
        self.tr = {"n_tracks": torch.tensor([9], dtype=torch.int32), "track_id": ints(22000, N, K), "length": ints(60, N * K)}
        return self.tr

    def landmarks(self, kp, kp_depth, C, tracks, camera, threshold, min_obs, weights=None):
        self.lm = {"status": ints(24000, N * K), "n_kept": ints(25000, N * K), "rms": reals(50.0, N * K), "xyz": reals(51.0, N * K, 3)}
        return self.lm


@pytest.fixture
def pipe(monkeypatch):
    monkeypatch.setattr(lib, "chain_poses", lambda T, n_nodes=None, start=None, out=None: (torch.zeros((1, n_nodes, 12), dtype=torch.float64),))
    return StubPipeline()


def result_dictionary():
    """A StreamingSequence result of N frames matched at both spacings."""
    res = {"frames": {"keypoints_pixel": reals(72.0, N, K, 2).float(), "descriptors": reals(70.0, N, K, D).float(), "scores": reals(71.0, N, K).float()}}
    for s in SPACINGS:
        res[s] = {"matches": ints(28000 + 1000 * s, N - s, K, 2).long(), "match_count": ints(6000 + 100 * s, N - s)}
    return res


def counted(monkeypatch, call):
    """call()'s value, having seen it read the device exactly once."""
    reads, real = [], torch.Tensor.cpu
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", lambda t, *a, **kw: (reads.append(tuple(t.shape)), real(t, *a, **kw))[1])
        got = call()
    assert len(reads) == 1, reads
    return got


def same(got, want, at="result"):
    """Key order, Python types, dtypes, shapes and values, all the way down."""
    assert type(got) is type(want), (at, type(got), type(want))
    if isinstance(want, dict):
        assert list(got) == list(want), (at, list(got), list(want))
        for key in want:
            same(got[key], want[key], f"{at}[{key!r}]")
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape, (at, got.dtype, got.shape, want.dtype, want.shape)
        assert got.tobytes() == want.tobytes(), (at, got, want)
    else:
        assert got == want, (at, got, want)


# ------------------------------------------------------------------------------------ the expected dictionaries, from the stub's names
def t44(T, rows):
    T = T[rows].numpy().reshape(-1, 3, 4)
    return np.concatenate([T, np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (len(T), 1, 4))], axis=1)


def i64(t, rows):
    return t[rows].numpy().astype(np.int64)


def summaries(out, match_count, poses, pairs, spacing):
    out["inlier_ratio"] = np.where(match_count > 0, out["inlier_count"] / np.maximum(match_count, 1), 0.0)
    if spacing == 1:
        out["trajectory"] = od.chain(out["T"], None if poses is None else poses[pairs[0][0]])
    if poses is not None:
        out["rpe"] = od.rpe_summary(od.relative_pose_errors(out["T"], poses, pairs))
        out["ate"] = od.ate_summary(out["trajectory"], poses[:len(pairs) + 1]) if spacing == 1 else None


def want_pairs(pipe, match_count, pairs, rows, poses, spacing, refine):
    """What odometry(spacing=spacing, refine=refine) returns for `pairs`, rows `rows` of the launch."""
    est, mc = pipe.est, i64(match_count, rows)
    out = {"pairs": list(pairs), "T": t44(est["T"], rows)}
    out.update({key: i64(est[key], rows) for key in ("inlier_count", "usable_count", "best_hypothesis", "refit_kept")})
    out.update(match_count=mc, rms=est["rms"][rows].numpy().copy())
    if not refine:
        summaries(out, mc, poses, pairs, spacing)
        return out
    ransac = {key: out[key] for key in ("T", "inlier_count", "rms")}
    summaries(ransac, mc, poses, pairs, spacing)
    ref = pipe.ref
    out.update(T=t44(ref["T"], rows), inlier_count=i64(ref["inlier_count"], rows), rms=ref["rms"][rows].numpy().copy())
    summaries(out, mc, poses, pairs, spacing)
    out["ransac"] = ransac
    out["refine"] = {key: i64(ref[key], rows) for key in ("status", "iterations", "selected_count")}
    out["refine"].update(cost_in=ref["cost_in"][rows].numpy().copy(), cost=ref["cost"][rows].numpy().copy(), info=od.info_matrix(ref["info"][rows].numpy()))
    if "weight_sum" in ref:
        out["refine"]["weight_sum"] = ref["weight_sum"][rows].numpy().copy()
    return out


def want_graph(g, pairs, poses):
    C44 = t44(g["C"], slice(None))
    out = {"trajectory": np.stack([np.linalg.inv(c) for c in C44]), "pairs": pairs}
    out.update({key: int(g[key]) for key in ("status", "iterations", "used_edges", "skipped_edges", "failed_row")})
    out.update(cost_in=float(g["cost_in"]), cost=float(g["cost"]), edge_chi2=g["edge_chi2"].numpy().copy())
    if poses is not None:
        out["ate"] = od.ate_summary(out["trajectory"], poses[:N])
    if "cg_steps" in g:
        out["cg_steps"] = g["cg_steps"].numpy().astype(np.int64)
    return out


def want_spacings_and_graph(pipe, match_count, poses):
    out, at = {}, 0
    for s in SPACINGS:
        out[s] = want_pairs(pipe, match_count, LISTS[s], slice(at, at + len(LISTS[s])), poses, s, True)
        at += len(LISTS[s])
    out["graph"] = want_graph(pipe.graphs[0], PAIRS, poses)
    if poses is not None:
        out["graph"]["ate_chain"] = out[1]["ate"]
    return out


def result_match_count(res, more=()):
    return torch.cat([res[s]["match_count"][:len(LISTS[s])] for s in SPACINGS] + list(more))


# -------------------------------------------------------------------------------------------------------------------- the calls
@pytest.mark.parametrize("poses", (None, POSES), ids=("no_poses", "poses"))
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("refine", (False, True))
def test_odometry_result(pipe, monkeypatch, refine, spacing, poses):
    res = result_dictionary()
    got = counted(monkeypatch, lambda: od.odometry_result(pipe, res, kp_depth=ints(26000, N, K), camera=CAMERA, poses=poses, spacing=spacing,
                                                          refine=refine))
    assert ("ransac" in got) == refine
    same(got, want_pairs(pipe, res[spacing]["match_count"], LISTS[spacing], slice(0, N - spacing), poses, spacing, refine))


@pytest.mark.parametrize("poses", (None, POSES), ids=("no_poses", "poses"))
def test_odometry_weighted(pipe, monkeypatch, poses):
    depth = np.zeros((N, CAMERA.height, CAMERA.width), dtype=np.uint16)
    got = counted(monkeypatch, lambda: od.odometry(pipe, tokens=torch.zeros((N, 2, 3)), depth=depth, camera=CAMERA, poses=poses, refine=True,
                                                   weights=PoseWeights.product()))
    assert list(got["refine"])[-1] == "weight_sum"
    same(got, want_pairs(pipe, pipe.far["match_count"], LISTS[1], slice(0, N - 1), poses, 1, True))


@pytest.mark.parametrize("poses", (None, POSES), ids=("no_poses", "poses"))
def test_odometry_result_graph(pipe, monkeypatch, poses):
    res = result_dictionary()
    got = counted(monkeypatch, lambda: od.odometry_result_graph(pipe, res, kp_depth=ints(26000, N, K), camera=CAMERA, poses=poses))
    assert list(got) == [1, 2, "graph"]
    same(got, want_spacings_and_graph(pipe, result_match_count(res), poses))


@pytest.mark.parametrize("weighted", (False, True), ids=("plain", "weighted"))
def test_odometry_graph_with_tracks(pipe, monkeypatch, weighted):
    depth = np.zeros((N, CAMERA.height, CAMERA.width), dtype=np.uint16)
    got = counted(monkeypatch, lambda: od.odometry_graph(pipe, tokens=torch.zeros((N, 2, 3)), depth=depth, camera=CAMERA, poses=POSES, spacings=SPACINGS,
                                                         tracks=True, weights=PoseWeights.product() if weighted else None))
    assert list(got) == [1, 2, "graph", "tracks"] and ("weight_sum" in got[2]["refine"]) == weighted
    want = want_spacings_and_graph(pipe, pipe.far["match_count"], POSES)
    tr, lm, nt = pipe.tr, pipe.lm, 9
    length = length_statistics(tr["length"].numpy()[:nt].astype(np.int64), [nt])
    del length["n_tracks"]
    want["tracks"] = {"n_tracks": nt, "length": length, "track_id": tr["track_id"].numpy().copy(), "landmarks": lm["xyz"].numpy()[:nt].copy(),
                      "status": lm["status"].numpy()[:nt].copy(), "n_kept": lm["n_kept"].numpy()[:nt].copy(), "rms": lm["rms"].numpy()[:nt].copy()}
    same(got, want)
    # the links come from the spacing-1 rows of the launch, masked by the refinement's inliers of those rows
    assert torch.equal(pipe.linked["mask"], pipe.ref["inlier_of_slot"][:N - 1]) and torch.equal(pipe.linked["matches"]["match_count"], pipe.far["match_count"][:N - 1])


@pytest.mark.parametrize("poses", (None, POSES), ids=("no_poses", "poses"))
@pytest.mark.parametrize("prune_chi", (None, 2.5))
def test_odometry_result_loop_graph(pipe, monkeypatch, prune_chi, poses):
    res = result_dictionary()
    got = counted(monkeypatch, lambda: od.odometry_result_loop_graph(pipe, res, kp_depth=ints(26000, N, K), camera=CAMERA, poses=poses, prune_chi=prune_chi,
                                                                     loops=dict(per_frame=PER_FRAME, min_inliers=MIN_INLIERS)))
    names = ["loop_graph"] if prune_chi is None else ["loop_graph_unpruned", "loop_graph"]
    assert list(got) == [1, 2, "graph", "loops"] + names
    match_count = result_match_count(res, [pipe.far["match_count"]])
    want = want_spacings_and_graph(pipe, match_count, poses)
    cand, ref, slots = pipe.cand, pipe.ref, slice(P, P + L)
    kept = (np.array(CAND_FIRST) >= 0) & (ref["status"][slots].numpy() != lib.REFINE_NOT_ATTEMPTED) & (ref["inlier_count"][slots].numpy() >= MIN_INLIERS)
    assert kept.tolist() == [False] * 8 + [True, True]
    want["loops"] = {"first": np.array(CAND_FIRST, dtype=np.int32), "second": np.array(CAND_SECOND, dtype=np.int32), "sim": cand["sim"].numpy().copy(),
                     "count": cand["count"].numpy().copy(), "kept": kept, "match_count": i64(match_count, slots), "T": t44(ref["T"], slots),
                     "status": i64(ref["status"], slots), "inlier_count": i64(ref["inlier_count"], slots), "info": od.info_matrix(ref["info"][slots].numpy())}
    assert want["loops"]["sim"].dtype == np.float32 and want["loops"]["count"].dtype == np.int32
    all_pairs = PAIRS + list(zip(CAND_FIRST, CAND_SECOND))
    assert len(pipe.graphs) == 1 + len(names)
    for name, g in zip(names, pipe.graphs[1:]):
        want[name] = want_graph(g, all_pairs, poses)
        assert list(want[name])[-1] == "cg_steps" and want[name]["edge_chi2"].shape == (P + L,)
    same(got, want)
