"""The cases of tests/graph_limit_cases.py held to what their names say, by the restatements alone and without a device: each
sits at the limit tests/graph_table.py or tests/loop_table.py names (read from the table), the named operand passes 2^31 bytes, the
marked positions are distinct and what tests/periodic.py marks, the restatement gives the statuses, step counts and picks the
device test relies on, the far-end change shows in the restatement's output, and no periodic operand has more than 13 distinct
items.  The big cases are built once per process (the builders cache)."""
import numpy as np
import pytest

import graph_limit_cases as glc
import graph_table as gt
import loop_ref as lr
import loop_table as lt
import pose_graph_ref as pg

FAR = 1 << 31
GRAPH, SPARSE = gt.LIMITS["sslg_pose_graph"]["largest"], lt.LIMITS["ssll_pose_graph_sparse"]["largest"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not np.array_equal(_bits(a), _bits(b))


def _periodic(c, operand_frame_bytes):
    """The marks are periodic.py's for the case's frame, distinct, {0, the holder of byte 2^31, n - 1}; at most 13 distinct items."""
    import periodic as pd
    n, marked = c["n"], c["marked"]
    assert n * operand_frame_bytes > FAR and operand_frame_bytes == c["frame_bytes"], "the named operand passes 2^31 bytes"
    assert marked == pd.marks(n, c["frame_bytes"]) == [0, FAR // c["frame_bytes"], n - 1] and len(set(marked)) == 3
    assert 0 < marked[1] < n - 1
    assert pd.n_distinct(marked) == glc.P + 3 <= 13
    assert np.array_equal(glc.slots(n, marked), pd.slots(n, marked).numpy())
    return glc.P + 3


def test_the_wrapper_takes_as_many_chains_as_the_entry():
    """chain_poses refuses above the entry's own limit, 0x7fffffff / 256 chains, not above the pose graph's 65 535 graphs."""
    import torch
    from sslam_amd import lib
    assert lib.GRAPH_MAX_CHAINS == gt.LIMITS["sslg_chain_poses"]["largest"]["n_graphs"] == 0x7fffffff // 256
    with pytest.raises(ValueError, match="CUDA"):                    # accepted as far as a host without a device can tell
        lib.chain_poses(torch.zeros((gt.MAX_GRAPHS + 1, 1, 12), dtype=torch.float64))
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.chain_poses(torch.empty((lib.GRAPH_MAX_CHAINS + 1, 1, 12), dtype=torch.float64))


def test_chains_at_the_count_limit_past_2_31():
    c = glc.chains_at_the_count_limit_past_2_31()
    assert c["n"] == gt.LIMITS["sslg_chain_poses"]["largest"]["n_graphs"] and c["n_nodes"] == 3
    d = _periodic(c, c["n_nodes"] * 96)                              # C
    assert c["n"] * 2 * 96 < FAR, "T stays below"
    assert c["T"].shape == (d, 2, 12) and c["start"].shape == (d, 12) and c["want"].shape == (d, 3, 12)
    assert len({c["want"][i].tobytes() for i in range(d)}) == d, "every distinct chain has its own result"
    assert np.array_equal(_bits(c["want"][:, 0]), _bits(c["start"])), "C_0 is C_start"
    assert _differ(c["want_far"], c["want"][-1]) and np.array_equal(_bits(c["want_far"][:2]), _bits(c["want"][-1][:2])), \
        "the last T's last element moves the last pose and no other"


def test_chains_at_the_node_limit():
    c = glc.chains_at_the_node_limit()
    assert c["n_nodes"] == gt.LIMITS["sslg_chain_poses"]["largest"]["n_nodes"] == gt.MAX_NODES and c["n"] == 257
    assert c["want"].shape == (3, c["n_nodes"], 12) and np.isfinite(c["want"]).all() and sorted(set(c["slot"].tolist())) == [0, 1, 2]
    assert len({w.tobytes() for w in c["want"][:, -1]}) == 3
    R = c["want"][:, -1].reshape(3, 3, 4)[:, :, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-9, "4095 products later the poses are still rigid"


@pytest.fixture(scope="module")
def banded_big():
    c = glc.banded_at_the_node_and_band_limit()
    return c, glc.run_banded(c)


def test_banded_at_the_node_and_band_limit(banded_big):
    c, want = banded_big
    n_nodes = len(c["C_in"])
    assert n_nodes == GRAPH["n_nodes"] and c["band"] == GRAPH["band"] == gt.MAX_BAND and c["n_iter"] == 1
    rows, M = 6 * (n_nodes - 1), 6 * c["band"] + 6
    assert (rows, M, rows - M) == (24570, 198, 24372), "the window slides 24 372 times"
    assert (c["second"] - c["first"]).max() == c["band"] and want["used_edges"] == len(c["first"]) and want["skipped_edges"] == 0
    assert (want["status"], want["iterations"], want["failed_row"]) == (0, 1, -1), "the one step is accepted: the solve shows in C"
    assert _differ(want["C"][-1], c["C_in"][-1]) and want["cost"] < want["cost_in"]
    # the far end: the last used slot names the last node; its change shows without a solve (the device test takes the whole new result)
    far = c["far_slot"]
    assert far == len(c["first"]) - 1 and c["second"][far] == n_nodes - 1
    a, b = glc.run_banded(c, n_iter=0), glc.run_banded(glc.with_far_slot(c), n_iter=0)
    changed = np.flatnonzero(a["edge_chi2"] != b["edge_chi2"])
    assert changed.tolist() == [far] and a["cost_in"] != b["cost_in"]


def test_banded_at_the_slot_limit():
    c = glc.banded_at_the_slot_limit()
    E = len(c["first"])
    assert E == GRAPH["n_edges"] == gt.MAX_EDGES and len(c["C_in"]) == 40 and c["band"] == 20
    assert E * 21 * 8 < FAR, "no operand of one graph reaches 2^31 bytes"
    G = pg.Graph(c["first"], c["second"], c["T"], c["info"], 40, 20)
    assert {0, 255, 256, E - 1} <= set(G.slots.tolist()) and set(G.slots.tolist()) == set(c["planted_at"].tolist()) | set(c["duplicates_at"].tolist())
    absent = int((c["first"] == -1).sum())
    want = glc.run_banded(c)
    assert want["used_edges"] == 149 + 60 and want["skipped_edges"] == 400 == len(c["skipped_at"]) and want["used_edges"] + want["skipped_edges"] + absent == E
    assert not G.used[c["skipped_at"]].any() and (c["first"][c["skipped_at"]] != -1).all()
    assert np.isnan(c["T"][c["first"] == -1]).any(), "some absent slots hold NaN"
    assert want["status"] == 0 and want["iterations"] >= 1 and want["edge_chi2"].shape == (E,)
    assert np.array_equal(np.flatnonzero(want["edge_chi2"]), G.slots)
    far = glc.run_banded(glc.with_far_slot(c))
    assert c["far_slot"] == E - 1 and far["edge_chi2"][E - 1] != want["edge_chi2"][E - 1] and _differ(far["C"], want["C"])


def _small_graph_conditions(c, want, frame, n_nodes=4, n_edges=200):
    d = _periodic(c, frame)
    assert (c["n"], c["n_nodes"], c["n_edges"]) == (gt.MAX_GRAPHS, n_nodes, n_edges)
    assert c["C_in"].shape == (d + 1, n_nodes, 12) and c["first"].shape == (d + 1, n_edges) and c["workspace_bytes"] > 4 * FAR
    status = want["status"].tolist()
    assert status[glc.NOT_ATTEMPTED] == 3 and status[glc.FAILED_PIVOT] == 2 and want["failed_row"][glc.FAILED_PIVOT] == 6
    assert all(s == 0 for g, s in enumerate(status) if g not in (glc.NOT_ATTEMPTED, glc.FAILED_PIVOT)), status
    assert (want["iterations"][np.array(status) == 0] >= 1).all()
    assert (want["used_edges"] + want["skipped_edges"] + (c["first"] == -1).sum(axis=1) == n_edges).all() and (want["skipped_edges"] >= 3).all()
    assert len({want["C"][g].tobytes() for g in range(d)}) == d
    assert pg.used_mask(c["first"][d], c["second"][d], c["T"][d], c["info"][d], n_nodes, c["band"])[n_edges - 1], "the last slot is used"
    changed = [k for k in glc.GRAPH_OPERANDS if _differ(c[k][d], c[k][d - 1])]
    assert changed == ["T"] and np.flatnonzero((c["T"][d].view(np.int64) != c["T"][d - 1].view(np.int64)).any(axis=1)).tolist() == [n_edges - 1]
    for key in ("C", "cost", "edge_chi2"):
        assert _differ(want[key][d], want[key][d - 1]), key
    for key in ("used_edges", "skipped_edges"):
        assert want[key][d] == want[key][d - 1]
    return d


def test_banded_at_the_graph_limit_past_2_31():
    c = glc.banded_at_the_graph_limit_past_2_31()
    _small_graph_conditions(c, c["want"], 200 * 21 * 8)             # edge_info
    assert c["band"] == 3 and c["workspace_bytes"] == 8 * 65535 * (18 * 24 + 54 + 48 + 256 * 90) > 12 * 10 ** 9
    assert c["n"] * 200 * 96 + c["n"] * 200 * 168 + c["workspace_bytes"] < 17 * 10 ** 9, "T, info and the workspace: below the 24 GiB cap with room"


def test_sparse_at_the_graph_limit_past_2_31():
    c = glc.sparse_at_the_graph_limit_past_2_31()
    d = _small_graph_conditions(c, c["want"], 200 * 21 * 8)
    assert 9.6e9 < c["workspace_bytes"] < 9.8e9
    cg = c["want"]["cg_steps"]
    assert cg.shape == (d + 1, lt.MAX_ITER) and not cg[glc.NOT_ATTEMPTED].any() and not cg[glc.FAILED_PIVOT].any()
    good = c["want"]["status"] == 0
    assert (cg[good, 0] > 0).all() and (cg[good].max(axis=1) < c["cg_iterations"]).all(), "every good graph's CG converges below the count"


def test_banded_workspace_past_2_31_words():
    """No element index of the two cases above leaves 31 bits; this one's graph * workspace words does."""
    small = glc.banded_at_the_graph_limit_past_2_31()
    assert small["n"] * 200 * 21 < FAR and small["workspace_bytes"] // 8 < FAR
    c = glc.banded_workspace_past_2_31_words()
    words = gt.workspace_bytes(1, glc.WIDE_NODES, glc.WIDE_BAND) // 8
    assert c["band"] == glc.WIDE_BAND < gt.MAX_BAND and c["workspace_words"] == words == 37302
    _small_graph_conditions(c, c["want"], words, glc.WIDE_NODES, 40)                   # the marks count workspace words
    assert c["workspace_bytes"] == 8 * c["n"] * words and c["workspace_bytes"] + c["n"] * 40 * (96 + 168 + 8) + 2 * c["n"] * 20 * 96 < 21 << 30
    assert (c["second"] - c["first"])[c["first"] >= 0].max() == c["band"]


def test_sparse_at_the_node_and_slot_limit():
    c = glc.sparse_at_the_node_and_slot_limit()
    E0, E = c["padding"]
    assert len(c["C_in"]) == SPARSE["n_nodes"] and len(c["first"]) == E == SPARSE["n_edges"] and E0 == 65440
    G = lr.SparseGraph(c["first"], c["second"], c["T"], c["info"], len(c["C_in"]))
    assert not G.used[E0:E0 + 4].any() and G.used[E0 + 4:].all() and G.used[:E0].all() and c["first"][E0] == -1 and G.skipped == 3
    assert (c["second"] - c["first"])[G.used].max() == 4000 and G.degree.max() >= 32
    want = glc.run_sparse(c)
    assert (want["status"], want["iterations"]) == (0, 2) and want["cg_steps"][:3].tolist() == [30, 30, 0]
    assert want["used_edges"] == E - 4 and want["skipped_edges"] == 3
    far = glc.run_sparse(glc.with_far_slot(c))
    assert c["far_slot"] == E - 1 and far["edge_chi2"][E - 1] != want["edge_chi2"][E - 1] and _differ(far["C"], want["C"])
    assert far["status"] == 0


def test_sparse_at_the_iteration_limits():
    c = glc.sparse_at_the_iteration_limit()
    assert c["n_iter"] == lt.MAX_ITER == 16 and c["damping"] == glc.FULL_ITERATIONS_DAMPING
    want = glc.run_sparse(c)
    assert want["status"] == 0 and want["iterations"] == 16 and want["cg_steps"][15] > 0 and (want["cg_steps"] > 0).all(), "every word of steps_of[] is filled"
    assert (want["cg_steps"] < c["cg_iterations"]).all()
    c = glc.sparse_at_the_cg_limit()
    assert c["cg_iterations"] == SPARSE["cg_iterations"] == lt.MAX_CG and c["cg_tol"] == 0.0 and c["n_iter"] == 1
    want = glc.run_sparse(c)
    assert want["cg_steps"][0] == c["cg_first"] and not want["cg_steps"][1:].any() and c["cg_ended"] in ("count", "pq", "tol")
    assert (c["cg_ended"] == "count") == (c["cg_first"] == lt.MAX_CG)
    assert c["cg_first"] > 40, "past where cg_tol 1e-3 would have stopped it"
    print(f"cg_tol 0: the restatement's CG loop took {c['cg_first']} steps and ended by {c['cg_ended']!r}")


@pytest.mark.parametrize("which", ["frame", "keypoint"])
def test_signatures_past_2_31(which):
    L = lt.LIMITS["ssll_frame_signatures"]["largest"]
    if which == "frame":
        c = glc.signatures_at_the_frame_limit_past_2_31()
        assert (c["n"], c["k"], c["d"]) == (L["n_frames"], 520, L["d"]) and c["n"] * c["k"] * c["d"] * 4 == 2181038080
    else:
        c = glc.signatures_at_the_keypoint_limit_past_2_31()
        assert (c["n"], c["k"], c["d"]) == (1030, L["k"], 128) and c["n"] * c["k"] * c["d"] * 4 == 2160066560
    d = _periodic(c, c["k"] * c["d"] * 4)
    assert c["desc"].shape == (d, c["k"], c["d"]) and c["want"].shape == (c["n"], c["d"]) and c["want"].dtype == np.float32
    assert np.abs(np.linalg.norm(c["want"].astype(np.float64), axis=1) - 1).max() < 1e-5
    s = glc.slots(c["n"], c["marked"])
    small = lr.signatures(c["desc"][s[:40]], c["scores"][s[:40]])    # the split changed no arithmetic: 40 frames both ways
    assert np.array_equal(_bits(small), _bits(lr.finish_signatures(lr.raw_signatures(c["desc"], c["scores"])[s[:40]])))
    assert _differ(c["want_far"][-1], c["want"][-1]), "the last descriptor element moves the last row"


def test_candidates_at_the_frame_limit():
    c = glc.candidates_at_the_frame_limit()
    L = lt.LIMITS["ssll_loop_candidates"]["largest"]
    n, per = c["n"], c["per_frame"]
    assert (n, c["d"], per) == (L["n_frames"], L["d"], L["per_frame"]) and (c["min_gap"], c["suppress"]) == (30, 5)
    assert len(c["rows"]) <= 200 and c["sig"].shape == (n, 256) and c["S"].shape == (n, n)
    own = [0, 255, 256, n - 2, n - 1]
    assert all((c["slot"] == c["slot"][f]).sum() == 1 for f in own), "rows of their own"
    assert np.abs(np.linalg.norm(c["rows"].astype(np.float64), axis=1) - 1).max() < 1e-6
    probe = [0, 1, 255, 256, 2000, n - 1]                            # the expanded matrix is the matrix: six whole rows the long way
    long_way = np.zeros((len(probe), n), np.float32)
    for col in range(c["d"]):
        long_way = lr.fmaf32(c["sig"][probe][:, None, col], c["sig"][None, :, col], long_way)
    assert np.array_equal(_bits(long_way), _bits(c["S"][probe]))
    w = c["want"]
    first, count = w["first"].reshape(n, per), w["count"]
    assert count.sum() > 0 and (count == per).any(), "some frame fills all 8 slots"
    assert (first >= n - 256).any(), "some pick lies in the workgroup's last stride"
    assert first[glc.LATE_AGAIN, 0] == glc.LATE_FIRST
    tie = 0
    for i in np.flatnonzero(count > 0):
        row = c["S"][i, :i - c["min_gap"] + 1]
        best = np.flatnonzero(row == w["sim"][i * per])
        tie += first[i, 0] == best[0] and len(set(((best % 256) // 64).tolist())) > 1
    assert tie > 100, "the first pick of many frames is the lowest of equal values held by different waves"
