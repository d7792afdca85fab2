"""libsslam_graph.so and libsslam_loop.so run at the size limits their headers state and with operands past 2^31 bytes
(tests/graph_limit_cases.py builds the cases, tests/test_graph_limit_cases_cpu.py holds them to their names), bit for bit and for
every output against the restatements (tests/pose_graph_ref.py, tests/loop_ref.py): tolerance none.

An operand past 2^31 bytes is built on the device from its at most 13 distinct graphs, chains or frames (tests/periodic.py) and
compared there, as integer bits, over the whole output.  After the passing comparison every case changes one input element at the
far end - the last chain, graph, frame or slot - and compares with the restatement's new result: the output changes there and,
where the items are independent, nowhere else.  A call one past a limit is refused by the entry itself, with its stated code,
nothing launched and the outputs untouched.

Every test frees what it allocated, prints its peak of device memory and asserts it below 24 GiB.  One test at a time.
profiles/graph_loop_limits.txt holds the audit of the index expressions, the measured durations and the peaks."""
import ctypes as C
import time

import numpy as np
import pytest

import graph_limit_cases as glc
import graph_table as gt
import loop_ref as lr
import loop_table as lt
import periodic as pd
import pose_graph_ref as pg
from test_gpu_size_limits import _dev, _memory

pytestmark = pytest.mark.gpu
SENTINEL = -0x0123456789abcdf
FLOAT_KEYS = ("C", "cost_in", "cost", "edge_chi2")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def lib():
    from sslam_amd import lib
    return lib


def _raw(T, t):
    return t.view(T.int64) if t.dtype == T.float64 else (t.view(T.int32) if t.dtype == T.float32 else t)


def _same(T, got, want, what):
    """A device tensor against a numpy expectation of its shape, on integer bits, compared where the output lives."""
    w = _dev(T, want)
    assert got.dtype == w.dtype and got.shape == w.shape, (what, got.dtype, w.dtype, tuple(got.shape), tuple(w.shape))
    bad = T.nonzero(_raw(T, got).reshape(-1) != _raw(T, w).reshape(-1)).flatten()
    assert bad.numel() == 0, f"{what}: differs from the restatement in {bad.numel()} elements of {got.numel()}, the first at flat index {int(bad[0])}: " \
                             f"{got.reshape(-1)[bad[0]].item()!r} for {w.reshape(-1)[bad[0]].item()!r}"
    print(f"{what}: 0 mismatching elements of {got.numel()}")


def _same_all(T, got, want, keys, what):
    """Every output of `keys`; `want` may be one graph's dict of the restatement's optimize(): scalars and arrays without the graph axis."""
    for key in keys:
        w = np.asarray(want[key])
        w = w.astype(np.float64 if key in FLOAT_KEYS else w.dtype if key == "sim" else np.int32).reshape(tuple(got[key].shape))
        _same(T, got[key], w, f"{what}, {key}")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _poison(T, tensors):
    for t in tensors:
        _raw(T, t).fill_(SENTINEL if t.element_size() == 8 else SENTINEL & 0x7fffffff)


def _untouched(T, tensors, what):
    for k, t in enumerate(tensors):
        r = _raw(T, t)
        assert bool((r == (SENTINEL if t.element_size() == 8 else SENTINEL & 0x7fffffff)).all()), f"{what}: a refused call wrote output {k}"


def _far_end(T, name, n, marked, expected, changed, out2, must_change):
    """Items that do not depend on each other: after the change of the last item's input, every output equals its old expectation
    everywhere but at the last item (and differs there, for the keys of must_change), and equals the new expectation everywhere."""
    last = pd.n_distinct(marked) - 1
    assert marked[-1] == n - 1
    for key, exp in expected.items():
        new = _dev(T, np.ascontiguousarray(changed[key])).view(exp.dtype).reshape(exp.shape[1:])
        moved = not T.equal(_raw(T, new), _raw(T, exp[last]))
        assert moved or key not in must_change, f"{name}: the change of the last item's input does not show in the restatement's {key}"
        bad, _ = pd.mismatches(out2[key], exp, marked)
        assert bad == ([n - 1] if moved else []), f"{name}, {key}: after changing the last item's input the output differs from the old expectation in items {bad[:8]}"
        exp2 = exp.clone()
        exp2[last] = new
        pd.report(out2[key], exp2, marked, f"{name}, {key}, last item changed")


# ------------------------------------------------------------------------------------------------------------------- chains
def test_chains_at_the_count_limit_past_2_31(T, lib):
    """8 388 607 chains of 3 nodes with C_start: C is 2.42 GB.  One chain more is refused by the entry with nothing launched and a
    poisoned C untouched."""
    c = glc.chains_at_the_count_limit_past_2_31()
    n, marked, name = c["n"], c["marked"], c["name"]
    assert n == gt.LIMITS["sslg_chain_poses"]["largest"]["n_graphs"] and n * c["frame_bytes"] > 1 << 31
    with _memory(T, name):
        whole_T = T.empty((n + 1, 2, 12), dtype=T.float64, device="cuda")
        whole_s = T.empty((n + 1, 12), dtype=T.float64, device="cuda")
        whole_C = T.empty((n + 1, 3, 12), dtype=T.float64, device="cuda")
        Td, sd = pd.build(_dev(T, c["T"]), n, marked, out=whole_T[:n]), pd.build(_dev(T, c["start"]), n, marked, out=whole_s[:n])
        whole_T[n], whole_s[n] = Td[0], sd[0]
        # one chain more: the entry itself, and the wrapper
        _poison(T, [whole_C])
        n0 = lib.graph_launch_count()
        assert lib.graph().sslg_chain_poses(_ptr(whole_T), _ptr(whole_s), n + 1, 3, _ptr(whole_C), None) == gt.E_UNSUPPORTED
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.chain_poses(whole_T, start=whole_s, out=whole_C)
        T.cuda.synchronize()
        assert lib.graph_launch_count() == n0, "a refused call launches nothing"
        _untouched(T, [whole_C], name)
        out = whole_C[:n]
        assert lib.chain_poses(Td, start=sd, out=out) is out and lib.graph_launch_count() == n0 + 1
        expected = _dev(T, c["want"])
        pd.report(out, expected, marked, name)
        Td[n - 1] = _dev(T, c["T_far"])                              # the last element of the last chain's last T
        lib.chain_poses(Td, start=sd, out=out)
        _far_end(T, name, n, marked, dict(C=expected), dict(C=c["want_far"]), dict(C=out), ("C",))
        del whole_T, whole_s, whole_C, Td, sd, out, expected


def test_chains_at_the_node_limit(T, lib):
    """4096 nodes, 257 chains (one thread past a workgroup) from [I | 0], chain i the distinct chain i % 3."""
    c = glc.chains_at_the_node_limit()
    assert c["n_nodes"] == gt.LIMITS["sslg_chain_poses"]["largest"]["n_nodes"]
    with _memory(T, c["name"]):
        slot = _dev(T, c["slot"])
        out = lib.chain_poses(_dev(T, c["T"])[slot].contiguous())
        want = _dev(T, c["want"])[slot]
        assert out.shape == (257, 4096, 12)
        bad = T.nonzero((_raw(T, out) != _raw(T, want)).reshape(257, -1).any(dim=1)).flatten().tolist()
        assert not bad, f"{c['name']}: {len(bad)} mismatching chains of 257: {bad[:8]}"
        print(f"{c['name']}: 0 mismatching chains of 257")
        del out, want, slot


# ------------------------------------------------------------------------------------------------------------------- graphs
def _graph_ops(T, c):
    return [_dev(T, np.ascontiguousarray(np.asarray(c[k])[None])) for k in glc.GRAPH_OPERANDS]


def _launch(T, lib, c, ops, sparse, keys):
    """One launch through the wrapper (which makes the outputs and the workspace), waited for and timed on the host."""
    T.cuda.synchronize()
    t0 = time.perf_counter()
    if sparse:
        out = lib.pose_graph_sparse(*ops, c["chi"], c["damping"], c["n_iter"], c["cg_iterations"], c["cg_tol"])
    else:
        out = lib.pose_graph(*ops, c["band"], c["chi"], c["damping"], c["n_iter"])
    T.cuda.synchronize()
    print(f"{c['name']}: the launch took {1e3 * (time.perf_counter() - t0):.1f} ms")
    return dict(zip(keys, out))


def _one_graph(T, lib, c, sparse, reference):
    """One graph at a limit: every output against the restatement, then the T of the far slot changed."""
    keys = lr.KEYS if sparse else pg.KEYS
    name = c["name"]

    def launch(ops):
        return _launch(T, lib, c, ops, sparse, keys)

    want = reference(c)
    with _memory(T, name):
        ops = _graph_ops(T, c)
        got = launch(ops)
        _same_all(T, got, want, keys, name)
        far = glc.with_far_slot(c)
        want2 = reference(far)
        assert want2["edge_chi2"][c["far_slot"]] != want["edge_chi2"][c["far_slot"]] and want2["C"].tobytes() != want["C"].tobytes(), \
            "the change of the far slot shows in the restatement"
        ops[2][0, c["far_slot"]] = _dev(T, c["T_far"])
        _same_all(T, launch(ops), want2, keys, name + ", far slot changed")
        del ops, got
    return want


def test_banded_at_the_node_and_band_limit(T, lib):
    """4096 nodes at band 32: 24 570 rows through the 198-row window in 158 KB of LDS, one iteration."""
    c = glc.banded_at_the_node_and_band_limit()
    assert len(c["C_in"]) == gt.MAX_NODES and c["band"] == gt.MAX_BAND
    want = _one_graph(T, lib, c, False, glc.run_banded)
    assert (want["status"], want["iterations"]) == (0, 1)


def test_banded_at_the_slot_limit(T, lib):
    """1 048 576 slots of one 40-node graph, 209 of them used: edge_chi2 whole, and the counts add up to the slot count."""
    c = glc.banded_at_the_slot_limit()
    assert len(c["first"]) == gt.MAX_EDGES
    want = _one_graph(T, lib, c, False, glc.run_banded)
    assert want["used_edges"] + want["skipped_edges"] + int((c["first"] == -1).sum()) == gt.MAX_EDGES


def test_sparse_at_the_node_and_slot_limit(T, lib):
    """4096 nodes and 65 536 slots: cur[] and the scan of prepare() at 16 nodes a thread, two iterations of 30 CG steps."""
    c = glc.sparse_at_the_node_and_slot_limit()
    assert len(c["C_in"]) == lt.MAX_NODES and len(c["first"]) == lt.MAX_EDGES
    want = _one_graph(T, lib, c, True, glc.run_sparse)
    assert want["status"] == 0 and want["cg_steps"][:3].tolist() == [30, 30, 0]


def _refused_graph_call(T, lib, sparse, ops, n_graphs, n_nodes, n_edges, c, n_iter, cg_iterations, code, what):
    """The entry itself, called with one argument past its limit on real operands: `code`, nothing launched, nothing written."""
    shapes = (lib.pose_graph_sparse_shapes if sparse else lib.pose_graph_shapes)(1, n_nodes, n_edges)
    keys = lr.KEYS if sparse else pg.KEYS
    outs = [T.empty(shapes[k][0], dtype=shapes[k][1], device="cuda") for k in keys]
    ws = T.empty(64, dtype=T.uint8, device="cuda")
    _poison(T, outs)
    count = lib.loop_launch_count if sparse else lib.graph_launch_count
    n0 = count()
    head = [_ptr(t) for t in ops[:4]] + [n_graphs, n_nodes, n_edges, _ptr(ops[4])]
    if sparse:
        rc = lib.loop().ssll_pose_graph_sparse(*head, C.c_double(c["chi"]), C.c_double(c["damping"]), n_iter, cg_iterations, C.c_double(c["cg_tol"]),
                                               _ptr(ws), *[_ptr(t) for t in outs], None)
    else:
        rc = lib.graph().sslg_pose_graph(*head, c["band"], C.c_double(c["chi"]), C.c_double(c["damping"]), n_iter, _ptr(ws), *[_ptr(t) for t in outs], None)
    T.cuda.synchronize()
    assert rc == code, (what, rc)
    assert count() == n0, f"{what}: a refused call launches nothing"
    _untouched(T, outs, what)


def _many_graphs(T, lib, c, sparse):
    """65 535 graphs from 10 distinct ones: every output of every graph on the device, then the last graph's last used slot changed;
    one graph more refused."""
    keys = lr.KEYS if sparse else pg.KEYS
    n, marked, name, want = c["n"], c["marked"], c["name"], c["want"]
    d = pd.n_distinct(marked)
    assert n * c["frame_bytes"] > 1 << 31 and c["workspace_bytes"] > 4 << 31      # frame_bytes: of the operand the marks follow

    def launch(ops):
        return _launch(T, lib, c, ops, sparse, keys)

    with _memory(T, name):
        distinct = [_dev(T, c[k]) for k in glc.GRAPH_OPERANDS]       # d + 1 rows: the last is the changed last graph
        ops = [pd.build(t[:d], n, marked) for t in distinct]
        if sparse:
            assert lib.pose_graph_sparse_workspace_bytes(n, c["n_nodes"], c["n_edges"]) == c["workspace_bytes"]
        else:
            assert lib.pose_graph_workspace_bytes(n, c["n_nodes"], c["band"]) == c["workspace_bytes"]
        _refused_graph_call(T, lib, sparse, ops, n + 1, c["n_nodes"], c["n_edges"], c, c["n_iter"], c["cg_iterations"] if sparse else None, gt.E_UNSUPPORTED, name + ", one graph more")
        expected = {k: _dev(T, np.ascontiguousarray(want[k][:d])) for k in keys}
        got = launch(ops)
        for k in keys:
            pd.report(got[k], expected[k], marked, f"{name}, {k}")
        del got
        for t, dt in zip(ops, distinct):
            t[n - 1] = dt[d]
        _far_end(T, name, n, marked, expected, {k: want[k][d] for k in keys}, launch(ops), ("C", "cost", "edge_chi2"))
        del ops, distinct, expected


def test_banded_at_the_graph_limit_past_2_31(T, lib):
    """4 nodes, 200 slots: edge_info 2.20 GB, the workspace 12.4 GB - the bytes of gi * n_edges * 21 and gi * ws_words past 2^31;
    one graph of the seven repeating ones is not attempted, one fails its first pivot."""
    c = glc.banded_at_the_graph_limit_past_2_31()
    assert c["n"] * c["n_edges"] * 21 * 8 > 1 << 31
    _many_graphs(T, lib, c, False)


def test_sparse_at_the_graph_limit_past_2_31(T, lib):
    """The same graphs through ssll_pose_graph_sparse: the workspace is 9.7 GB, cg_steps compared for every graph."""
    c = glc.sparse_at_the_graph_limit_past_2_31()
    assert c["n"] * c["n_edges"] * 21 * 8 > 1 << 31
    _many_graphs(T, lib, c, True)


def test_banded_workspace_past_2_31_words(T, lib):
    """20 nodes at band 19, 40 slots: 37 302 workspace words a graph, so gi * ws_words itself, not only its bytes, passes 2^31 - at
    graph 57 570, which has operands of its own.  The workspace is 19.6 GB."""
    c = glc.banded_workspace_past_2_31_words()
    assert c["marked"][1] * c["workspace_words"] <= 1 << 31 < (c["marked"][1] + 1) * c["workspace_words"] and c["workspace_bytes"] < 20 << 30
    _many_graphs(T, lib, c, False)


def test_sparse_at_the_iteration_limits(T, lib):
    """Two small launches on twelve_nodes_two_loops: 16 accepted steps (every word of steps_of[]), and cg_iterations 4096 with
    cg_tol 0; n_iter 17 and cg_iterations 4097 are refused by the entry with nothing written."""
    with _memory(T, "sparse_at_the_iteration_limits"):
        for c in (glc.sparse_at_the_iteration_limit(), glc.sparse_at_the_cg_limit()):
            want = glc.run_sparse(c)
            ops = _graph_ops(T, c)
            got = dict(zip(lr.KEYS, lib.pose_graph_sparse(*ops, c["chi"], c["damping"], c["n_iter"], c["cg_iterations"], c["cg_tol"])))
            _same_all(T, got, want, lr.KEYS, c["name"])
            if c["n_iter"] == lt.MAX_ITER:
                assert want["iterations"] == 16 and want["cg_steps"][15] > 0
            else:
                assert want["cg_steps"][0] == c["cg_first"]
                print(f"{c['name']}: {c['cg_first']} CG steps, the loop ended by {c['cg_ended']!r}")
        n_nodes, n_edges = len(c["C_in"]), len(c["first"])
        _refused_graph_call(T, lib, True, ops, 1, n_nodes, n_edges, c, lt.MAX_ITER + 1, 30, lt.E_INVALID, "n_iter 17")
        _refused_graph_call(T, lib, True, ops, 1, n_nodes, n_edges, c, 1, lt.MAX_CG + 1, lt.E_UNSUPPORTED, "cg_iterations 4097")
        with pytest.raises(ValueError):
            lib.pose_graph_sparse(*ops, iterations=lt.MAX_ITER + 1)
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.pose_graph_sparse(*ops, cg_iterations=lt.MAX_CG + 1)
        del ops, got


# --------------------------------------------------------------------------------------------------------------- signatures
@pytest.mark.parametrize("which", ["frame_limit", "keypoint_limit"])
def test_signatures_past_2_31(T, lib, which):
    """4096 frames of 520 keypoints at width 256 (2.18 GB) and 1030 frames of 4096 keypoints at width 128 (2.16 GB), periodic frames.
    The signatures are centred on the sequence's mean: after the change of the last descriptor element every row may move, the
    device equals the new restatement."""
    c = glc.signatures_at_the_frame_limit_past_2_31() if which == "frame_limit" else glc.signatures_at_the_keypoint_limit_past_2_31()
    n, marked, name = c["n"], c["marked"], c["name"]
    assert n * c["frame_bytes"] > 1 << 31
    assert c["want"][-1].tobytes() != c["want_far"][-1].tobytes(), "the change shows in the restatement's last row"
    with _memory(T, name):
        desc, scores = pd.build(_dev(T, c["desc"]), n, marked), pd.build(_dev(T, c["scores"]), n, marked)
        assert desc.numel() * 4 > 1 << 31
        n0 = lib.loop_launch_count()
        _same(T, lib.frame_signatures(desc, scores), c["want"], name)
        assert lib.loop_launch_count() == n0 + 2
        desc[n - 1] = _dev(T, c["desc_far"])
        _same(T, lib.frame_signatures(desc, scores), c["want_far"], name + ", last descriptor element changed")
        del desc, scores


# --------------------------------------------------------------------------------------------------------------- candidates
def test_candidates_at_the_frame_limit(T, lib):
    """4096 frames, 8 picks a frame: S[4096] in LDS filled to its end, exact ties all over the range; one frame more refused."""
    c = glc.candidates_at_the_frame_limit()
    n, name = c["n"], c["name"]
    assert n == lt.MAX_FRAMES and c["per_frame"] == lt.MAX_PER_FRAME
    with _memory(T, name):
        whole = T.zeros((n + 1, c["d"]), dtype=T.float32, device="cuda")
        whole[:n] = _dev(T, c["sig"])
        whole[n] = whole[0]
        got = dict(zip(lr.CANDIDATE_KEYS, lib.loop_candidates(whole[:n], c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"])))
        _same_all(T, got, c["want"], lr.CANDIDATE_KEYS, name)
        shapes = lib.loop_candidate_shapes(n + 1, c["per_frame"])
        outs = [T.empty(shapes[k][0], dtype=shapes[k][1], device="cuda") for k in lr.CANDIDATE_KEYS]
        _poison(T, outs)
        n0 = lib.loop_launch_count()
        rc = lib.loop().ssll_loop_candidates(_ptr(whole), n + 1, c["d"], c["min_gap"], C.c_float(c["min_sim"]), c["per_frame"], c["suppress"],
                                             *[_ptr(t) for t in outs], None)
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.loop_candidates(whole, c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"])
        T.cuda.synchronize()
        assert rc == lt.E_UNSUPPORTED and lib.loop_launch_count() == n0, "one frame more is refused, nothing launched"
        _untouched(T, outs, name)
        del whole, got, outs
