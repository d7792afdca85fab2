"""libsslam_loop.so on the device against its restatement (tests/loop_ref.py), bit for bit and for every output: the signatures at
every keypoint count around a wave and both widths, the candidates below, at and past one stride of the workgroup with the
contract's tie, gap and suppression rows, the sparse pose graph on edges past any band - a hub, an unreachable node, rows one past
the workgroup's stride, the conjugate gradients cut short and run to the end - several graphs in one launch, every pointer at its
least alignment, outputs and workspace in poisoned guarded buffers (tests/guarded.py), repeatability, a captured graph - and
odometry_loop_graph on a short synthetic sequence against the restatement fed the same device-produced edges."""
import numpy as np
import pytest

import guarded
import loop_cases as lc
import loop_ref as ref
import loop_table as lt

pytestmark = pytest.mark.gpu
KEYS = ref.KEYS


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what, keys):
    for key in keys:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(_bits(g).reshape(-1) != _bits(w).reshape(-1))
        assert bad.size == 0, f"{what}: {key} differs from the restatement in {bad.size} elements, the first at flat index {bad[0]}: " \
                              f"{g.reshape(-1)[bad[0]]!r} for {w.reshape(-1)[bad[0]]!r}"


def _in(T, a, name):
    """A guarded input; float64 travels as int64 bits (tests/guarded.py has no float64 sentinel)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        whole, mid = guarded.guarded_input(T, a.view(np.int64), name=name)
        return whole, mid.view(T.float64)
    return guarded.guarded_input(T, a, name=name)


def _out(T, shape, dtype, name):
    if dtype == T.float64:
        whole, mid = guarded.guarded(T, shape, T.int64, name=name)
        return whole, mid.view(T.float64)
    return guarded.guarded(T, shape, dtype, name=name)


def _raw(T, t):
    return t.view(T.int64) if t.dtype == T.float64 else t


def _check(T, ins, outs, ws, what):
    for name, (whole, mid) in list(ins.items()) + list(outs.items()) + ([("workspace", ws)] if ws is not None else []):
        guarded.assert_guards(whole, _raw(T, mid), f"{what} {name}")
    for name, (_, mid) in outs.items():
        guarded.assert_written(_raw(T, mid), f"{what} {name}")


def _counts():
    from sslam_amd import lib
    return lib.loop_launch_count(), lib.launch_count(), lib.ext_launch_count(), lib.graph_launch_count()


def _only_the_fourth_library(before, launches):
    after = _counts()
    assert after[0] - before[0] == launches and after[1:] == before[1:], f"{launches} launches, of the fourth library"


# ------------------------------------------------------------------------------------------------------------------ signatures
def run_signatures(T, desc, scores, what):
    from sslam_amd import lib
    ins = dict(desc=_in(T, desc, "desc"), scores=_in(T, scores, "scores"))
    outs = dict(sig=_out(T, (desc.shape[0], desc.shape[2]), T.float32, "sig"))
    ws = guarded.guarded(T, lt.signature_workspace_bytes(desc.shape[0], desc.shape[2]), T.uint8, name="workspace")
    before = _counts()
    back = lib.frame_signatures(ins["desc"][1], ins["scores"][1], out=outs["sig"][1], workspace=ws[1])
    T.cuda.synchronize()
    _only_the_fourth_library(before, 2)
    assert back is outs["sig"][1]
    _check(T, ins, outs, ws, what)
    assert np.array_equal(_bits(ins["desc"][1].cpu().numpy()), _bits(desc)), "the input was written"
    return outs["sig"][1].cpu().numpy()


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 500])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_signatures_equal_the_restatement(T, n, k, d):
    desc, scores = lc.bank(n, k, d, 100 * n + k + d, zero_frame=1 if n >= 3 else None)
    got = run_signatures(T, desc, scores, f"signatures {n} {k} {d}")
    _same(dict(sig=got), dict(sig=ref.signatures(desc, scores)), f"signatures {n} {k} {d}", ("sig",))
    if n == 1:
        assert (got == 0).all(), "one frame: the centred signature is zero"
    else:
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-5


def test_one_frame_gives_a_zero_signature_and_no_candidates(T):
    from sslam_amd import lib
    desc, scores = lc.bank(1, 64, 128, 9)
    sig = lib.frame_signatures(T.from_numpy(desc).cuda(), T.from_numpy(scores).cuda())
    first, second, sim, count = lib.loop_candidates(sig, min_gap=1, min_sim=-1.0, per_frame=3, suppress=0)
    assert (sig == 0).all() and count.tolist() == [0] and first.tolist() == [-1] * 3 and second.tolist() == [-1] * 3 and (sim == 0).all()


# ------------------------------------------------------------------------------------------------------------------ candidates
def run_candidates(T, c, what):
    from sslam_amd import lib
    n = len(c["sig"])
    ins = dict(sig=_in(T, c["sig"], "sig"))
    shapes = lib.loop_candidate_shapes(n, c["per_frame"])
    outs = {k: _out(T, shapes[k][0], shapes[k][1], k) for k in ref.CANDIDATE_KEYS}
    before = _counts()
    back = lib.loop_candidates(ins["sig"][1], c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"], out=tuple(outs[k][1] for k in ref.CANDIDATE_KEYS))
    T.cuda.synchronize()
    _only_the_fourth_library(before, 1)
    assert all(b is outs[k][1] for b, k in zip(back, ref.CANDIDATE_KEYS))
    _check(T, ins, outs, None, what)
    return {k: outs[k][1].cpu().numpy() for k in ref.CANDIDATE_KEYS}


CANDIDATES = lc.candidate_size_cases() + lc.candidate_cases()


@pytest.mark.parametrize("index", range(len(CANDIDATES)), ids=[c["name"] for c in CANDIDATES])
def test_candidates_equal_the_restatement(T, index):
    c = CANDIDATES[index]
    want = ref.candidates(c["sig"], c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"])
    _same(run_candidates(T, c, c["name"]), want, c["name"], ref.CANDIDATE_KEYS)
    if c["name"] in ("n_2", "n_64", "n_65", "n_300", "duplicate_frames", "suppression_clipped_at_frame_0", "per_frame_8"):
        assert want["count"].sum() > 0, "the case proposes pairs"


# ------------------------------------------------------------------------------------------------------------ the sparse graph
NAMES = dict(first="edge_first", second="edge_second", T="edge_T", info="edge_info", C_in="C_in")


def run_sparse(T, ops, c, what):
    """One guarded launch of ssll_pose_graph_sparse on stacked operands (graph axis first) -> dict of numpy arrays."""
    from sslam_amd import lib
    n_graphs, n_nodes, n_edges = ops["C_in"].shape[0], ops["C_in"].shape[1], ops["first"].shape[1]
    ins = {NAMES[k]: _in(T, ops[k], NAMES[k]) for k in NAMES}
    shapes = lib.pose_graph_sparse_shapes(n_graphs, n_nodes, n_edges)
    outs = {k: _out(T, shapes[k][0], shapes[k][1], k) for k in KEYS}
    ws = guarded.guarded(T, lib.pose_graph_sparse_workspace_bytes(n_graphs, n_nodes, n_edges), T.uint8, name="workspace")
    before = _counts()
    back = lib.pose_graph_sparse(*(ins[NAMES[k]][1] for k in NAMES), c["chi"], c["damping"], c["n_iter"], c["cg_iterations"], c["cg_tol"],
                                 out=tuple(outs[k][1] for k in KEYS), workspace=ws[1])
    T.cuda.synchronize()
    _only_the_fourth_library(before, 1)
    assert all(b is outs[k][1] for b, k in zip(back, KEYS))
    _check(T, ins, outs, ws, what)
    for k in NAMES:
        assert np.array_equal(_bits(ins[NAMES[k]][1].cpu().numpy()), _bits(ops[k])), f"{what}: input {k} was written"
    return {k: outs[k][1].cpu().numpy() for k in KEYS}


def _one(case):
    return {k: np.ascontiguousarray(np.asarray(case[k])[None]) for k in NAMES}


def _want(ops, c):
    return ref.optimize_graphs(ops["first"], ops["second"], ops["T"], ops["info"], ops["C_in"], c["chi"], c["damping"], c["n_iter"], c["cg_iterations"],
                               c["cg_tol"])


SPARSE = lc.sparse_cases()
STATUS = dict(exact_graph_plus_0_4=1, unreachable_node=2, no_iterations=1)


@pytest.mark.parametrize("index", range(len(SPARSE)), ids=[c["name"] for c in SPARSE])
def test_sparse_graphs_equal_the_restatement(T, index):
    c = SPARSE[index]
    ops = _one(c)
    want = _want(ops, c)
    assert want["status"][0] == STATUS.get(c["name"], 0), "the case is what its name says"
    got = run_sparse(T, ops, c, c["name"])
    _same(got, want, c["name"], KEYS)
    if got["status"][0] != 0:
        assert np.array_equal(_bits(got["C"]), _bits(ops["C_in"])), "C = C_in bit for bit unless a step was accepted"
    assert np.array_equal(_bits(got["C"][:, 0]), _bits(ops["C_in"][:, 0])), "the anchor is returned bit for bit"


def test_several_graphs_in_one_launch_are_independent(T):
    """Three different graphs of twelve nodes - one of them with a slot list of its own length, one not attempted - in one launch:
    every graph's outputs are what it gives alone."""
    a = lc.with_loops(12, (1, 2), 23, [(0, 11), (2, 9)])
    b = lc.with_loops(12, (1, 3, 5), 26, [(1, 10)], outliers=0.1)
    bad = lc.with_loops(12, (1,), 27, [(0, 11)])
    bad["C_in"] = bad["C_in"].copy()
    bad["C_in"][5, 2] = np.inf
    d = lc.with_loops(12, (1, 2, 4), 28, [(0, 9), (3, 11), (0, 11)])
    cases = [a, b, bad, d]
    ops = lc.stacked(cases)
    want = _want(ops, a)
    assert list(want["status"]) == [0, 0, 3, 0]
    got = run_sparse(T, ops, a, "four graphs")
    _same(got, want, "four graphs", KEYS)
    for k, c in enumerate(cases):
        alone = run_sparse(T, _one(c), a, f"graph {k} alone")
        e = len(c["first"])
        for key in KEYS:
            g, w = (got[key][k][:e], alone[key][0]) if key == "edge_chi2" else (got[key][k], alone[key][0])
            assert np.array_equal(_bits(g), _bits(w)), (k, key)


# ------------------------------------------------------------------------------------------------- beside the banded solver
def _driver_cases():
    """(name, band, cases stacked into one launch): the shapes at which the driver both solvers share can go wrong."""
    import pose_graph_cases as pc
    small = pc._with_edges(pc.graph_case("small", 5, (1, 2), 2, 31), "small", first=(1, -1), second=(5, 1))      # absent; a = b = 1
    assert len(small["first"]) == 7
    big = pc.graph_case("chunks", 40, (1, 2, 3) * 3, 3, 32)          # three measurements of every edge up to the band
    big = {k: (v[:300] if k in ("first", "second", "T", "info") else v) for k, v in big.items()}
    big["T"][100, 5] = np.nan
    big["info"][280, 20] = np.inf
    bad = pc.graph_case("nan_in_C_in", 6, (1, 2), 2, 33)
    bad["C_in"][3, 7] = np.nan
    return [("small", 2, [small]), ("chunks", 3, [big]), ("nan_in_C_in", 2, [bad]), ("two_graphs", 2, [pc.graph_case("chain", 5, (1,), 2, 34), small])]


def run_banded(T, ops, band, c):
    from sslam_amd import lib
    n0 = lib.graph_launch_count()
    out = lib.pose_graph(*(T.from_numpy(ops[k]).cuda() for k in NAMES), band, c["chi"], c["damping"], c["n_iter"])
    T.cuda.synchronize()
    assert lib.graph_launch_count() - n0 == 1
    return {k: t.cpu().numpy() for k, t in zip(KEYS[:-1], out)}


def test_both_solvers_share_the_driver_bit_for_bit(T):
    """The same operands to sslg_pose_graph (a band that admits every listed edge) and to ssll_pose_graph_sparse.  Without a step
    every output is the driver's alone and the two are equal byte for byte; with three steps the counts and cost_in still are.
    Each is also held against its own restatement, and a graph of a two-graph launch against its launch alone."""
    import pose_graph_cases as pc
    import pose_graph_ref as pg
    for name, band, cases in _driver_cases():
        ops = pc.stacked_graphs(cases)
        used = [pg.used_mask(c["first"], c["second"], c["T"], c["info"], len(c["C_in"]), band) for c in cases]
        if name == "chunks":
            assert ops["first"].shape == (1, 300) and used[0][255] and used[0][256] and not used[0][100] and not used[0][280]
            assert (ops["second"] - ops["first"])[0][used[0]].max() == band
        for n_iter in (0, 3):
            c = dict(chi=4.0, damping=0.0, n_iter=n_iter, cg_iterations=512, cg_tol=1e-3)
            what = f"{name}, {n_iter} iterations"
            banded, sparse = run_banded(T, ops, band, c), run_sparse(T, ops, c, what)
            _same(banded, pg.optimize_graphs(ops["first"], ops["second"], ops["T"], ops["info"], ops["C_in"], band, 4.0, 0.0, n_iter), what, KEYS[:-1])
            _same(sparse, _want(ops, c), what, KEYS)
            _same(sparse, banded, what + ": the sparse entry beside the banded one",
                  KEYS[:-1] if n_iter == 0 else ("used_edges", "skipped_edges", "cost_in"))
            for k, u in enumerate(used):
                assert banded["used_edges"][k] == u.sum() and banded["skipped_edges"][k] == ((cases[k]["first"] != -1) & ~u).sum(), (what, k)
            if name == "nan_in_C_in":
                assert sparse["status"][0] == 3 and not sparse["cg_steps"].any() and not _bits(sparse["edge_chi2"]).any() and not sparse["cost"].any()
            if len(cases) > 1:
                for k, case in enumerate(cases):
                    e = len(case["first"])
                    for got, alone in ((banded, run_banded(T, _one(case), band, c)), (sparse, run_sparse(T, _one(case), c, what + f" graph {k} alone"))):
                        for key in alone:
                            g = got[key][k][:e] if key == "edge_chi2" else got[key][k]
                            assert np.array_equal(_bits(g), _bits(alone[key][0])), (what, k, key)


# ------------------------------------------------------------------------------------------------------- alignment and replay
@pytest.mark.parametrize("mode", ["lo", "hi"])
def test_every_pointer_at_its_least_alignment(T, mode):
    """Each operand at the alignment include/sslam_loop.h states and no better, just past and just before a 256-byte boundary:
    the same bits as the restatement."""
    def placed(entry, fn):
        with guarded.placed(guarded.Placement(lt.ALIGN[entry], mode)) as p:
            got = fn()
        assert sorted(r["name"] for r in p.made) == sorted(lt.ALIGN[entry]), entry
        for r in p.made:
            a = r["align"]
            assert r["middle"].data_ptr() % 256 == (a if mode == "lo" else 256 - a), (entry, r["name"])
        return got
    desc, scores = lc.bank(5, 65, 256, 12)
    got = placed("ssll_frame_signatures", lambda: run_signatures(T, desc, scores, f"signatures {mode}"))
    _same(dict(sig=got), dict(sig=ref.signatures(desc, scores)), f"signatures {mode}", ("sig",))
    c = lc.candidate_size_cases()[3]
    got = placed("ssll_loop_candidates", lambda: run_candidates(T, c, f"candidates {mode}"))
    _same(got, ref.candidates(c["sig"], c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"]), f"candidates {mode}", ref.CANDIDATE_KEYS)
    c = SPARSE[-1]
    ops = _one(c)
    got = placed("ssll_pose_graph_sparse", lambda: run_sparse(T, ops, c, f"sparse {mode}"))
    _same(got, _want(ops, c), f"sparse {mode}", KEYS)


def test_the_same_call_twice_and_a_captured_graph_give_the_same_bits(T):
    from sslam_amd import lib
    desc, scores = lc.bank(40, 64, 128, 13)
    dd, ds = T.from_numpy(desc).cuda(), T.from_numpy(scores).cuda()
    c = lc.with_loops(40, (1, 5, 10), 29, [(a, a + 33) for a in range(6)], outliers=0.03)
    ops = {k: T.from_numpy(v).cuda() for k, v in _one(c).items()}
    args = (ops["first"], ops["second"], ops["T"], ops["info"], ops["C_in"], c["chi"], c["damping"], c["n_iter"], c["cg_iterations"], c["cg_tol"])
    eager = [t.clone() for t in lib.pose_graph_sparse(*args)]
    again = lib.pose_graph_sparse(*args)
    T.cuda.synchronize()
    for k, a, b in zip(KEYS, eager, again):
        assert T.equal(_raw(T, a), _raw(T, b)), k
    shapes = lib.pose_graph_sparse_shapes(1, 40, len(c["first"]))
    out = tuple(T.zeros(shapes[k][0], dtype=shapes[k][1], device="cuda") for k in KEYS)
    ws = T.empty(lib.pose_graph_sparse_workspace_bytes(1, 40, len(c["first"])), dtype=T.uint8, device="cuda")
    sig, sws = T.zeros((40, 128), device="cuda"), T.empty(4 * 40 * 128, dtype=T.uint8, device="cuda")
    cshapes = lib.loop_candidate_shapes(40, 2)
    cand = tuple(T.zeros(cshapes[k][0], dtype=cshapes[k][1], device="cuda") for k in ref.CANDIDATE_KEYS)

    def work():
        lib.frame_signatures(dd, ds, out=sig, workspace=sws)
        lib.loop_candidates(sig, 10, 0.0, 2, 3, out=cand)
        lib.pose_graph_sparse(*args, out=out, workspace=ws)
    stream = T.cuda.Stream()
    stream.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(stream):
        work()
    T.cuda.current_stream().wait_stream(stream)
    T.cuda.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):
        work()
    want = _want(_one(c), c)
    want_sig = ref.signatures(desc, scores)
    want_cand = ref.candidates(want_sig, 10, 0.0, 2, 3)
    for _ in range(2):
        for t in out + cand + (sig,):
            t.zero_()
        g.replay()
        T.cuda.synchronize()
        _same({k: t.cpu().numpy() for k, t in zip(KEYS, out)}, want, "replay", KEYS)
        _same(dict(sig=sig.cpu().numpy()), dict(sig=want_sig), "replay", ("sig",))
        _same({k: t.cpu().numpy() for k, t in zip(ref.CANDIDATE_KEYS, cand)}, want_cand, "replay", ref.CANDIDATE_KEYS)
    _same({k: t.cpu().numpy() for k, t in zip(KEYS, eager)}, want, "eager", KEYS)


# ---------------------------------------------------------------------------------------------------------- through the layers
E2E_THRESHOLD = 12.0        # px: the selector's keypoints sit on the 16-px patch grid (tests/test_gpu_pose_refine.py's choice)
E2E_HYP, E2E_SEED, E2E_HUBER, E2E_ITER = 64, 5, 4.0, 5
E2E_LOOPS = dict(min_gap=4, min_sim=-1.0, per_frame=2, suppress=1, min_inliers=8)      # 12 frames: every frame past the gap proposes


@pytest.fixture(scope="module")
def seq(T):
    import pose_depth_cases
    import pose_eval_ref as pr
    from sslam_amd import evaluation as ev
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K), inp["selector"], inp["refiner"], device="cuda")
    toks = T.from_numpy(inp["tokens"]).cuda()
    return dict(pipe=pipe, toks=toks, poses=inp["poses"], depth=pose_depth_cases.sequence_depth(), cam=ev.Camera(),
                rule=MatchRule.mnn_ratio(0.9), k=pr.SEQ_K)


def _same_value(a, b, what):
    if isinstance(a, dict):
        assert list(a) == list(b), what
        for key in a:
            _same_value(a[key], b[key], (what, key))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    else:
        assert repr(a) == repr(b), what


def _restated_loop_graph(got, C_start, gone=None):
    """The restatement on the device's own edges: every spacing's refined poses, then the candidate slots that were kept."""
    import pose_graph_ref as pg
    sps = [k for k in got if isinstance(k, int)]
    iu = np.triu_indices(6)
    lp = got["loops"]
    Tm = np.concatenate([got[sp]["T"][:, :3].reshape(-1, 12) for sp in sps] + [lp["T"][:, :3].reshape(-1, 12)])
    info = np.concatenate([got[sp]["refine"]["info"][:, iu[0], iu[1]] for sp in sps] + [lp["info"][:, iu[0], iu[1]]])
    status = np.concatenate([got[sp]["refine"]["status"] for sp in sps] + [lp["status"]])
    pairs = [pr for sp in sps for pr in got[sp]["pairs"]]
    first = np.concatenate([[a for a, _ in pairs], np.where(lp["kept"], lp["first"], -1)])
    first = np.where(status == 3, -1, first).astype(np.int32)
    if gone is not None:
        first = np.where(gone, -1, first).astype(np.int32)
    second = np.concatenate([[b for _, b in pairs], lp["second"]]).astype(np.int32)
    want = ref.optimize(first, second, Tm, info, C_start, 4.0, 0.0, 8, 512, 1e-3)
    return want, pg.trajectory(want["C"]), pairs + list(zip(lp["first"].tolist(), lp["second"].tolist()))


def _assert_loop_graph(g, want, trajectory, pairs, poses):
    from sslam_amd import odometry as od
    assert list(g) == ["trajectory", "pairs", "status", "iterations", "used_edges", "skipped_edges", "failed_row", "cost_in", "cost", "edge_chi2",
                       "ate", "cg_steps"]
    assert g["trajectory"].tobytes() == trajectory.tobytes() and g["pairs"] == pairs
    for key in ("status", "iterations", "used_edges", "skipped_edges", "failed_row"):
        assert g[key] == want[key], key
    assert np.float64(g["cost_in"]).tobytes() == np.float64(want["cost_in"]).tobytes() and np.float64(g["cost"]).tobytes() == np.float64(want["cost"]).tobytes()
    assert g["edge_chi2"].tobytes() == want["edge_chi2"].tobytes() and g["cg_steps"].tolist() == want["cg_steps"].tolist()
    _same_value(g["ate"], od.ate_summary(g["trajectory"], poses), "ate")


def test_odometry_loop_graph_equals_the_restatement_fed_the_device_edges(T, seq):
    """The planted 12-frame sequence of synthetic tokens: every spacing and 'graph' what odometry_graph returns, byte for byte; the
    candidate lists what the restatement makes of the device's descriptors; the loop graph what the restatement makes of the
    device's refined poses, information matrices and kept mask, from the banded restatement's poses - also after pruning, and from
    a streamed result."""
    import pose_graph_ref as pg
    from sslam_amd import lib
    from sslam_amd import odometry as od
    from sslam_amd.harness import StreamingSequence
    s = seq
    pipe = s["pipe"]
    kw = dict(camera=s["cam"], poses=s["poses"], threshold=E2E_THRESHOLD, hypotheses=E2E_HYP, seed=E2E_SEED, huber=E2E_HUBER, iterations=E2E_ITER)
    base = od.odometry_graph(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], **kw)
    n0, g0 = lib.loop_launch_count(), lib.graph_launch_count()
    got = od.odometry_loop_graph(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], loops=E2E_LOOPS, **kw)
    assert lib.loop_launch_count() - n0 == 4 and lib.graph_launch_count() - g0 == 2, "signatures (2), candidates, the sparse graph; the chain and the banded graph"
    assert list(got) == [1, 5, 10, "graph", "loops", "loop_graph"]
    for key in (1, 5, 10, "graph"):
        _same_value(got[key], base[key], key)
    # the candidates: the restatement on the device's descriptors
    ex = pipe.extract(s["toks"], None)
    cand = ref.candidates(ref.signatures(ex["descriptors"].cpu().numpy(), ex["scores"].cpu().numpy()), E2E_LOOPS["min_gap"], E2E_LOOPS["min_sim"],
                          E2E_LOOPS["per_frame"], E2E_LOOPS["suppress"])
    lp = got["loops"]
    assert list(lp) == ["first", "second", "sim", "count", "kept", "match_count", "T", "status", "inlier_count", "info"]
    for key in ref.CANDIDATE_KEYS:
        assert lp[key].dtype == cand[key].dtype and lp[key].tobytes() == cand[key].tobytes(), key
    assert lp["count"].sum() >= 12 - 4 and (lp["count"][:4] == 0).all() and (lp["first"][lp["first"] >= 0] <= lp["second"][lp["first"] >= 0] - 4).all()
    assert np.array_equal(lp["kept"], (lp["first"] >= 0) & (lp["status"] != 3) & (lp["inlier_count"] >= E2E_LOOPS["min_inliers"]))
    assert lp["kept"].any(), "the sequence revisits its windows: some candidate is verified"
    # the loop graph: the restatement from the banded restatement's poses
    pairs = [pr for sp in (1, 5, 10) for pr in got[sp]["pairs"]]
    iu = np.triu_indices(6)
    Tm = np.concatenate([got[sp]["T"][:, :3].reshape(-1, 12) for sp in (1, 5, 10)])
    info = np.concatenate([got[sp]["refine"]["info"][:, iu[0], iu[1]] for sp in (1, 5, 10)])
    status = np.concatenate([got[sp]["refine"]["status"] for sp in (1, 5, 10)])
    first = np.where(status == 3, -1, [a for a, _ in pairs]).astype(np.int32)
    banded = pg.optimize(first, np.array([b for _, b in pairs], np.int32), Tm, info, pg.chain(Tm[:11], np.linalg.inv(s["poses"][0])[:3].reshape(12)),
                         10, 4.0, 0.0, 8)
    want, trajectory, all_pairs = _restated_loop_graph(got, banded["C"])
    _assert_loop_graph(got["loop_graph"], want, trajectory, all_pairs, s["poses"])
    assert want["used_edges"] == base["graph"]["used_edges"] + int(lp["kept"].sum()) and want["status"] in (0, 1)
    print(f"loop graph: {int(lp['count'].sum())} candidates, {int(lp['kept'].sum())} kept; status {want['status']}, {want['iterations']} steps, CG "
          f"{want['cg_steps'][:9].tolist()}, cost {want['cost_in']:.4g} -> {want['cost']:.4g}; ate rmse graph {base['graph']['ate']['rmse']:.4g}, "
          f"loop graph {got['loop_graph']['ate']['rmse']:.4g} (synthetic frames: no accuracy claim)")
    # pruning: a second launch on the reduced list, from the same poses
    prune_chi = float(np.sqrt(np.median(want["edge_chi2"][want["edge_chi2"] > 0])))
    n0 = lib.loop_launch_count()
    pruned = od.odometry_loop_graph(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], loops=E2E_LOOPS, prune_chi=prune_chi, **kw)
    assert lib.loop_launch_count() - n0 == 5 and list(pruned) == [1, 5, 10, "graph", "loops", "loop_graph_unpruned", "loop_graph"]
    _same_value(pruned["loop_graph_unpruned"], got["loop_graph"], "unpruned")
    _same_value(pruned["loops"], got["loops"], "loops")
    gone = want["edge_chi2"] > prune_chi * prune_chi
    assert 0 < gone.sum() < (want["edge_chi2"] > 0).sum()
    want2, trajectory2, _ = _restated_loop_graph(got, banded["C"], gone)
    _assert_loop_graph(pruned["loop_graph"], want2, trajectory2, all_pairs, s["poses"])
    assert want2["used_edges"] == want["used_edges"] - int(gone.sum())
    # the same from a streamed result
    result = StreamingSequence(pipe, (1, 5, 10), rule=s["rule"]).run(s["toks"])
    _same_value(od.odometry_result_loop_graph(pipe, result, depth=T.from_numpy(s["depth"]).cuda(), loops=E2E_LOOPS, rule=s["rule"], **kw), got,
                "odometry_result_loop_graph")
    _same_value(od.odometry_graph(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], **kw), base, "afterwards")


def test_run_directory_adds_the_loop_keys_and_only_when_asked(T, tmp_path):
    import synth
    from sslam_amd import evaluation as ev
    from sslam_amd import odometry as od
    from sslam_amd.harness import run_directory
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    from sslam_amd.tum import TUMSequence
    name, g, k = "rgbd_dataset_freiburg1_desk", 5, 12
    synth.write_tum_sequence(str(tmp_path / name))
    tum = TUMSequence(str(tmp_path), name)
    depth = tum.load_depth_raw(range(len(tum)))
    cam = ev.Camera(fx=517.3 / 20, fy=516.5 / 20, cx=318.6 / 20, cy=255.3 / 20, width=32, height=24)      # the fixture's frames are 32 x 24
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    toks = T.from_numpy(synth.token_sequence(len(tum), g)).cuda()
    kw = dict(pipe=pipe, tokens_fn=lambda a, b: toks[a:b], chunk=4, decode_workers=2)
    base = dict(num_pairs=4, threshold=20.0, depth=True, camera=cam, odometry=True, refine=True, graph=True)
    loops = dict(min_gap=2, min_sim=-1.0, per_frame=1, suppress=0, min_inliers=3)
    old = run_directory(str(tmp_path), name, (1, 3), evaluate=base, **kw)
    got = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(base, loops=dict(loops, cg_iterations=64)), **kw)
    assert list(got["odometry"]) == [1, 3, "graph", "loops", "loop_graph"] and list(old["odometry"]) == [1, 3, "graph"]
    for key in (1, 3, "graph"):
        _same_value(got["odometry"][key], old["odometry"][key], key)
    direct = od.odometry_result_loop_graph(pipe, got, depth=depth, camera=cam, poses=tum.poses, spacings=(1, 3), num_pairs=4, threshold=20.0, loops=loops,
                                           cg_iterations=64)
    for key in ("loops", "loop_graph"):
        _same_value(got["odometry"][key], direct[key], key)
    assert got["odometry"]["loop_graph"]["trajectory"].shape == (5, 4, 4) and got["odometry"]["loops"]["count"].tolist() == [0, 0, 1, 1, 1]


def test_the_numpy_drop_ins_equal_the_restatement(T):
    import evaluation as dropin
    c = lc.with_loops(12, (1, 2), 23, [(0, 11), (2, 9)])
    iu = np.triu_indices(6)
    H = np.zeros((len(c["first"]), 6, 6))
    H[:, iu[0], iu[1]] = c["info"]
    H[:, iu[1], iu[0]] = c["info"]
    T44 = np.tile(np.eye(4), (len(c["first"]), 1, 1))
    T44[:, :3] = c["T"].reshape(-1, 3, 4)
    C, status, chi2, cg = dropin.optimize_pose_graph_sparse(c["first"], c["second"], T44, H, 12, c["C_in"].reshape(12, 3, 4), cg_iterations=100, cg_tol=1e-6)
    want = ref.optimize(c["first"], c["second"], c["T"], c["info"], c["C_in"], 4.0, 0.0, 8, 100, 1e-6)
    assert C[:, :3].tobytes() == want["C"].reshape(-1, 3, 4).tobytes() and status == want["status"] and chi2.tobytes() == want["edge_chi2"].tobytes()
    assert cg.tolist() == want["cg_steps"].tolist() and np.array_equal(C[:, 3], np.tile([0, 0, 0, 1.0], (12, 1)))
    desc, scores = lc.bank(30, 20, 128, 14)
    pairs, sim = dropin.find_loop_candidates(desc, scores, min_gap=10, min_sim=-1.0, per_frame=2, suppress=2)
    w = ref.candidates(ref.signatures(desc, scores), 10, -1.0, 2, 2)
    filled = w["first"] >= 0
    assert pairs.tobytes() == np.stack([w["first"][filled], w["second"][filled]], axis=1).tobytes() and sim.tobytes() == w["sim"][filled].tobytes()
    assert len(pairs) == int(w["count"].sum()) >= 20 and (pairs[:, 1] - pairs[:, 0] >= 10).all()
