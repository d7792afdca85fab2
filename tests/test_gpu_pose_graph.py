"""libsslam_graph.so on the device against its float64 restatement (tests/pose_graph_ref.py), bit for bit and for every output:
the smallest shapes at which the band indexing can go wrong, the contract's rows, several graphs in one launch, the chain, every
pointer at its least alignment, outputs and workspace in poisoned guarded buffers (tests/guarded.py), repeatability, a captured
graph - and odometry_graph on a planted sequence against the restatement fed the same device-produced edges."""
import numpy as np
import pytest

import graph_table as gt
import guarded
import pose_graph_cases as pc
import pose_graph_ref as ref

pytestmark = pytest.mark.gpu
KEYS = ref.KEYS


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what, keys=KEYS):
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


def _check_guards(T, pairs, what):
    for name, (whole, mid) in pairs:
        guarded.assert_guards(whole, _raw(T, mid), f"{what} {name}")


OUT_NAMES = dict(zip(KEYS, ("C", "status", "iterations", "used_edges", "skipped_edges", "failed_row", "cost_in", "cost", "edge_chi2")))


def run(T, ops, band, chi, damping, n_iter, what):
    """One guarded launch of sslg_pose_graph on stacked operands (graph axis first) -> dict of numpy arrays."""
    from sslam_amd import lib
    n_graphs, n_nodes, n_edges = ops["C_in"].shape[0], ops["C_in"].shape[1], ops["first"].shape[1]
    names = dict(first="edge_first", second="edge_second", T="edge_T", info="edge_info", C_in="C_in")
    ins = {k: _in(T, ops[k], names[k]) for k in names}
    shapes = lib.pose_graph_shapes(n_graphs, n_nodes, n_edges)
    outs = {k: _out(T, shapes[k][0], shapes[k][1], OUT_NAMES[k]) for k in KEYS}
    ws = guarded.guarded(T, lib.pose_graph_workspace_bytes(n_graphs, n_nodes, band), T.uint8, name="workspace")
    n0, m0, x0 = lib.graph_launch_count(), lib.launch_count(), lib.ext_launch_count()
    back = lib.pose_graph(ins["first"][1], ins["second"][1], ins["T"][1], ins["info"][1], ins["C_in"][1], band, chi, damping, n_iter,
                          out=tuple(outs[k][1] for k in KEYS), workspace=ws[1])
    T.cuda.synchronize()
    assert lib.graph_launch_count() - n0 == 1 and lib.launch_count() == m0 and lib.ext_launch_count() == x0, "one launch, of the third library"
    assert all(b is outs[k][1] for b, k in zip(back, KEYS))
    _check_guards(T, list(ins.items()) + list(outs.items()) + [("workspace", ws)], what)
    for k in KEYS:
        guarded.assert_written(_raw(T, outs[k][1]), f"{what} {k}")
    for k in names:
        assert np.array_equal(_bits(ins[k][1].cpu().numpy()), _bits(ops[k])), f"{what}: input {k} was written"
    return {k: outs[k][1].cpu().numpy() for k in KEYS}


def _one(case):
    return {k: np.ascontiguousarray(np.asarray(case[k])[None]) for k in ("first", "second", "T", "info", "C_in")}


def _want(ops, band, chi, damping, n_iter):
    return ref.optimize_graphs(ops["first"], ops["second"], ops["T"], ops["info"], ops["C_in"], band, chi, damping, n_iter)


SHAPES = pc.shape_cases()
CONTRACT = pc.contract_cases()


@pytest.mark.parametrize("index", range(len(SHAPES)), ids=[c["name"] for c in SHAPES])
def test_shapes_equal_the_restatement(T, index):
    c = SHAPES[index]
    ops = _one(c)
    want = _want(ops, c["band"], c["chi"], c["damping"], c["n_iter"])
    assert want["status"][0] == 0 and want["iterations"][0] >= 1, "the case takes steps"
    if c["name"] == "huber_branch":
        assert (want["edge_chi2"][0] > c["chi"] ** 2).any() and (want["edge_chi2"][0][want["edge_chi2"][0] > 0] <= c["chi"] ** 2).any()
    _same(run(T, ops, c["band"], c["chi"], c["damping"], c["n_iter"], c["name"]), want, c["name"])


@pytest.mark.parametrize("index", range(len(CONTRACT)), ids=[c["name"] for c in CONTRACT])
def test_contract_rows_equal_the_restatement(T, index):
    c = CONTRACT[index]
    ops = _one(c)
    want = _want(ops, c["band"], c["chi"], c["damping"], c["n_iter"])
    got = run(T, ops, c["band"], c["chi"], c["damping"], c["n_iter"], c["name"])
    _same(got, want, c["name"])
    if got["status"][0] != 0:
        assert np.array_equal(_bits(got["C"]), _bits(ops["C_in"])), "C = C_in bit for bit unless a step was accepted"
    assert np.array_equal(_bits(got["C"][:, 0]), _bits(ops["C_in"][:, 0])), "the anchor is returned bit for bit"


def _by_name(name):
    return next(c for c in CONTRACT if c["name"] == name)


def test_several_graphs_in_one_launch_are_independent(T):
    """Two good graphs around a status-2 and a status-3 one, and three different good ones: every graph's outputs are what it
    gives alone."""
    base = pc.graph_case("base", 7, (1, 2, 3), 3, 11)
    four = [base, _by_name("disconnected_node"), _by_name("nan_in_C_in"), _by_name("duplicate_edges")]
    three = [pc.graph_case(f"g{seed}", 7, (1, 2, 3), 3, seed) for seed in (21, 22, 23)]
    for cases, statuses in ((four, [0, 2, 3, 0]), (three, [0, 0, 0])):
        ops = pc.stacked_graphs(cases)
        want = _want(ops, 3, 4.0, 0.0, 8)
        assert list(want["status"]) == statuses
        got = run(T, ops, 3, 4.0, 0.0, 8, f"{len(cases)} graphs")
        _same(got, want, f"{len(cases)} graphs")
        for k, c in enumerate(cases):                          # alone: the same bits (padding slots apart)
            alone = pc.run(c)
            assert np.array_equal(_bits(got["C"][k]), _bits(alone["C"])) and got["status"][k] == alone["status"]


def _chain(T, Tm, start, what):
    from sslam_amd import lib
    n_graphs, n_nodes = Tm.shape[0], Tm.shape[1] + 1
    wt, dt = _in(T, Tm, "T") if n_nodes > 1 else (None, T.zeros((n_graphs, 0, 12), dtype=T.float64, device="cuda"))
    ws_, ds = _in(T, start, "C_start") if start is not None else (None, None)
    wo, do = _out(T, (n_graphs, n_nodes, 12), T.float64, "C")
    n0 = lib.graph_launch_count()
    back = lib.chain_poses(dt, start=ds, out=do)
    T.cuda.synchronize()
    assert back is do and lib.graph_launch_count() - n0 == 1
    guarded.assert_guards(wo, do.view(T.int64), f"{what} C")
    guarded.assert_written(do.view(T.int64), f"{what} C")
    if wt is not None:
        guarded.assert_guards(wt, dt.view(T.int64), f"{what} T")
    return do.cpu().numpy()


@pytest.mark.parametrize("n_nodes", [1, 2, 40])
@pytest.mark.parametrize("with_start", [False, True])
def test_chain_equals_the_restatement(T, n_nodes, with_start):
    p = [pc.planted(max(n_nodes, 2), (1,), seed) for seed in (31, 32, 33)]
    Tm = np.stack([q["T"][:n_nodes - 1] for q in p])
    start = np.stack([q["truth"][-1] for q in p]) if with_start else None
    got = _chain(T, Tm, start, f"chain {n_nodes}")
    want = np.stack([ref.chain(Tm[k], None if start is None else start[k]) for k in range(3)])
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("mode", ["lo", "hi"])
def test_every_pointer_at_its_least_alignment(T, mode):
    """Each operand at the alignment include/sslam_graph.h states and no better, just past and just before a 256-byte boundary:
    the same bits as the restatement."""
    c = SHAPES[4]
    ops = _one(c)
    with guarded.placed(guarded.Placement(gt.ALIGN["sslg_pose_graph"], mode)) as p:
        got = run(T, ops, c["band"], c["chi"], c["damping"], c["n_iter"], f"pose_graph {mode}")
    assert sorted(r["name"] for r in p.made) == sorted(gt.ALIGN["sslg_pose_graph"])
    for r in p.made:
        a = r["align"]
        assert r["middle"].data_ptr() % 256 == (a if mode == "lo" else 256 - a), r["name"]
    _same(got, _want(ops, c["band"], c["chi"], c["damping"], c["n_iter"]), f"pose_graph {mode}")
    q = pc.planted(9, (1,), 41)
    with guarded.placed(guarded.Placement(gt.ALIGN["sslg_chain_poses"], mode)) as p:
        got = _chain(T, q["T"][None], q["truth"][-1][None], f"chain {mode}")
    assert sorted(r["name"] for r in p.made) == sorted(gt.ALIGN["sslg_chain_poses"])
    assert np.array_equal(_bits(got[0]), _bits(ref.chain(q["T"], q["truth"][-1])))


def test_the_same_call_twice_and_a_captured_graph_give_the_same_bits(T):
    from sslam_amd import lib
    c = SHAPES[5]                                             # forty nodes, five spacings
    ops = {k: T.from_numpy(v).cuda() for k, v in _one(c).items()}
    args = (ops["first"], ops["second"], ops["T"], ops["info"], ops["C_in"], c["band"], c["chi"], c["damping"], c["n_iter"])
    eager = [t.clone() for t in lib.pose_graph(*args)]
    again = lib.pose_graph(*args)
    T.cuda.synchronize()
    for k, a, b in zip(KEYS, eager, again):
        assert T.equal(_raw(T, a), _raw(T, b)), k
    shapes = lib.pose_graph_shapes(1, c["C_in"].shape[0], len(c["first"]))
    out = tuple(T.zeros(shapes[k][0], dtype=shapes[k][1], device="cuda") for k in KEYS)
    ws = T.empty(lib.pose_graph_workspace_bytes(1, c["C_in"].shape[0], c["band"]), dtype=T.uint8, device="cuda")
    chained = T.zeros((1, c["C_in"].shape[0], 12), dtype=T.float64, device="cuda")
    Tm = T.from_numpy(np.ascontiguousarray(c["T"][None, :c["C_in"].shape[0] - 1])).cuda()
    stream = T.cuda.Stream()
    stream.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(stream):
        lib.chain_poses(Tm, out=chained)
        lib.pose_graph(*args[:4], chained, *args[5:], out=out, workspace=ws)
    T.cuda.current_stream().wait_stream(stream)
    T.cuda.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):
        lib.chain_poses(Tm, out=chained)
        lib.pose_graph(*args[:4], chained, *args[5:], out=out, workspace=ws)
    want = _want(_one(c), c["band"], c["chi"], c["damping"], c["n_iter"])
    for _ in range(2):
        for t in out:
            t.zero_()
        chained.zero_()
        g.replay()
        T.cuda.synchronize()
        _same({k: t.cpu().numpy() for k, t in zip(KEYS, out)}, want, "replay")
        assert np.array_equal(_bits(chained.cpu().numpy()[0]), _bits(c["C_in"])), "the case's initial guess is the chain of its spacing-1 edges"
    _same({k: t.cpu().numpy() for k, t in zip(KEYS, eager)}, want, "eager")


# ---------------------------------------------------------------------------------------------------------- through the layers
E2E_THRESHOLD = 12.0        # px: the selector's keypoints sit on the 16-px patch grid (tests/test_gpu_pose_refine.py's choice)
E2E_HYP, E2E_SEED, E2E_HUBER, E2E_ITER = 64, 5, 4.0, 5


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


def test_odometry_graph_equals_the_restatement_fed_the_device_edges(T, seq):
    """The planted 12-frame sequence of synthetic tokens: per spacing what odometry(refine=True) returns, byte for byte; the graph
    what the restatement makes of the same refined poses and information matrices."""
    from sslam_amd import lib
    from sslam_amd import odometry as od
    from sslam_amd.harness import StreamingSequence
    s = seq
    pipe = s["pipe"]
    kw = dict(camera=s["cam"], poses=s["poses"], threshold=E2E_THRESHOLD, hypotheses=E2E_HYP, seed=E2E_SEED, huber=E2E_HUBER, iterations=E2E_ITER)
    before = {sp: od.odometry(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], spacing=sp, refine=True, **kw) for sp in (1, 5, 10)}
    n0 = lib.graph_launch_count()
    got = od.odometry_graph(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], **kw)
    assert lib.graph_launch_count() - n0 == 2, "the chain and the graph"
    assert list(got) == [1, 5, 10, "graph"], "12 frames hold no pair at spacing 15 or 20"
    for sp in (1, 5, 10):
        _same_value(got[sp], before[sp], f"spacing {sp}")
        _same_value(od.odometry(pipe, tokens=s["toks"], depth=s["depth"], rule=s["rule"], spacing=sp, refine=True, **kw), before[sp], "afterwards")
    g = got["graph"]
    assert list(g) == ["trajectory", "pairs", "status", "iterations", "used_edges", "skipped_edges", "failed_row", "cost_in", "cost", "edge_chi2",
                       "ate", "ate_chain"]
    pairs = [pr for sp in (1, 5, 10) for pr in got[sp]["pairs"]]
    assert g["pairs"] == pairs and len(pairs) == 11 + 7 + 2
    Tm = np.concatenate([got[sp]["T"][:, :3].reshape(-1, 12) for sp in (1, 5, 10)])
    iu = np.triu_indices(6)
    info = np.concatenate([got[sp]["refine"]["info"][:, iu[0], iu[1]] for sp in (1, 5, 10)])
    status = np.concatenate([got[sp]["refine"]["status"] for sp in (1, 5, 10)])
    first = np.where(status == 3, -1, [a for a, _ in pairs]).astype(np.int32)
    second = np.array([b for _, b in pairs], np.int32)
    C_in = ref.chain(Tm[:11], np.linalg.inv(s["poses"][0])[:3].reshape(12))
    want = ref.optimize(first, second, Tm, info, C_in, 10, 4.0, 0.0, 8)
    assert g["trajectory"].tobytes() == ref.trajectory(want["C"]).tobytes(), "the trajectory is the inverse of the restatement's poses"
    for key in ("status", "iterations", "used_edges", "skipped_edges", "failed_row"):
        assert g[key] == want[key], key
    assert np.float64(g["cost_in"]).tobytes() == np.float64(want["cost_in"]).tobytes() and np.float64(g["cost"]).tobytes() == np.float64(want["cost"]).tobytes()
    assert g["edge_chi2"].tobytes() == want["edge_chi2"].tobytes()
    assert g["used_edges"] == int((status != 3).sum()) and g["used_edges"] >= 11
    _same_value(g["ate"], od.ate_summary(g["trajectory"], s["poses"]), "ate")
    _same_value(g["ate_chain"], before[1]["ate"], "ate_chain")
    print(f"graph: status {g['status']}, {g['iterations']} steps, cost {g['cost_in']:.4g} -> {g['cost']:.4g}; ate rmse chain "
          f"{g['ate_chain']['rmse']:.4g}, graph {g['ate']['rmse']:.4g} (synthetic frames: no accuracy claim)")
    # the same from a streamed result
    result = StreamingSequence(pipe, (1, 5, 10), rule=s["rule"]).run(s["toks"])
    _same_value(od.odometry_result_graph(pipe, result, depth=T.from_numpy(s["depth"]).cuda(), **kw), got, "odometry_result_graph")
    with pytest.raises(ValueError):
        od.odometry_graph(pipe, tokens=s["toks"], depth=s["depth"], spacings=(5, 10), **kw)


def test_run_directory_adds_the_graph_and_only_when_asked(T, tmp_path):
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
    base = dict(num_pairs=4, threshold=20.0, depth=True, camera=cam, odometry=True, refine=True)
    old = run_directory(str(tmp_path), name, (1, 3), evaluate=base, **kw)
    got = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(base, graph=True), **kw)
    assert list(got["odometry"]) == [1, 3, "graph"] and list(old["odometry"]) == [1, 3]
    for sp in (1, 3):
        _same_value(got["odometry"][sp], old["odometry"][sp], f"spacing {sp}")
    direct = od.odometry_result_graph(pipe, got, depth=depth, camera=cam, poses=tum.poses, spacings=(1, 3), num_pairs=4, threshold=20.0)
    _same_value(got["odometry"]["graph"], direct["graph"], "graph")
    assert got["odometry"]["graph"]["trajectory"].shape == (5, 4, 4)


def test_the_numpy_drop_in_equals_the_restatement(T):
    import evaluation as dropin
    c = SHAPES[4]
    iu = np.triu_indices(6)
    H = np.zeros((len(c["first"]), 6, 6))
    H[:, iu[0], iu[1]] = c["info"]
    H[:, iu[1], iu[0]] = c["info"]
    T44 = np.tile(np.eye(4), (len(c["first"]), 1, 1))
    T44[:, :3] = c["T"].reshape(-1, 3, 4)
    C, status, chi2 = dropin.optimize_pose_graph(c["first"], c["second"], T44, H, len(c["C_in"]), band=c["band"], huber_chi=c["chi"])
    want = pc.run(c)                                           # the case's C_in is the chain of its spacing-1 edges
    assert C[:, :3].tobytes() == want["C"].reshape(-1, 3, 4).tobytes() and status == want["status"] and chi2.tobytes() == want["edge_chi2"].tobytes()
    assert np.array_equal(C[:, 3], np.tile([0, 0, 0, 1.0], (len(C), 1)))
