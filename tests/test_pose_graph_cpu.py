"""The pose graph without a GPU: the restatement (tests/pose_graph_ref.py) against an independent dense solve and independent
normal equations, the planted study DESIGN.md §4k records, the contract's rows, and the interface of libsslam_graph.so -
include/sslam_graph.h, sslam_amd.lib.GRAPH_EXPORTS and tests/graph_table.py hold the same entries; the built library's symbols are
tests/test_libraries_cpu.py - with every host-side check raising before the library is loaded and one past each size limit refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ext_table as et
import graph_table as gt
import loose_table as lt
import pose_graph_cases as pc
import pose_graph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sslam_graph.h")
CASES = pc.shape_cases() + pc.contract_cases()
BY = {c["name"]: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_every_step_solves_the_independent_dense_system():
    """At every step of every case the restatement's reduced A and g, dense, and its banded delta are held to
    |A delta + g|_inf <= 1e-9 (|A|_inf |delta|_inf + |g|_inf), and delta to np.linalg.solve.  The bound is derived, not measured: an
    unpivoted LDL^T of an SPD matrix is backward stable at about n 2^-53 with n <= 6 * 40, so 1e-9 is four orders loose - and still
    catches any band-indexing error.  A and g themselves are formed again the plain way (matrix products, np.linalg.inv, their own
    Jacobians) and equal the restatement's to 1e-12 of the largest entry: the difference is rounding alone."""
    steps = 0
    for c in CASES:
        r = pc.run(c, detail=True)
        for st in r["steps"]:
            cost, A, g = ref.plain_normal_equations(c["first"], c["second"], c["T"], c["info"], st["C"], c["band"], c["chi"], c["damping"])
            low = np.tril(st["A"])
            mine = low + np.tril(low, -1).T
            assert np.abs(mine - A).max() <= 1e-12 * np.abs(A).max() and np.abs(st["g"] - g).max() <= 1e-12 * max(np.abs(g).max(), np.abs(A).max()), c["name"]
            if st["delta"] is None:
                continue
            d = st["delta"]
            lhs = np.abs(mine @ d + st["g"]).max()
            bound = 1e-9 * (np.abs(mine).sum(axis=1).max() * np.abs(d).max() + np.abs(st["g"]).max())
            assert lhs <= bound, (c["name"], lhs, bound)
            assert np.abs(d - np.linalg.solve(mine, -st["g"])).max() <= 1e-6 * max(np.abs(d).max(), 1e-300), c["name"]
            steps += 1
    assert steps >= 60


def test_the_band_is_what_the_header_says():
    """An entry of A outside the band 6 * band + 5 never forms, and the factor fills nothing outside it."""
    c = BY["forty_nodes_five_spacings"]
    st = pc.run(c, detail=True)["steps"][0]
    i, j = np.indices(st["A"].shape)
    assert (np.tril(st["A"])[i - j > 6 * c["band"] + 5] == 0).all()
    assert (np.tril(st["A"])[i - j == 6 * c["band"] + 5] != 0).any(), "the band is reached"


def test_the_gradient_is_the_costs_derivative():
    """g against central differences of the plain cost through exp(xi) C, at residuals small enough for J_b = I (exact at r = 0,
    off by O(|r|) of the rotation residual, here below 0.02 rad): 5 % of |g|_inf."""
    c = pc.graph_case("small", 5, (1, 2), 2, 77, chi=1e9, sigma_t=0.002, sigma_r=0.001)
    cost0, A, g = ref.plain_normal_equations(c["first"], c["second"], c["T"], c["info"], c["C_in"], 2, 1e9, 0.0)
    fd, h = np.zeros(len(g)), 1e-6
    for k in range(len(g)):
        costs = []
        for sgn in (1.0, -1.0):
            Cp = c["C_in"].copy()
            xi = np.zeros(6)
            xi[k % 6] = sgn * h
            Cp[k // 6 + 1] = pc.perturb(Cp[k // 6 + 1], xi)
            costs.append(ref.plain_normal_equations(c["first"], c["second"], c["T"], c["info"], Cp, 2, 1e9, 0.0)[0])
        fd[k] = (costs[0] - costs[1]) / (4 * h)
    assert np.abs(fd - g).max() <= 0.05 * np.abs(g).max(), (np.abs(fd - g).max(), np.abs(g).max())


# ------------------------------------------------------------------------------------------------------------------ the study
def test_planted_study_the_graph_beats_the_chain_in_every_seed():
    """20 planted 120-frame trajectories, 549 edges at the five spacings, noise drawn from each edge's own covariance, 3 % gross
    outliers (tests/pose_graph_cases.py).  Position rmse after rigid alignment, measured with this restatement, median over the
    seeds: the spacing-1 chain 0.2654 m, the graph without the Huber weight (chi = 1e9) 0.0396 m, with it at chi = 4 0.0101 m;
    2 to 8 accepted steps.  Asserted: the graph's error is below the chain's in all 20 seeds, in both forms."""
    chain, plain, huber, steps = [], [], [], []
    for seed in range(20):
        p = pc.planted(120, seed=seed, outliers=0.03)
        chain.append(pc.ate_rmse(p["C_chain"], p["truth"]))
        for chi, into in ((1e9, plain), (4.0, huber)):
            r = ref.optimize(p["first"], p["second"], p["T"], p["info"], p["C_chain"], 20, chi, 0.0, 8)
            assert r["status"] == 0
            into.append(pc.ate_rmse(r["C"], p["truth"]))
            steps.append(r["iterations"])
    print(f"planted study, median ate rmse over 20 seeds: chain {np.median(chain):.4f} m, graph at chi 1e9 {np.median(plain):.4f} m, "
          f"graph at chi 4 {np.median(huber):.4f} m; accepted steps {min(steps)} to {max(steps)}")
    assert len(p["first"]) == 549
    assert all(h < c for h, c in zip(huber, chain)) and all(g < c for g, c in zip(plain, chain))


# --------------------------------------------------------------------------------------------------------------- the contract
def test_contract_rows():
    r = pc.run(BY["exact_edges"])
    assert r["status"] == 1 and r["cost_in"] == 0.0 and r["cost"] == 0.0 and r["iterations"] == 0
    assert r["C"].tobytes() == BY["exact_edges"]["C_in"].tobytes() and (r["edge_chi2"] == 0).all()
    r = pc.run(BY["no_iterations"])
    assert r["status"] == 1 and r["iterations"] == 0 and r["cost"] == r["cost_in"] > 0 and r["C"].tobytes() == BY["no_iterations"]["C_in"].tobytes()
    assert (r["edge_chi2"] > 0).all()
    base = pc.run(pc.graph_case("base", 7, (1, 2, 3), 3, 11))
    r = pc.run(BY["absent_slot"])
    assert (r["used_edges"], r["skipped_edges"]) == (base["used_edges"] - 1, 0) and r["edge_chi2"][4] == 0 and r["status"] == 0
    for name, slot in (("second_before_first", 7), ("equal_nodes", 8), ("node_out_of_range", 9), ("negative_node", 9), ("nan_in_T", 3),
                       ("inf_in_info", 10), ("nan_in_info", 2)):
        r = pc.run(BY[name])
        assert (r["used_edges"], r["skipped_edges"]) == (base["used_edges"] - 1, 1), name
        assert r["edge_chi2"][slot] == 0 and r["status"] == 0 and np.isfinite(r["C"]).all(), name
        # the skipped slot is as good as absent
        gone = dict(BY[name], first=BY[name]["first"].copy())
        gone["first"][slot] = -1
        assert pc.run(gone)["C"].tobytes() == r["C"].tobytes(), name
    r = pc.run(BY["past_the_band"])
    assert (r["used_edges"], r["skipped_edges"]) == (11, 4) and (r["edge_chi2"][11:] == 0).all()
    r = pc.run(BY["disconnected_node"])
    assert r["status"] == 2 and r["failed_row"] == 6 * (4 - 1) and r["failed_row"] // 6 + 1 == 4 and r["iterations"] == 0
    assert r["C"].tobytes() == BY["disconnected_node"]["C_in"].tobytes() and r["cost"] == r["cost_in"]
    r = pc.run(BY["disconnected_node_damped"])
    assert r["status"] == 0 and r["failed_row"] == -1 and (r["C"][4] == BY["disconnected_node"]["C_in"][4]).all()
    assert not (r["C"][3] == BY["disconnected_node"]["C_in"][3]).all()
    r = pc.run(BY["duplicate_edges"])
    assert r["used_edges"] == base["used_edges"] + 5 and (r["edge_chi2"][-5:] > 0).all() and r["C"].tobytes() != base["C"].tobytes()
    for name in ("nan_in_C_in", "no_used_edge"):
        r = pc.run(BY[name])
        assert r["status"] == 3 and r["cost_in"] == 0 and r["cost"] == 0 and (r["edge_chi2"] == 0).all() and r["failed_row"] == -1
        assert r["C"].tobytes() == BY[name]["C_in"].tobytes()
    assert pc.run(BY["nan_in_C_in"])["used_edges"] == base["used_edges"] and pc.run(BY["no_used_edge"])["used_edges"] == 0
    for c in CASES:                                            # everywhere: the anchor bit for bit, the cost never rises
        r = pc.run(c)
        assert r["C"][0].tobytes() == np.asarray(c["C_in"])[0].tobytes() and (r["status"] == 3 or r["cost"] <= r["cost_in"]), c["name"]
    r = pc.run(BY["huber_branch"])
    assert (r["edge_chi2"] > 1.0).any() and ((r["edge_chi2"] > 0) & (r["edge_chi2"] <= 1.0)).any(), "both branches of the weight"


def test_the_chain_is_the_product_of_its_transforms():
    p = pc.planted(9, (1,), 3)
    got = ref.chain(p["T"], p["truth"][2])
    want = [ref._m44(p["truth"][2])]
    for t in p["T"]:
        want.append(ref._m44(t) @ want[-1])
    assert np.abs(got.reshape(-1, 3, 4) - np.stack(want)[:, :3]).max() <= 1e-12 and got[0].tobytes() == p["truth"][2].tobytes()
    assert ref.chain(np.zeros((0, 12))).tolist() == [[1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]


# ---------------------------------------------------------------------------------------------------------------- the interface
def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_header_symbols_exports_and_table_agree():
    """The tables (this library's and, as when it arrived, the two before it), the constants and the key list against the export
    lists; those lists against the headers and the built libraries are tests/test_libraries_cpu.py."""
    from sslam_amd import lib
    declared = lib.GRAPH_EXPORTS
    assert set(gt.ALIGN) | set(gt.HOST_ONLY) == set(declared) and not set(gt.ALIGN) & set(gt.HOST_ONLY) and set(gt.LIMITS) == set(gt.ALIGN)
    assert set(lib.EXT_EXPORTS) == set(et.ALIGN) | set(et.HOST_ONLY)
    assert set(lib.EXPORTS) == set(lt.ALIGN) | set(lt.HOST_ONLY)
    consts = dict(re.findall(r"#define (SSLG_\w+) (\d+)", open(HEADER).read()))
    assert {k: int(v) for k, v in consts.items()} == dict(SSLG_MAX_BAND=gt.MAX_BAND, SSLG_MAX_NODES=gt.MAX_NODES, SSLG_MAX_EDGES=gt.MAX_EDGES,
                                                           SSLG_MAX_GRAPHS=gt.MAX_GRAPHS, SSLG_GRAPH_MAX_ITER=gt.MAX_ITER)
    assert (lib.GRAPH_MAX_BAND, lib.GRAPH_MAX_NODES, lib.GRAPH_MAX_EDGES, lib.GRAPH_MAX_GRAPHS, lib.GRAPH_MAX_ITER) == \
        (gt.MAX_BAND, gt.MAX_NODES, gt.MAX_EDGES, gt.MAX_GRAPHS, gt.MAX_ITER) == (ref.MAX_BAND, ref.MAX_NODES, ref.MAX_EDGES, ref.MAX_GRAPHS, ref.MAX_ITER)
    assert lib.POSE_GRAPH_KEYS == ref.KEYS


def test_the_header_states_both_tables_line_for_line():
    elem = {"int32_t": 4, "double": 8, "void": 8}
    text = _header()
    for entry, row in gt.ALIGN.items():
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*?)\)\s*;", text)
        assert m, entry
        args = [re.match(r"(.*?)(\w+)$", " ".join(a.split())).groups() for a in m.group(1).split(",")]
        pointers = [(t.strip(), n) for t, n in args if "*" in t and n != "stream"]
        assert [n for _, n in pointers] == list(row), entry
        for t, n in pointers:
            assert row[n] == elem[t.replace("const", "").replace("*", "").strip()], (entry, n)
    raw = open(HEADER).read()
    for title, lines, count in (("ALIGNMENT, every entry", gt.header_lines(), len(gt.ALIGN)), ("SIZE LIMITS: the expressions", gt.limit_lines(), len(gt.LIMITS))):
        start = raw.index(title)
        stated = re.sub(r"\n \*\s+", " ", raw[start:raw.index("*/", start)]).strip()          # the block's lines joined, the margin dropped
        for line in lines:
            assert line + " " in stated + " ", f"include/sslam_graph.h does not state: {line}"
        assert len(re.findall(r"\bsslg_\w+: ", stated)) == count
    for text_ in ("k ascending from max(0, i - bw)", "bw = 6 * band + 5", "0.5 * (D_21 - D_12)", "s <= huber_chi * huber_chi", "A_ii = A_ii + damping"):
        assert text_ in raw, text_


def test_every_check_comes_before_the_library_is_loaded(monkeypatch):
    import torch
    from sslam_amd import lib
    from sslam_amd.pipeline import SequencePipeline

    def boom():
        raise AssertionError("the library was loaded before the arguments were judged")
    monkeypatch.setattr(lib, "graph", boom)
    E, N = 5, 4
    f, s = torch.zeros(E, dtype=torch.int32), torch.ones(E, dtype=torch.int32)
    Tm, info, Cc = torch.zeros((E, 12), dtype=torch.float64), torch.zeros((E, 21), dtype=torch.float64), torch.zeros((N, 12), dtype=torch.float64)
    ok = dict(first=f, second=s, T=Tm, info=info, C_in=Cc, band=2)
    bad = [dict(first=f.long()), dict(second=s[:4]), dict(T=Tm.float()), dict(T=Tm[:, :11]), dict(info=info[:4]), dict(info=info.numpy()),
           dict(C_in=Cc.float()), dict(C_in=Cc[:, :6]), dict(C_in=Cc.t()), dict(band=0), dict(band=True), dict(band=2.0), dict(huber_chi=0.0),
           dict(huber_chi=float("nan")), dict(huber_chi=float("inf")), dict(damping=-1.0), dict(damping=float("inf")), dict(damping=float("nan")),
           dict(iterations=-1), dict(iterations=17), dict(iterations=2.0), dict(workspace=torch.zeros(8, dtype=torch.uint8)),
           dict(out=(Cc,)), dict(first=torch.zeros((1, 0), dtype=torch.int32))]
    for change in bad:
        with pytest.raises(ValueError):
            lib.pose_graph(**dict(ok, **change))
    for change in (dict(band=33), dict(C_in=torch.zeros((4097, 12), dtype=torch.float64)),
                   dict(first=torch.zeros(2 ** 20 + 1, dtype=torch.int32), second=torch.zeros(2 ** 20 + 1, dtype=torch.int32))):
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.pose_graph(**dict(ok, **change))
    with pytest.raises(ValueError, match="CUDA"):                    # well-formed host tensors: refused, still nothing loaded
        lib.pose_graph(**ok)
    for Tbad in (Tm.float(), Tm[:, :11], Tm.numpy(), torch.zeros((2, 3, 4, 12), dtype=torch.float64)):
        with pytest.raises(ValueError):
            lib.chain_poses(Tbad)
    with pytest.raises(ValueError):
        lib.chain_poses(Tm, n_nodes=3)
    with pytest.raises(ValueError):
        lib.chain_poses(Tm, start=torch.zeros((2, 12), dtype=torch.float64))
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.chain_poses(torch.zeros((4096, 12), dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA"):
        lib.chain_poses(Tm)
    opt = SequencePipeline.optimize_pose_graph
    for args, kw in ((([0, 1], [1, 2], Tm[:2], info[:2], 0), {}), (([0, 1], [1], Tm[:2], info[:2], 3), {}),
                     ((f, [1] * E, Tm, info, 3), {}), ((f, s, Tm, info, 3), {}), (([0, 1], [1, 2], Tm, info[:2], 3), {}),
                     (([0, 0], [1, 2], Tm[:2], info[:2], 3), {}), (([0, 1], [1, 2], Tm[:2], info[:2], 3), dict(huber_chi=-1.0)),
                     (([0, 1], [1, 2], Tm[:2], info[:2], 3), dict(iterations=99))):
        with pytest.raises(ValueError):
            opt(*args, **kw)


def test_the_layers_judge_their_arguments_first(tmp_path):
    from sslam_amd import odometry as od
    from sslam_amd.harness import run_directory
    with pytest.raises(ValueError, match='"refine": True'):
        run_directory(str(tmp_path / "nowhere"), "none", (1, 5), evaluate={"odometry": True, "graph": True})
    with pytest.raises(ValueError, match="flag"):
        run_directory(str(tmp_path / "nowhere"), "none", (1, 5), evaluate={"odometry": True, "refine": True, "graph": 1})
    for spacings in ((), (5, 10), (1, 1)):
        with pytest.raises(ValueError, match="spacings"):
            od._check_graph(spacings, 12, None, None)
    sp, lists, n, band = od._check_graph(od.GRAPH_SPACINGS, 12, None, None)
    assert sp == (1, 5, 10) and n == 12 and band == 10 and [len(lists[s]) for s in sp] == [11, 7, 2]
    sp, lists, n, band = od._check_graph((1, 3), 9, 4, None)
    assert n == 5 and lists[3] == [(0, 3), (1, 4)] and band == 3
    with pytest.raises(ValueError):
        od._check_graph((1, 5), 1, None, None)
    with pytest.raises(ValueError):
        od.GraphSettings(4.0, -1.0, 8)                               # the record every graph call builds of its solver settings
    import evaluation as dropin
    for args in (([0], [1], np.zeros((1, 12)), np.zeros((1, 6, 6)), 2), ([0], [1], np.zeros((1, 4, 4)), np.zeros((1, 21)), 2),
                 ([0], [1, 2], np.zeros((1, 4, 4)), np.zeros((1, 6, 6)), 2)):
        with pytest.raises(ValueError):
            dropin.optimize_pose_graph(*args)


# ------------------------------------------------------------------------------------------------------------ the size limits
P = [0x10000 * (i + 1) for i in range(16)]       # never dereferenced: every call below is refused before the launch


def _graph_call(G, n_graphs=1, n_nodes=4, n_edges=5, band=2, chi=4.0, damping=0.0, n_iter=8, ptr=None):
    p = list(P) if ptr is None else ptr
    return G.sslg_pose_graph(p[0], p[1], p[2], p[3], n_graphs, n_nodes, n_edges, p[4], band, C.c_double(chi), C.c_double(damping), n_iter,
                             p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14], None)


def test_one_past_each_size_limit_is_refused_with_nothing_launched():
    from sslam_amd import lib
    G = lib.graph()
    before = G.sslg_launch_count()
    for entry, row in gt.LIMITS.items():
        for name, largest in row["largest"].items():
            if entry == "sslg_pose_graph":
                assert _graph_call(G, **{name: largest + 1}) == gt.E_UNSUPPORTED, (entry, name)
            else:
                kw = dict(n_graphs=1, n_nodes=4)
                kw[name] = largest + 1
                assert G.sslg_chain_poses(P[0], None, kw["n_graphs"], kw["n_nodes"], P[1], None) == gt.E_UNSUPPORTED, (entry, name)
    for shape in ((gt.MAX_GRAPHS + 1, 4, 2), (1, gt.MAX_NODES + 1, 2), (1, 4, gt.MAX_BAND + 1), (0, 4, 2), (1, 0, 2), (1, 4, 0)):
        assert G.sslg_pose_graph_workspace_bytes(*shape) == 0, shape
    # invalid arguments: -1, still nothing launched
    for kw in (dict(n_graphs=0), dict(n_nodes=0), dict(n_edges=0), dict(band=0), dict(chi=0.0), dict(chi=float("nan")), dict(chi=float("inf")),
               dict(damping=-1.0), dict(damping=float("nan")), dict(n_iter=-1), dict(n_iter=gt.MAX_ITER + 1)):
        assert _graph_call(G, **kw) == gt.E_INVALID, kw
    names = list(gt.ALIGN["sslg_pose_graph"])
    for k, name in enumerate(names):                               # a NULL, and a pointer that misses its alignment
        p = list(P)
        p[k] = None
        assert _graph_call(G, ptr=p) == gt.E_INVALID, name
        p[k] = P[k] + gt.ALIGN["sslg_pose_graph"][name] // 2
        assert _graph_call(G, ptr=p) == gt.E_INVALID, name
        p[k] = P[k] + gt.ALIGN["sslg_pose_graph"][name]
        assert _graph_call(G, n_nodes=gt.MAX_NODES + 1, ptr=p) == gt.E_UNSUPPORTED, name      # at its alignment: judged by size
    p = list(P)
    p[6] = p[4]
    assert _graph_call(G, ptr=p) == gt.E_INVALID, "C must not be C_in"
    assert G.sslg_chain_poses(None, None, 1, 2, P[1], None) == gt.E_INVALID and G.sslg_chain_poses(P[0], None, 1, 2, None, None) == gt.E_INVALID
    assert G.sslg_chain_poses(P[0], P[1], 1, 2, P[1], None) == gt.E_INVALID and G.sslg_chain_poses(P[0] + 4, None, 1, 2, P[1], None) == gt.E_INVALID
    assert G.sslg_chain_poses(P[0], None, 0, 2, P[1], None) == gt.E_INVALID and G.sslg_chain_poses(P[0], None, 1, 0, P[1], None) == gt.E_INVALID
    assert G.sslg_launch_count() == before, "a refused call launches nothing"
    # the workspace size is what the table and the wrapper say, at the limits too
    for shape in ((1, 1, 1), (1, 2, 1), (3, 40, 20), (1, 613, 20), (1, 34, 32), (gt.MAX_GRAPHS, gt.MAX_NODES, gt.MAX_BAND)):
        assert G.sslg_pose_graph_workspace_bytes(*shape) == gt.workspace_bytes(*shape) == lib.pose_graph_workspace_bytes(*shape), shape
    assert gt.workspace_bytes(gt.MAX_GRAPHS, gt.MAX_NODES, gt.MAX_BAND) > 2 ** 40, "why the graph offsets are 64 bits wide"
    assert 6 * (gt.MAX_NODES - 1) * (6 * gt.MAX_BAND + 6) < 2 ** 31, "why a row offset fits 31 bits"
