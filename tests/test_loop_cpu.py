"""Loop closures without a GPU: the restatement (tests/loop_ref.py) against independent statements - the oracle's similarity
chain, a brute-force candidate search, the banded restatement (tests/pose_graph_ref.py) and a dense solve of independently formed
normal equations - the planted loop study DESIGN.md section 4l records, and the interface of libsslam_loop.so:
include/sslam_loop.h, sslam_amd.lib.LOOP_EXPORTS and tests/loop_table.py hold the same entries (the built library's symbols are
tests/test_libraries_cpu.py), every host-side check raises before the library is loaded, and one past each size limit is refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import loop_cases as lc
import loop_ref as ref
import loop_table as lt
import pose_graph_cases as pc
import pose_graph_ref as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sslam_loop.h")
SPARSE = lc.sparse_cases()
BY = {c["name"]: c for c in SPARSE}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


# ------------------------------------------------------------------------------------------------------- signatures, candidates
def test_the_float32_chains_are_the_oracles():
    """fmaf32 - a fused multiply-add made of float64 operations - gives the bits of the oracle's C fmaf chain: the raw sums (a chain
    over the keypoints) and the similarity (a chain over the columns, ora.sim_matrix(sig, sig))."""
    from oracle import ora
    for d, k, seed in ((128, 63, 1), (256, 65, 2)):
        desc, scores = lc.bank(5, k, d, seed)
        raw = ref.raw_signatures(desc, scores)
        want = np.stack([ora.sim_matrix(scores[i:i + 1], np.ascontiguousarray(desc[i].T))[0] for i in range(5)])
        assert np.array_equal(_bits(raw), _bits(want)), d
        sig = ref.signatures(desc, scores)
        assert np.array_equal(_bits(ref.similarity(sig)), _bits(ora.sim_matrix(sig, sig))), d
    rng = np.random.default_rng(3)                                  # and where the float64 sum itself is inexact: wide exponent ranges
    a, b = (rng.standard_normal((64, 200)) * 10.0 ** rng.integers(-6, 6, (64, 200))).astype(np.float32), rng.standard_normal((64, 200)).astype(np.float32)
    S = np.zeros((64, 64), np.float32)
    for c in range(200):
        S = ref.fmaf32(a[:, None, c], b[None, :, c], S)
    assert np.array_equal(_bits(S), _bits(ora.sim_matrix(a, b)))


def test_signatures_are_centred_unit_vectors():
    """The reason for the centring, on banks that share a strong common part: the raw sums of all frames are nearly parallel (every cosine
    above 0.9); the centred signatures are unit vectors whose cosines take both signs."""
    desc, scores = lc.bank(9, 40, 128, 4)
    raw = ref.raw_signatures(desc, scores).astype(np.float64)
    sig = ref.signatures(desc, scores).astype(np.float64)
    unit = raw / np.linalg.norm(raw, axis=1, keepdims=True)
    assert (unit @ unit.T).min() > 0.9, "raw sums: every pair nearly parallel"
    assert np.abs(np.linalg.norm(sig, axis=1) - 1).max() < 1e-5
    off = (sig @ sig.T)[~np.eye(9, dtype=bool)]
    assert off.min() < -0.3, "centred: the cosines spread over both signs"
    desc, scores = lc.bank(9, 40, 128, 4, zero_frame=3)
    raw, sig = ref.raw_signatures(desc, scores), ref.signatures(desc, scores).astype(np.float64)
    assert (raw[3] == 0).all() and np.abs(np.linalg.norm(sig[3]) - 1) < 1e-5, "a frame without scores is the mean's opposite, still a unit vector"
    one = ref.signatures(desc[:1], scores[:1])
    assert (one == 0).all(), "one frame: the centred sum is zero, and so is the signature"
    assert (ref.candidates(one, 1, -1.0, 2, 0)["count"] == 0).all()


def _brute_force(S, min_gap, min_sim, per_frame, suppress):
    """The candidates, written differently: all eligible frames sorted once by (value descending, j ascending), then taken in that
    order unless within `suppress` of one already taken."""
    n = len(S)
    first, second, sim, count = [], [], [], []
    for i in range(n):
        order = sorted((j for j in range(n) if j <= i - min_gap and S[i, j] >= np.float32(min_sim)), key=lambda j: (-float(S[i, j]), j))
        taken = []
        for j in order:
            if len(taken) < per_frame and all(abs(j - t) > suppress for t in taken):
                taken.append(j)
        pad = per_frame - len(taken)
        first += taken + [-1] * pad
        second += [i] * len(taken) + [-1] * pad
        sim += [S[i, j] for j in taken] + [np.float32(0)] * pad
        count.append(len(taken))
    return dict(first=np.array(first, np.int32), second=np.array(second, np.int32), sim=np.array(sim, np.float32), count=np.array(count, np.int32))


@pytest.mark.parametrize("case", lc.candidate_cases() + lc.candidate_size_cases()[:4], ids=lambda c: c["name"])
def test_candidates_equal_a_brute_force_search(case):
    S = ref.similarity(case["sig"])
    got = ref.candidates(case["sig"], case["min_gap"], case["min_sim"], case["per_frame"], case["suppress"], S=S)
    want = _brute_force(S, case["min_gap"], case["min_sim"], case["per_frame"], case["suppress"])
    for key in ref.CANDIDATE_KEYS:
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key
    filled = got["first"] >= 0
    assert (got["first"][filled] < got["second"][filled]).all() and (got["second"][filled] - got["first"][filled] >= case["min_gap"]).all()
    pf = case["per_frame"]
    assert np.array_equal(filled.reshape(-1, pf).sum(axis=1), got["count"]) and (np.diff(filled.reshape(-1, pf).astype(int), axis=1) <= 0).all()


def test_the_candidate_rows_of_the_contract():
    by = {c["name"]: c for c in lc.candidate_cases()}
    run = lambda c: ref.candidates(c["sig"], c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"])
    r = run(by["duplicate_frames"])                                 # frames 0 .. 4 and 12 are one signature
    assert list(r["first"][12 * 4:13 * 4]) == [0, 1, 2, 3] and len(set(_bits(r["sim"][12 * 4:13 * 4]).tolist())) == 1, "equal sims: the lower j first"
    assert list(run(by["duplicate_frames_suppressed"])["first"][12 * 4:13 * 4])[:3] == [0, 2, 4]
    for name in ("gap_at_least_n", "gap_past_n"):
        r = run(by[name])
        assert (r["count"] == 0).all() and (r["first"] == -1).all() and (r["second"] == -1).all() and (_bits(r["sim"]) == 0).all()
    r = run(by["suppression_clipped_at_frame_0"])
    assert r["first"][30 * 3] == 1 and (np.abs(r["first"][30 * 3 + 1:31 * 3] - 1) > 5).all() and r["count"][30] == 3
    assert run(by["per_frame_8"])["count"].max() == 8 and run(by["per_frame_1"])["count"].max() == 1
    r = run(by["fewer_eligible_than_slots"])
    assert 0 < r["count"].max() < 8
    assert run(by["everything_suppressed_after_one"])["count"].max() == 1


# ------------------------------------------------------------------------------------------------------------- the sparse graph
def test_the_edge_terms_and_blocks_are_the_banded_restatements_bit_for_bit():
    """The sparse restatement evaluates and stages its edges with pose_graph_ref's functions; its blocks D_m, g_m and B_e equal, bit
    for bit, the corresponding entries of the banded restatement's A and g at a band that holds every edge."""
    for c in (lc.from_banded(pc.shape_cases()[5]), BY["huber_and_damping"],
              BY["hub_of_70"]):
        n_nodes = len(c["C_in"])
        G, B = ref.SparseGraph(c["first"], c["second"], c["T"], c["info"], n_nodes), pg.Graph(c["first"], c["second"], c["T"], c["info"], n_nodes, n_nodes)
        assert np.array_equal(G.slots, B.slots)
        ev, evb = G.eval(c["C_in"], c["chi"]), pg.edge_eval(c["C_in"], B.a, B.b, B.T[B.slots], B.info[B.slots], c["chi"])
        for key in ("Tp", "s", "w", "rho"):
            assert np.array_equal(_bits(ev[key]), _bits(evb[key])), key
        D, g, BA = G.blocks(c["C_in"], c["chi"], c["damping"])
        A, gb = B.assemble(c["C_in"], c["chi"], c["damping"])
        low = np.tri(6, dtype=bool)
        for m in range(1, n_nodes):
            r = 6 * (m - 1)
            assert np.array_equal(_bits(D[m - 1][low]), _bits(A[r:r + 6, r:r + 6][low])), m
        assert np.array_equal(_bits(g.reshape(-1)), _bits(gb))
        pairs = list(zip(G.a, G.b))
        for k, (a, b) in enumerate(pairs):
            if a >= 1 and pairs.count((a, b)) == 1:
                assert np.array_equal(_bits(BA[k]), _bits(A[6 * (b - 1):6 * b, 6 * (a - 1):6 * a])), (a, b)


def _banded_and_sparse():
    out = []
    for c in pc.shape_cases():
        banded = pc.run(c)
        sparse = ref.optimize(c["first"], c["second"], c["T"], c["info"], c["C_in"], c["chi"], c["damping"], c["n_iter"], 4096, 1e-10, detail=True)
        out.append((c, banded, sparse))
    return out


@pytest.fixture(scope="module")
def banded_and_sparse():
    return _banded_and_sparse()


COST_BOUND = 4e-14      # ten times the largest observed below (3.7e-15, huber_branch)


def test_on_band_limited_graphs_the_sparse_solve_reaches_the_banded_result(banded_and_sparse):
    """pose_graph_cases.shape_cases() from the same start, cg_tol 1e-10 and 4096 iterations allowed: the same status, the same
    number of accepted steps, and the final cost within COST_BOUND of the banded restatement's, relative.  Measured: the largest
    relative difference is 3.7e-15 (huber_branch; 0 to 8.5e-16 elsewhere); the bound is ten times that."""
    worst = 0.0
    for c, banded, sparse in banded_and_sparse:
        assert sparse["status"] == banded["status"] == 0 and sparse["iterations"] == banded["iterations"], c["name"]
        rel = abs(sparse["cost"] - banded["cost"]) / banded["cost"] if banded["cost"] > 0 else abs(sparse["cost"])
        print(f"{c['name']}: cost banded {banded['cost']!r} sparse {sparse['cost']!r} relative difference {rel:.3g}, cg_steps {sparse['cg_steps'][:9].tolist()}")
        worst = max(worst, rel)
        assert rel <= COST_BOUND, (c["name"], rel)
        assert (sparse["used_edges"], sparse["skipped_edges"], sparse["failed_row"]) == (banded["used_edges"], banded["skipped_edges"], banded["failed_row"])
    print(f"largest relative difference of the final cost: {worst:.3g}")


SOLVE_BOUND = 3e-10     # ten times the largest observed below (2.62e-11), relative to the first step's |dense|_inf


def test_every_cg_solution_solves_the_independent_dense_system(banded_and_sparse):
    """Every step's delta against np.linalg.solve on pose_graph_ref.plain_normal_equations (band = n_nodes) at that step's poses:
    |delta - dense|_inf <= SOLVE_BOUND * |dense|_inf of the graph's FIRST step.  The scale is the first step's because the error is
    absolute - rounding in g, 1e-17 to 1e-13 here - while |dense| falls to 1e-12 as the iteration converges; a graph that starts
    at its minimum (two_nodes_one_edge: |dense| 3e-18) has nothing to solve and is left out.  Measured over the 48 steps of
    pose_graph_cases.shape_cases(): the largest is 2.62e-11; the bound is ten times that."""
    worst, steps = 0.0, 0
    for c, _, sparse in banded_and_sparse:
        n_nodes = len(c["C_in"])
        scale = None
        for st in sparse["steps"]:
            _, A, g = pg.plain_normal_equations(c["first"], c["second"], c["T"], c["info"], st["C"], n_nodes, c["chi"], c["damping"])
            dense = np.linalg.solve(A, -g)
            scale = np.abs(dense).max() if scale is None else scale
            if scale < 1e-12:                                        # the graph starts at its minimum: rounding error on both sides
                break
            rel = np.abs(st["delta"] - dense).max() / scale
            worst, steps = max(worst, rel), steps + 1
            print(f"{c['name']}: |dense|_inf {np.abs(dense).max():.3g}, |delta - dense|_inf / first step's |dense|_inf {rel:.3g}")
            assert rel <= SOLVE_BOUND, (c["name"], rel)
    print(f"{steps} CG solutions, largest |delta - dense|_inf / first step's |dense|_inf: {worst:.3g}")
    assert steps >= 40


def test_the_sparse_rows_of_the_contract():
    r = lc.run(BY["two_nodes_one_edge"])
    assert r["status"] == 0 and r["iterations"] == 1 and r["cg_steps"][0] == 1, "one block: the preconditioner is the inverse"
    r = lc.run(BY["exact_graph_plus_0_4"])
    assert r["status"] == 1 and r["cost"] == 0.0 and (r["cg_steps"] == 0).all() and r["used_edges"] == 8
    assert r["C"].tobytes() == BY["exact_graph_plus_0_4"]["C_in"].tobytes()
    r = lc.run(BY["forty_nodes_322_slots"])
    assert (r["used_edges"], r["skipped_edges"]) == (316, 5) and r["status"] == 0
    assert (r["edge_chi2"][[7, 20, 200, 41, 170, 300]] == 0).all() and (r["edge_chi2"][149:161] > 0).all(), "the loop edges are used"
    c = BY["hub_of_70"]
    G = ref.SparseGraph(c["first"], c["second"], c["T"], c["info"], len(c["C_in"]))
    assert G.degree[5] == 72 and len(G.rounds) == 72 and lc.run(c)["status"] == 0
    r = lc.run(BY["unreachable_node"])
    assert r["status"] == 2 and r["failed_row"] == 6 * (3 - 1) and r["iterations"] == 0 and r["cost"] == r["cost_in"] and (r["cg_steps"] == 0).all()
    assert r["C"].tobytes() == BY["unreachable_node"]["C_in"].tobytes()
    assert 6 * (len(BY["rows_258_past_one_stride"]["C_in"]) - 1) == 258 and len(BY["nodes_257_past_one_stride"]["C_in"]) - 1 == 257
    r = lc.run(BY["no_iterations"])
    assert r["status"] == 1 and r["iterations"] == 0 and r["cost"] == r["cost_in"] > 0 and (r["cg_steps"] == 0).all()
    r = lc.run(BY["one_cg_iteration"])
    assert r["status"] == 0 and set(r["cg_steps"][:r["iterations"]].tolist()) == {1}, "an inexact step is still a descent step"
    r = lc.run(BY["cg_tol_zero"])
    assert r["status"] == 0 and (r["cg_steps"][:3] == 40).all(), "cg_tol 0 never stops early"
    full = lc.run(dict(BY["one_cg_iteration"], cg_iterations=512))
    assert full["cost"] < lc.run(BY["one_cg_iteration"])["cost"]
    for c in SPARSE:                                                # everywhere: the anchor bit for bit, the cost never rises
        r = lc.run(c)
        assert r["C"][0].tobytes() == np.asarray(c["C_in"])[0].tobytes() and (r["status"] == 3 or r["cost"] <= r["cost_in"]), c["name"]
    bad = dict(BY["no_iterations"], C_in=BY["no_iterations"]["C_in"].copy())
    bad["C_in"][3, 7] = np.nan
    r = lc.run(bad)
    assert r["status"] == 3 and r["used_edges"] == 23 and (r["edge_chi2"] == 0).all() and (r["cg_steps"] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ the study
STUDY_SEEDS = (0, 1, 2, 3)


def test_planted_loop_study_loop_edges_lower_the_error_in_every_seed():
    """420 planted frames whose path turns a full circle in about 370, the five spacings, 3 % gross outliers, noise x 3 (sigma_t 0.03,
    sigma_r 0.012), and 30 loop edges (a, a + 370), a = 0 .. 29, measured at a spacing-1 edge's noise (tests/loop_cases.py).  Gauss-
    Newton with PCG at cg_tol 1e-3, at most 600 iterations.  Position rmse after rigid alignment (metres), seeds 0 - 3, odometry
    edges only / with the loop edges: 0.0743 / 0.0402, 0.0407 / 0.0339, 0.0388 / 0.0312, 0.0521 / 0.0327 - medians 0.0464 and
    0.0333.  The odometry-only figures are those of the prototype quoted in the issue to four digits; the loop figures differ from
    it in the third digit, as the loop edges' noise draw is this file's own.  Asserted: the loop edges lower the error in every
    seed."""
    odo, loops = [], []
    for seed in STUDY_SEEDS:
        c = lc.study_case(seed)
        n = c["n_odometry"]
        assert n == 2049 and len(c["first"]) == n + 30
        o = ref.optimize(c["first"][:n], c["second"][:n], c["T"][:n], c["info"][:n], c["C_in"], 4.0, 0.0, 8, 600, 1e-3)
        w = ref.optimize(c["first"], c["second"], c["T"], c["info"], c["C_in"], 4.0, 0.0, 8, 600, 1e-3)
        assert o["status"] == 0 and w["status"] == 0
        odo.append(pc.ate_rmse(o["C"], c["truth"]))
        loops.append(pc.ate_rmse(w["C"], c["truth"]))
        print(f"seed {seed}: chain {pc.ate_rmse(c['C_in'], c['truth']):.4f} m, odometry edges {odo[-1]:.4f} m in {o['iterations']} steps, CG "
              f"{o['cg_steps'][:9].tolist()}; with loop edges {loops[-1]:.4f} m in {w['iterations']} steps, CG {w['cg_steps'][:9].tolist()}")
    print(f"planted loop study, median ate rmse over {len(STUDY_SEEDS)} seeds: odometry edges {np.median(odo):.4f} m, with loop edges {np.median(loops):.4f} m")
    assert all(w < o for w, o in zip(loops, odo)), (odo, loops)


def test_pruning_by_chi2_is_a_second_run_on_the_reduced_list():
    """What odometry_loop_graph does with prune_chi, on the restatement: the slots whose edge_chi2 exceeds prune_chi^2 after the
    first run become absent, and the second run starts from the same poses.  A planted FALSE loop edge (two places 60 frames
    apart declared one) is among the pruned; whether the second run then does better than the first is printed, not asserted."""
    c = lc.with_loops(120, pc.SPACINGS, 31, [(a, a + 100) for a in range(0, 20, 2)], outliers=0.03)
    false_T = pg.compose(c["truth"][70], pg.inverse(c["truth"][10]))[None]          # frame 100 is said to be where frame 70 is
    first, second = np.append(c["first"], 10).astype(np.int32), np.append(c["second"], 100).astype(np.int32)
    T, info = np.concatenate([c["T"], false_T]), np.concatenate([c["info"], c["info"][-1:]])
    one = ref.optimize(first, second, T, info, c["C_in"], 4.0, 0.0, 8, 512, 1e-3)
    prune_chi = 6.0
    gone = one["edge_chi2"] > prune_chi ** 2
    assert gone[-1], "the false loop edge stands out"
    two = ref.optimize(np.where(gone, -1, first).astype(np.int32), second, T, info, c["C_in"], 4.0, 0.0, 8, 512, 1e-3)
    assert two["used_edges"] == one["used_edges"] - int(gone.sum()) and two["skipped_edges"] == 0 and (two["edge_chi2"][gone] == 0).all()
    clean = ref.optimize(first[:-1], second[:-1], T[:-1], info[:-1], c["C_in"], 4.0, 0.0, 8, 512, 1e-3)
    print(f"pruning at chi {prune_chi}: {int(gone.sum())} slots pruned; ate rmse with the false edge {pc.ate_rmse(one['C'], c['truth']):.4f} m, "
          f"after pruning {pc.ate_rmse(two['C'], c['truth']):.4f} m, without it from the start {pc.ate_rmse(clean['C'], c['truth']):.4f} m")


# ---------------------------------------------------------------------------------------------------------------- the interface
def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_header_symbols_exports_and_table_agree():
    """The table, the constants and the key lists against the export list; that list against the header and the built library is
    tests/test_libraries_cpu.py."""
    from sslam_amd import lib
    declared = lib.LOOP_EXPORTS
    assert set(lt.ALIGN) | set(lt.HOST_ONLY) == set(declared) and not set(lt.ALIGN) & set(lt.HOST_ONLY) and set(lt.LIMITS) == set(lt.ALIGN)
    consts = {k: int(v) for k, v in re.findall(r"#define (SSLL_\w+) (\d+)", open(HEADER).read())}
    assert consts == dict(SSLL_MAX_FRAMES=lt.MAX_FRAMES, SSLL_MAX_K=lt.MAX_K, SSLL_MAX_PER_FRAME=lt.MAX_PER_FRAME, SSLL_MAX_NODES=lt.MAX_NODES,
                          SSLL_MAX_EDGES=lt.MAX_EDGES, SSLL_MAX_GRAPHS=lt.MAX_GRAPHS, SSLL_GRAPH_MAX_ITER=lt.MAX_ITER, SSLL_MAX_CG=lt.MAX_CG,
                          SSLL_FRAMES_PER_GROUP=ref.FRAMES_PER_GROUP)
    assert (lib.LOOP_MAX_FRAMES, lib.LOOP_MAX_K, lib.LOOP_MAX_PER_FRAME, lib.SPARSE_MAX_NODES, lib.SPARSE_MAX_EDGES, lib.SPARSE_MAX_GRAPHS,
            lib.SPARSE_MAX_ITER, lib.SPARSE_MAX_CG) == \
        (lt.MAX_FRAMES, lt.MAX_K, lt.MAX_PER_FRAME, lt.MAX_NODES, lt.MAX_EDGES, lt.MAX_GRAPHS, lt.MAX_ITER, lt.MAX_CG) == \
        (ref.MAX_FRAMES, ref.MAX_K, ref.MAX_PER_FRAME, ref.MAX_NODES, ref.MAX_EDGES, ref.MAX_GRAPHS, ref.MAX_ITER, ref.MAX_CG)
    assert lib.POSE_GRAPH_SPARSE_KEYS == ref.KEYS and lib.LOOP_CANDIDATE_KEYS == ref.CANDIDATE_KEYS


def test_the_header_states_both_tables_line_for_line():
    elem = {"int32_t": 4, "double": 8, "float": 4, "void": 4}
    text = _header()
    for entry, row in lt.ALIGN.items():
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*?)\)\s*;", text)
        assert m, entry
        args = [re.match(r"(.*?)(\w+)$", " ".join(a.split())).groups() for a in m.group(1).split(",")]
        pointers = [(t.strip(), n) for t, n in args if "*" in t and n != "stream"]
        assert [n for _, n in pointers] == list(row), entry
        for t, n in pointers:                                       # at least the element; more where the kernel reads vectors
            assert row[n] % elem[t.replace("const", "").replace("*", "").strip()] == 0, (entry, n)
    raw = open(HEADER).read()
    for title, lines, count in (("ALIGNMENT, every entry", lt.header_lines(), len(lt.ALIGN)), ("SIZE LIMITS: the expressions", lt.limit_lines(), len(lt.LIMITS))):
        start = raw.index(title)
        stated = re.sub(r"\n \*\s+", " ", raw[start:raw.index("*/", start)]).strip()          # the block's lines joined, the margin dropped
        for line in lines:
            assert line + " " in stated + " ", f"include/sslam_loop.h does not state: {line}"
        assert len(re.findall(r"\bssll_\w+: ", stated)) == count
    for text_ in ("acc = fmaf(scores[i][kk], desc[i][kk][c], acc)", "fmaxf(sqrtf(ss_i), 1e-12f)", "acc = fmaf(sig[i][c], sig[j][c], acc)",
                  "rz1 <= (cg_tol * cg_tol) * rz0", "there is no band test", "WHY CENTRED"):
        assert text_ in raw, text_


def test_every_check_comes_before_the_library_is_loaded(monkeypatch):
    import torch
    from sslam_amd import lib
    from sslam_amd.pipeline import SequencePipeline

    def boom():
        raise AssertionError("the library was loaded before the arguments were judged")
    monkeypatch.setattr(lib, "loop", boom)
    desc, scores = torch.zeros((3, 5, 128)), torch.zeros((3, 5))
    for args in ((desc.double(), scores), (desc[:, :, :100], scores), (desc, scores[:2]), (desc, scores.double()), (desc, None), (desc.numpy(), scores),
                 (desc.transpose(0, 1), scores)):
        with pytest.raises(ValueError):
            lib.frame_signatures(*args)
    with pytest.raises(ValueError):
        lib.frame_signatures(desc, scores, out=torch.zeros((3, 64)))
    with pytest.raises(ValueError):
        lib.frame_signatures(desc, scores, workspace=torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.frame_signatures(torch.zeros((1, 4097, 128)), torch.zeros((1, 4097)))
    with pytest.raises(ValueError, match="CUDA"):
        lib.frame_signatures(desc, scores)
    sig = torch.zeros((6, 128))
    for kw in (dict(min_gap=0), dict(min_gap=1.5), dict(min_gap=True), dict(min_sim=float("nan")), dict(min_sim=float("inf")), dict(min_sim="x"),
               dict(per_frame=0), dict(per_frame=9), dict(suppress=-1), dict(suppress=2.0), dict(out=(sig,))):
        with pytest.raises(ValueError):
            lib.loop_candidates(sig, **kw)
    for bad in (sig.double(), torch.zeros((6, 100)), torch.zeros(6), sig.numpy()):
        with pytest.raises(ValueError):
            lib.loop_candidates(bad)
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.loop_candidates(torch.zeros((4097, 128)))
    with pytest.raises(ValueError, match="CUDA"):
        lib.loop_candidates(sig)
    E, N = 5, 4
    f, s = torch.zeros(E, dtype=torch.int32), torch.ones(E, dtype=torch.int32)
    Tm, info, Cc = torch.zeros((E, 12), dtype=torch.float64), torch.zeros((E, 21), dtype=torch.float64), torch.zeros((N, 12), dtype=torch.float64)
    ok = dict(first=f, second=s, T=Tm, info=info, C_in=Cc)
    bad = [dict(first=f.long()), dict(second=s[:4]), dict(T=Tm.float()), dict(T=Tm[:, :11]), dict(info=info[:4]), dict(info=info.numpy()),
           dict(C_in=Cc.float()), dict(C_in=Cc[:, :6]), dict(C_in=Cc.t()), dict(huber_chi=0.0), dict(huber_chi=float("nan")), dict(damping=-1.0),
           dict(damping=float("inf")), dict(iterations=-1), dict(iterations=17), dict(iterations=2.0), dict(cg_iterations=0), dict(cg_iterations=2.5),
           dict(cg_iterations=True), dict(cg_tol=-1e-3), dict(cg_tol=float("nan")), dict(cg_tol=float("inf")), dict(cg_tol="x"),
           dict(workspace=torch.zeros(8, dtype=torch.uint8)), dict(out=(Cc,)), dict(first=torch.zeros((1, 0), dtype=torch.int32))]
    for change in bad:
        with pytest.raises(ValueError):
            lib.pose_graph_sparse(**dict(ok, **change))
    for change in (dict(cg_iterations=4097), dict(C_in=torch.zeros((4097, 12), dtype=torch.float64)),
                   dict(first=torch.zeros(65537, dtype=torch.int32), second=torch.zeros(65537, dtype=torch.int32))):
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.pose_graph_sparse(**dict(ok, **change))
    with pytest.raises(ValueError, match="CUDA"):                    # well-formed host tensors: refused, still nothing loaded
        lib.pose_graph_sparse(**ok)
    opt = SequencePipeline.optimize_pose_graph_sparse
    for args, kw in ((([0, 1], [1, 2], Tm[:2], info[:2], 0, Cc), {}), (([0, 1], [1], Tm[:2], info[:2], 4, Cc), {}), ((f, [1] * E, Tm, info, 4, Cc), {}),
                     (([0, 1], [1, 2], Tm, info[:2], 4, Cc), {}), (([0, 1], [1, 2], Tm[:2], info[:2], 4, None), {}),
                     (([0, 1], [1, 2], Tm[:2], info[:2], 4, Cc[:3]), {}), (([0, 1], [1, 2], Tm[:2], info[:2], 4, Cc), dict(cg_iterations=0)),
                     (([0, 1], [1, 2], Tm[:2], info[:2], 4, Cc), dict(cg_tol=-1.0)), (([0, 1], [1, 2], Tm[:2], info[:2], 4, Cc), dict(iterations=99))):
        with pytest.raises(ValueError):
            opt(*args, **kw)
    assert lib.pose_graph_sparse_shapes(2, 5, 7)["cg_steps"] == ((2, 16), torch.int32)


# ------------------------------------------------------------------------------------------------------------ the size limits
P = [0x10000 * (i + 1) for i in range(17)]       # never dereferenced: every call below is refused before the launch


def _sparse_call(L, n_graphs=1, n_nodes=4, n_edges=5, chi=4.0, damping=0.0, n_iter=8, cg_iterations=10, cg_tol=1e-3, ptr=None):
    p = list(P) if ptr is None else ptr
    return L.ssll_pose_graph_sparse(p[0], p[1], p[2], p[3], n_graphs, n_nodes, n_edges, p[4], C.c_double(chi), C.c_double(damping), n_iter,
                                    cg_iterations, C.c_double(cg_tol), *p[5:16], None)


def _sig_call(L, n_frames=3, k=5, d=128, ptr=None):
    p = list(P) if ptr is None else ptr
    return L.ssll_frame_signatures(p[0], p[1], n_frames, k, d, p[2], p[3], None)


def _cand_call(L, n_frames=3, d=128, min_gap=1, min_sim=0.3, per_frame=2, suppress=0, ptr=None):
    p = list(P) if ptr is None else ptr
    return L.ssll_loop_candidates(p[0], n_frames, d, min_gap, C.c_float(min_sim), per_frame, suppress, p[1], p[2], p[3], p[4], None)


def test_one_past_each_size_limit_is_refused_with_nothing_launched():
    from sslam_amd import lib
    L = lib.loop()
    before = L.ssll_launch_count()
    calls = dict(ssll_frame_signatures=_sig_call, ssll_loop_candidates=_cand_call, ssll_pose_graph_sparse=_sparse_call)
    for entry, row in lt.LIMITS.items():
        for name, largest in row["largest"].items():
            assert calls[entry](L, **{name: largest + 1}) == lt.E_UNSUPPORTED, (entry, name)
    assert _sig_call(L, d=64) == lt.E_UNSUPPORTED and _cand_call(L, d=192) == lt.E_UNSUPPORTED
    for shape in ((lt.MAX_GRAPHS + 1, 4, 2), (1, lt.MAX_NODES + 1, 2), (1, 4, lt.MAX_EDGES + 1), (0, 4, 2), (1, 0, 2), (1, 4, 0)):
        assert L.ssll_pose_graph_sparse_workspace_bytes(*shape) == 0, shape
    # invalid arguments: -1, still nothing launched
    for kw in (dict(n_graphs=0), dict(n_nodes=0), dict(n_edges=0), dict(chi=0.0), dict(chi=float("nan")), dict(chi=float("inf")), dict(damping=-1.0),
               dict(damping=float("nan")), dict(n_iter=-1), dict(n_iter=lt.MAX_ITER + 1), dict(cg_iterations=0), dict(cg_tol=-1.0),
               dict(cg_tol=float("nan")), dict(cg_tol=float("inf"))):
        assert _sparse_call(L, **kw) == lt.E_INVALID, kw
    for kw in (dict(n_frames=0), dict(k=0), dict(d=0)):
        assert _sig_call(L, **kw) == lt.E_INVALID, kw
    for kw in (dict(n_frames=0), dict(d=0), dict(min_gap=0), dict(per_frame=0), dict(suppress=-1), dict(min_sim=float("nan")), dict(min_sim=float("inf"))):
        assert _cand_call(L, **kw) == lt.E_INVALID, kw
    over = dict(ssll_frame_signatures=dict(n_frames=lt.MAX_FRAMES + 1), ssll_loop_candidates=dict(n_frames=lt.MAX_FRAMES + 1),
                ssll_pose_graph_sparse=dict(n_nodes=lt.MAX_NODES + 1))
    for entry, call in calls.items():
        for k, name in enumerate(lt.ALIGN[entry]):                 # a NULL, and a pointer that misses its alignment
            p = list(P)
            p[k] = None
            assert call(L, ptr=p) == lt.E_INVALID, (entry, name)
            p[k] = P[k] + lt.ALIGN[entry][name] // 2
            assert call(L, ptr=p) == lt.E_INVALID, (entry, name)
            p[k] = P[k] + lt.ALIGN[entry][name]
            assert call(L, ptr=p, **over[entry]) == lt.E_UNSUPPORTED, (entry, name)      # at its alignment: judged by size
    p = list(P)
    p[6] = p[4]
    assert _sparse_call(L, ptr=p) == lt.E_INVALID, "C must not be C_in"
    assert L.ssll_launch_count() == before, "a refused call launches nothing"
    # the workspace size is what the table and the wrapper say, at the limits too
    for shape in ((1, 1, 1), (1, 2, 1), (3, 40, 322), (1, 613, 3000), (1, 44, 87), (lt.MAX_GRAPHS, lt.MAX_NODES, lt.MAX_EDGES)):
        assert L.ssll_pose_graph_sparse_workspace_bytes(*shape) == lt.sparse_workspace_bytes(*shape) == lib.pose_graph_sparse_workspace_bytes(*shape), shape
    assert lt.sparse_workspace_bytes(lt.MAX_GRAPHS, lt.MAX_NODES, lt.MAX_EDGES) > 2 ** 40, "why the graph offsets are 64 bits wide"
    assert 90 * lt.MAX_EDGES < 2 ** 31 and lt.MAX_FRAMES * 256 < 2 ** 31 and lt.MAX_FRAMES * lt.MAX_K * 256 >= 2 ** 31, "the stated index widths"


def test_the_layers_judge_their_arguments_first(tmp_path):
    from sslam_amd import odometry as od
    from sslam_amd.harness import run_directory
    base = {"odometry": True, "refine": True}
    with pytest.raises(ValueError, match='"graph": True'):
        run_directory(str(tmp_path / "nowhere"), "none", (1, 5), evaluate=dict(base, loops=True))
    with pytest.raises(ValueError, match='"graph": True'):
        run_directory(str(tmp_path / "nowhere"), "none", (1, 5), evaluate=dict(base, loops={"min_gap": 10}))
    for loops in (1, "yes", {"gap": 3}, {"min_gap": 0}, {"per_frame": 9}, {"min_inliers": -1}, {"cg_iterations": 0}, {"cg_tol": -1.0}, {"prune_chi": 0.0}):
        with pytest.raises(ValueError):
            run_directory(str(tmp_path / "nowhere"), "none", (1, 5), evaluate=dict(base, graph=True, loops=loops))
    assert od.check_loops(None) == od.check_loops(True) == od.LOOP_DEFAULTS and od.check_loops({"min_gap": 7})["min_gap"] == 7
    for args in (({"min_sim": float("nan")},), ({"suppress": -1},), (None, 0), (None, 5000.5), (None, 10, float("inf")), (None, 10, 1e-3, -2.0), ([],)):
        with pytest.raises(ValueError):
            od.check_loops(*args)
    with pytest.raises(Exception, match="unsupported"):
        od.check_loops(None, 4097)
    import evaluation as dropin
    for args in (([0], [1], np.zeros((1, 12)), np.zeros((1, 6, 6)), 2, np.zeros((2, 4, 4))), ([0], [1], np.zeros((1, 4, 4)), np.zeros((1, 21)), 2, np.zeros((2, 4, 4))),
                 ([0], [1], np.zeros((1, 4, 4)), np.zeros((1, 6, 6)), 2, np.zeros((3, 4, 4))), ([0], [1], np.zeros((1, 4, 4)), np.zeros((1, 6, 6)), 2, None)):
        with pytest.raises(ValueError):
            dropin.optimize_pose_graph_sparse(*args)
    for args in ((np.zeros((3, 4, 100)), np.zeros((3, 4))), (np.zeros((3, 4, 128)), np.zeros((3, 5))), (np.zeros((3, 128)), np.zeros(3))):
        with pytest.raises(ValueError):
            dropin.find_loop_candidates(*args)
    with pytest.raises(ValueError):
        dropin.find_loop_candidates(np.zeros((3, 4, 128)), np.zeros((3, 4)), min_gap=0)
