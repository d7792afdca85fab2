"""The cases of tests/test_gpu_graph_limits.py: libsslam_graph.so and libsslam_loop.so at the limits their headers state
(tests/graph_table.py, tests/loop_table.py: every size below is read from the tables' `largest`) and with operands past 2^31
bytes, each with the restatement's expectation (tests/pose_graph_ref.py, tests/loop_ref.py) and, for the far end, one changed
input element of the last graph, chain, frame or slot with the restatement's new result.  tests/test_graph_limit_cases_cpu.py
holds every case to what its name says.

An operand past 2^31 bytes is periodic as in tests/periodic.py - 7 repeating items and items of their own at 0, at the holder of
byte 2^31 and at the end: only the P + len(marked) distinct items exist here, the device test expands them.  marks() and slots()
restate periodic.marks and periodic.slots without torch (the CPU test holds them equal).

Builders are cached per process: the big ones take seconds.  Case generation uses np.linalg and random numbers freely: nothing
here is what the device computes.  No torch, no GPU: importable anywhere."""
from __future__ import annotations

import functools

import numpy as np

import graph_table as gt
import loop_cases as lc
import loop_ref as lr
import loop_table as lt
import pose_graph_cases as pc
import pose_graph_ref as pg

P = 7
FAR = 1 << 31
GRAPH_OPERANDS = ("first", "second", "T", "info", "C_in")


def marks(n, frame_bytes):
    m = {0, n - 1}
    if FAR < n * frame_bytes:
        m.add(FAR // frame_bytes)
    return sorted(m)


def slots(n, marked):
    s = np.arange(n, dtype=np.int64) % P
    s[np.asarray(marked, np.int64)] = P + np.arange(len(marked))
    return s


def _rigid(rng, count, angle, step):
    """count rigid transforms (count, 12): rotations of about `angle` radians, translations of about `step`."""
    return np.stack([pc.pose12(pc.so3(angle * rng.standard_normal(3)), step * rng.standard_normal(3)) for _ in range(count)])


def _xi(rng):
    return np.concatenate([0.01 * rng.standard_normal(3), 0.004 * rng.standard_normal(3)])


# ------------------------------------------------------------------------------------------------------------------- chains
@functools.lru_cache(maxsize=None)
def chains_at_the_count_limit_past_2_31():
    """The most chains the entry takes, of 3 nodes, with C_start: C is 2.42 GB, T 1.61 GB.  The marks are C's."""
    n, n_nodes = gt.LIMITS["sslg_chain_poses"]["largest"]["n_graphs"], 3
    frame_bytes = n_nodes * 12 * 8
    marked = marks(n, frame_bytes)
    d = P + len(marked)
    rng = np.random.default_rng(101)
    T, start = _rigid(rng, d * (n_nodes - 1), 0.3, 0.5).reshape(d, n_nodes - 1, 12), _rigid(rng, d, 0.5, 2.0)
    T_far = T[-1].copy()
    T_far[-1, 11] += 0.5                                             # the last element of the whole operand
    return dict(name="chains_at_the_count_limit_past_2_31", n=n, n_nodes=n_nodes, frame_bytes=frame_bytes, marked=marked, T=T, start=start,
                want=np.stack([pg.chain(T[i], start[i]) for i in range(d)]), T_far=T_far, want_far=pg.chain(T_far, start[-1]))


@functools.lru_cache(maxsize=None)
def chains_at_the_node_limit():
    """The most nodes, 257 chains (one thread past a workgroup), chain i the distinct chain i % 3, from [I | 0]."""
    n_nodes, n, d = gt.LIMITS["sslg_chain_poses"]["largest"]["n_nodes"], 257, 3
    T = _rigid(np.random.default_rng(102), d * (n_nodes - 1), 0.02, 0.05).reshape(d, n_nodes - 1, 12)
    return dict(name="chains_at_the_node_limit", n=n, n_nodes=n_nodes, T=T, slot=np.arange(n) % d, want=np.stack([pg.chain(T[i]) for i in range(d)]))


# ------------------------------------------------------------------------------------------------------------------- banded
def with_far_slot(c):
    """The case with the T of its far slot replaced: the far end's operands."""
    out = dict(c, T=c["T"].copy())
    out["T"][c["far_slot"]] = c["T_far"]
    return out


def run_banded(c, n_iter=None):
    return pg.optimize(c["first"], c["second"], c["T"], c["info"], c["C_in"], c["band"], c["chi"], c["damping"], c["n_iter"] if n_iter is None else n_iter)


def run_sparse(c, n_iter=None):
    return lr.optimize(c["first"], c["second"], c["T"], c["info"], c["C_in"], c["chi"], c["damping"], c["n_iter"] if n_iter is None else n_iter,
                       c["cg_iterations"], c["cg_tol"])


@functools.lru_cache(maxsize=None)
def banded_at_the_node_and_band_limit():
    """4096 nodes, band 32, spacings (1, 16, 32): 24 570 rows, the 198-row window slides 24 372 times; one iteration.  The far slot
    is the last, the edge (4063, 4095)."""
    L = gt.LIMITS["sslg_pose_graph"]["largest"]
    c = pc.graph_case("banded_at_the_node_and_band_limit", L["n_nodes"], (1, 16, 32), L["band"], 42, n_iter=1)
    far = len(c["first"]) - 1
    return dict(c, far_slot=far, T_far=pc.perturb(c["T"][far], 5.0 * _xi(np.random.default_rng(103))))


@functools.lru_cache(maxsize=None)
def banded_at_the_slot_limit():
    """1 048 576 slots, 40 nodes, band 20, one graph: the 149 planted edges scattered over the slot range in their order (slots 0,
    255, 256 and the last among them), 60 more measurements of planted edges (duplicates), 400 skipped slots of five kinds - each
    with a real measurement that would count if it were used - and the rest absent, some of those with NaN in T and info."""
    E = gt.LIMITS["sslg_pose_graph"]["largest"]["n_edges"]
    base = pc.graph_case("banded_at_the_slot_limit", 40, pc.SPACINGS, 20, 43, n_iter=3, outliers=0.03)
    n0 = len(base["first"])
    rng = np.random.default_rng(104)
    fixed = [0, 255, 256, E - 1]
    free = rng.permutation(np.setdiff1d(np.arange(E), fixed))[:n0 - 4 + 60 + 400 + 40]
    where = np.sort(np.concatenate([fixed, free[:n0 - 4]]))
    dup_at, skip_at, nan_at = free[n0 - 4:n0 + 56], free[n0 + 56:n0 + 456], free[n0 + 456:]
    first, second = np.full(E, -1, np.int32), np.full(E, -1, np.int32)
    T, info = np.zeros((E, 12)), np.zeros((E, 21))
    first[where], second[where], T[where], info[where] = base["first"], base["second"], base["T"], base["info"]
    again = rng.integers(0, n0, len(dup_at) + len(skip_at))
    pairs = list(zip(base["first"][again].tolist(), base["second"][again].tolist()))
    Tm, im = lc.measure(base["truth"], pairs, rng)
    at = np.concatenate([dup_at, skip_at])
    first[at], second[at], T[at], info[at] = base["first"][again], base["second"][again], Tm, im
    kinds = np.array_split(skip_at, 5)
    T[kinds[0], 5] = np.nan                                          # a non-finite T
    info[kinds[1], 20] = np.inf                                      # a non-finite info
    second[kinds[2]] = first[kinds[2]]                               # a = b
    first[kinds[3]], second[kinds[3]] = second[kinds[3]], first[kinds[3]]      # a > b
    first[kinds[4]], second[kinds[4]] = 0, 25                        # past the band
    T[nan_at], info[nan_at] = np.nan, np.nan                         # absent: never read
    return dict(base, first=first, second=second, T=T, info=info, planted_at=where, duplicates_at=dup_at, skipped_at=skip_at, far_slot=E - 1,
                T_far=pc.perturb(base["T"][-1], 5.0 * _xi(rng)))


# ------------------------------------------------------------------------------------------ many small graphs, both solvers
SMALL_NODES, SMALL_SLOTS, SMALL_BAND = 4, 200, 3
NOT_ATTEMPTED, FAILED_PIVOT = 2, 4          # the distinct graphs (of the 7 repeating ones) with NaN in C_in; with node 2 named by no edge


def _graphs(n, n_nodes, edges, n_free, frame_bytes, seed):
    """The distinct graphs of an n-graph launch marked by frame_bytes: per graph the edges measured on a path of its own, the start
    the spacing-1 chain, and among the first n_free slots five absent ones, three with a NaN in T and two with a = b.  One repeating
    graph is not attempted, one fails its first pivot at row 6.  Row d is the last graph with the T of its last slot changed."""
    marked = marks(n, frame_bytes)
    d = P + len(marked)
    ops = {k: [] for k in GRAPH_OPERANDS}
    for g in range(d):
        rng = np.random.default_rng(seed + g)
        T, info = lc.measure(pc.path(n_nodes, seed + g), edges, rng)
        first, second = np.array([a for a, _ in edges], np.int32), np.array([b for _, b in edges], np.int32)
        C_in = pg.chain(T[:n_nodes - 1])
        odd = rng.permutation(np.arange(n_nodes - 1, n_free))[:10]
        first[odd[:5]] = -1
        T[odd[5:8], rng.integers(0, 12)] = np.nan
        second[odd[8:]] = first[odd[8:]]
        if g == NOT_ATTEMPTED:
            C_in[3, 7] = np.nan
        if g == FAILED_PIVOT:
            first[(first == 2) | (second == 2)] = -1
        for k, v in zip(GRAPH_OPERANDS, (first, second, T, info, C_in)):
            ops[k].append(v)
    for k in GRAPH_OPERANDS:                                         # row d: the last graph, changed
        ops[k].append(ops[k][d - 1].copy())
    ops["T"][d][len(edges) - 1] = pc.perturb(ops["T"][d][len(edges) - 1], 5.0 * _xi(np.random.default_rng(seed - 1)))
    return dict({k: np.stack(v) for k, v in ops.items()}, n=n, n_nodes=n_nodes, n_edges=len(edges), frame_bytes=frame_bytes, marked=marked)


@functools.lru_cache(maxsize=None)
def small_graphs():
    """The distinct graphs of the two graph-limit cases: 65 535 graphs of 4 nodes and 200 slots - 33 measurements of each of the six
    edges, an absent slot, a last used slot (2, 3).  edge_info is 2.20 GB: the marks are its."""
    n = gt.LIMITS["sslg_pose_graph"]["largest"]["n_graphs"]
    assert n == lt.LIMITS["ssll_pose_graph_sparse"]["largest"]["n_graphs"]
    edges = pc.edge_list(SMALL_NODES, (1, 2, 3)) * 33 + [(0, 1), (2, 3)]
    assert len(edges) == SMALL_SLOTS
    c = _graphs(n, SMALL_NODES, edges, 198, SMALL_SLOTS * 21 * 8, 105)
    c["first"][:, 198] = -1
    return dict(c, band=SMALL_BAND, chi=4.0, damping=0.0, n_iter=4, cg_iterations=64, cg_tol=1e-3)


@functools.lru_cache(maxsize=None)
def banded_at_the_graph_limit_past_2_31():
    c = small_graphs()
    want = pg.optimize_graphs(c["first"], c["second"], c["T"], c["info"], c["C_in"], c["band"], c["chi"], c["damping"], c["n_iter"])
    return dict(c, name="banded_at_the_graph_limit_past_2_31", workspace_bytes=gt.workspace_bytes(c["n"], c["n_nodes"], c["band"]), want=want)


@functools.lru_cache(maxsize=None)
def sparse_at_the_graph_limit_past_2_31():
    c = small_graphs()
    want = lr.optimize_graphs(c["first"], c["second"], c["T"], c["info"], c["C_in"], c["chi"], c["damping"], c["n_iter"], c["cg_iterations"], c["cg_tol"])
    return dict(c, name="sparse_at_the_graph_limit_past_2_31", workspace_bytes=lt.sparse_workspace_bytes(c["n"], c["n_nodes"], c["n_edges"]), want=want)


WIDE_NODES, WIDE_BAND = 20, 19


@functools.lru_cache(maxsize=None)
def banded_workspace_past_2_31_words():
    """Beside the issue's cases: in those no ELEMENT index leaves 31 bits (65 535 * 200 * 21 = 2.8e8, 65 535 * 23 574 workspace words
    = 1.5e9), only byte addresses do.  65 535 graphs of 20 nodes at band 19 take 37 302 workspace words each, 2.44e9 words in all:
    graph * workspace words itself passes 2^31 (the row `graph * workspace doubles 64` of the table).  33 edges at spacings 1, 7
    and 19 and 7 second measurements: 40 slots.  The marks count workspace WORDS: graph 57 571 holds word 2^31."""
    n = gt.LIMITS["sslg_pose_graph"]["largest"]["n_graphs"]
    edges = pc.edge_list(WIDE_NODES, (1, 7, 19))
    edges = edges + edges[19:26]
    words = gt.workspace_bytes(1, WIDE_NODES, WIDE_BAND) // 8
    c = dict(_graphs(n, WIDE_NODES, edges, len(edges) - 1, words, 112), band=WIDE_BAND, chi=4.0, damping=0.0, n_iter=2)
    want = pg.optimize_graphs(c["first"], c["second"], c["T"], c["info"], c["C_in"], c["band"], c["chi"], c["damping"], c["n_iter"])
    return dict(c, name="banded_workspace_past_2_31_words", workspace_words=words, workspace_bytes=gt.workspace_bytes(n, WIDE_NODES, WIDE_BAND), want=want)


# ------------------------------------------------------------------------------------------------------------------- sparse
@functools.lru_cache(maxsize=None)
def sparse_at_the_node_and_slot_limit():
    """4096 nodes, every spacing 1 .. 16 and 40 loop edges (a, a + 4000): 65 440 slots, padded to the 65 536 the entry takes with
    an absent slot, a non-finite one, an a = b one, one out of range and 92 second measurements of the first edges; the last slot
    is used.  Two iterations of 30 CG steps."""
    L = lt.LIMITS["ssll_pose_graph_sparse"]["largest"]
    c = lc.with_loops(L["n_nodes"], tuple(range(1, 17)), 45, [(a, a + 4000) for a in range(40)], name="sparse_at_the_node_and_slot_limit", n_iter=2,
                      cg_iterations=30)
    E0, E = len(c["first"]), L["n_edges"]
    assert E0 == 65440
    rng = np.random.default_rng(106)
    dup = np.arange(E - E0)
    c["first"], c["second"] = np.concatenate([c["first"], c["first"][dup]]), np.concatenate([c["second"], c["second"][dup]])
    c["T"] = np.concatenate([c["T"], np.stack([pc.perturb(c["T"][e], _xi(rng)) for e in dup])])
    c["info"] = np.concatenate([c["info"], c["info"][dup]])
    c["first"][E0] = -1
    c["T"][E0 + 1, 4] = np.nan
    c["second"][E0 + 2] = c["first"][E0 + 2]
    c["second"][E0 + 3] = L["n_nodes"]
    c.update(padding=(E0, E), far_slot=E - 1, T_far=pc.perturb(c["T"][E - 1], 5.0 * _xi(rng)))
    return c


FULL_ITERATIONS_DAMPING = 1e4       # chosen on the CPU: with it the restatement accepts all 16 steps of twelve_nodes_two_loops


def _twelve_nodes():
    return lc.with_loops(12, (1, 2), 23, [(0, 11), (2, 9)], name="twelve_nodes_two_loops")


@functools.lru_cache(maxsize=None)
def sparse_at_the_iteration_limit():
    L = lt.LIMITS["ssll_pose_graph_sparse"]["largest"]
    assert lt.MAX_ITER == lr.MAX_ITER
    return dict(_twelve_nodes(), name="sparse_at_the_iteration_limit", n_iter=lt.MAX_ITER, damping=FULL_ITERATIONS_DAMPING, cg_iterations=L["cg_iterations"] // 8)


@functools.lru_cache(maxsize=None)
def sparse_at_the_cg_limit():
    """cg_iterations at its limit, cg_tol 0, one step.  `cg_ended` records how the restatement's CG loop ended: "count" (all
    cg_iterations taken), "pq" (p . A p no longer positive and finite) or "tol" (r . z reached +0.0 exactly)."""
    c = dict(_twelve_nodes(), name="sparse_at_the_cg_limit", n_iter=1, cg_tol=0.0, cg_iterations=lt.LIMITS["ssll_pose_graph_sparse"]["largest"]["cg_iterations"])
    G = lr.SparseGraph(c["first"], c["second"], c["T"], c["info"], len(c["C_in"]))
    D, g, BA = G.blocks(c["C_in"], c["chi"], c["damping"])
    f, fail = lr.block_ldl(D)
    assert fail < 0
    _, steps, ended = lr.pcg_trace(G, D, g, BA, f, c["cg_iterations"], c["cg_tol"])
    return dict(c, cg_ended=ended, cg_first=steps)


# --------------------------------------------------------------------------------------------------------------- signatures
def _signature_case(name, n, k, d, seed):
    frame_bytes = k * d * 4
    marked = marks(n, frame_bytes)
    desc, scores = lc.bank(P + len(marked), k, d, seed)
    raw = lr.raw_signatures(desc, scores)[slots(n, marked)]
    far = desc[-1].copy()
    far[k - 1, d - 1] += np.float32(0.5)                             # the last float of the whole operand
    raw_far = raw.copy()
    raw_far[n - 1] = lr.raw_signatures(far[None], scores[-1:])[0]
    return dict(name=name, n=n, k=k, d=d, frame_bytes=frame_bytes, marked=marked, desc=desc, scores=scores, want=lr.finish_signatures(raw),
                desc_far=far, want_far=lr.finish_signatures(raw_far))


@functools.lru_cache(maxsize=None)
def signatures_at_the_frame_limit_past_2_31():
    L = lt.LIMITS["ssll_frame_signatures"]["largest"]
    return _signature_case("signatures_at_the_frame_limit_past_2_31", L["n_frames"], 520, L["d"], 109)


@functools.lru_cache(maxsize=None)
def signatures_at_the_keypoint_limit_past_2_31():
    return _signature_case("signatures_at_the_keypoint_limit_past_2_31", 1030, lt.LIMITS["ssll_frame_signatures"]["largest"]["k"], 128, 110)


# --------------------------------------------------------------------------------------------------------------- candidates
CANDIDATE_PERIOD, LATE_PLACES, LATE_FIRST, LATE_AGAIN = 187, 6, 3850, 4050


@functools.lru_cache(maxsize=None)
def candidates_at_the_frame_limit():
    """4096 frames of 198 distinct unit rows: frame i shows row i % 187 - exact duplicates, so exact ties, all over the range -
    except that six places are seen late and only twice, at frames 3850 .. 3855 and again at 4050 .. 4055 (a pick in the
    workgroup's last stride), and that frames 0, 255, 256, 4094 and 4095 have rows of their own.  S_ij is a function of the two
    rows alone: the similarity of the distinct rows, expanded, is the whole matrix, exactly."""
    L = lt.LIMITS["ssll_loop_candidates"]["largest"]
    n, d, own = L["n_frames"], L["d"], [0, 255, 256, L["n_frames"] - 2, L["n_frames"] - 1]
    rows = lc.place_signatures(CANDIDATE_PERIOD + LATE_PLACES + len(own), d, 111, 23)
    slot = np.arange(n) % CANDIDATE_PERIOD
    for start in (LATE_FIRST, LATE_AGAIN):
        slot[start:start + LATE_PLACES] = CANDIDATE_PERIOD + np.arange(LATE_PLACES)
    slot[own] = CANDIDATE_PERIOD + LATE_PLACES + np.arange(len(own))
    S = lr.similarity(rows)[slot][:, slot]
    c = lc.candidate_case("candidates_at_the_frame_limit", np.ascontiguousarray(rows[slot]), 30, 0.3, L["per_frame"], 5)
    return dict(c, n=n, d=d, rows=rows, slot=slot, S=S, want=lr.candidates(None, c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"], S=S))
