#!/usr/bin/env python3
"""The loop-closure launches (libsslam_loop.so) beside the launches they stand next to, on the workload of tools/pose_graph_probe.py:
613 synthetic frames at K = 500 (G = 28), the five spacings 1, 5, 10, 15, 20 (3014 pairs; 32 extracted synthetic frames repeated,
the depth of a synthetic 640 x 480 scene), all in one process:

  similarity 612      sslam_sim_argmax_pairs on the 612 spacing-1 pairs (through lib.sim_argmax_pairs, which allocates its outputs)
  signatures          ssll_frame_signatures over the 613 frames: two launches
  candidates          ssll_loop_candidates over the 613 signatures: min_gap 30, min_sim 0.3, per_frame 2, suppress 5
  banded N            sslg_pose_graph over the 3014 refined poses, 613 nodes, band 20, chi 4, N steps at most, from the chain
  sparse N            ssll_pose_graph_sparse on the SAME edge list and start, cg_iterations 512, cg_tol 1e-3
  sparse+loops N      the same with the verified candidate slots behind the 3014 (one RANSAC and one refinement launch over them)

Both graph launches are ONE 256-thread workgroup: latencies, not throughputs.  The bank repeats 32 frames, so every frame 32 k
back is the same frame: the candidates are exact revisits, and the loop edges say that frames 32 k apart coincide - which the
odometry edges of a sliding window do not say.  The costs and steps printed show how much work each launch had, nothing else.

Protocol: that of tools/pose_graph_probe.py - calls on preallocated buffers, timed with device events; every variant warmed, then
`repeats` rounds taken ALTERNATELY, one block of `reps` back-to-back calls of every variant per round between two events on the
stream; printed: median and min - max of the per-call time over the rounds, in microseconds, and the ratios.
    tools/loop_probe.py [--repeats 7] [--out FILE]      (profiles/loop_closure.txt holds the output below the planted study's lines)"""
import ctypes as C
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import synth
from sslam_amd import evaluation, lib
from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline

args, repeats, out_path = sys.argv[1:], 7, None
while args:
    if args[0] == "--repeats" and len(args) > 1:
        repeats = int(args[1])
    elif args[0] == "--out" and len(args) > 1:
        out_path = args[1]
    else:
        raise SystemExit(__doc__)
    args = args[2:]
assert torch.cuda.is_available(), "this probe measures on the GPU only"

N_EXTRACT, N_SEQ, THRESHOLD, SEED = 32, 613, 12.0, 1
HYPOTHESES, HUBER, SPACINGS, BAND, CHI, GRAPH_ITER = 256, 4.0, (1, 5, 10, 15, 20), 20, 4.0, (1, 8)
LOOPS = dict(min_gap=30, min_sim=0.3, per_frame=2, suppress=5, min_inliers=12)
CG_ITER, CG_TOL = 512, 1e-3
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def ab_events(row, calls, reps):
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {v: [] for v in calls}
    for _ in range(repeats):
        for v, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[v].append(e0.elapsed_time(e1) / reps * 1e3)
    for v in calls:
        emit(f"{row:8s} {v:16s} median {statistics.median(us[v]):9.1f} us   min {min(us[v]):9.1f}   max {max(us[v]):9.1f}   "
             f"({reps} calls x {repeats} rounds)")
    return {v: statistics.median(x) for v, x in us.items()}


def scene_depth(n, h=480, w=640):
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w), np.uint16)
    for f in range(n):
        steps = rng.integers(0, 1500, (h // 32 + 1, w // 32 + 1))[yy // 32, xx // 32]
        out[f] = (7500 + 10 * f + 8.0 * xx + 4.0 * yy + steps).astype(np.uint16)
        out[f, 100 + 5 * f:120 + 5 * f] = 0
    return out


emit(f"# loop-closure launches, 613 frames, K 500, spacings {SPACINGS}; us per call, all measured; {torch.cuda.get_device_name(0)}")
cam = evaluation.Camera()
with torch.no_grad():
    grid, K = 28, 500
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * grid, num_keypoints=K), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    ex = pipe.extract(torch.from_numpy(synth.token_sequence(N_EXTRACT, grid)).cuda(), None)
    idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
    desc, scores, kp = (ex[k][idx].contiguous() for k in ("descriptors", "scores", "keypoints_pixel"))
    D = int(desc.shape[2])
    pairs = [(i, i + s) for s in SPACINGS for i in range(N_SEQ - s)]
    P = len(pairs)
    first = torch.tensor([a for a, _ in pairs], dtype=torch.int32, device="cuda")
    second = torch.tensor([b for _, b in pairs], dtype=torch.int32, device="cuda")
    depth = torch.from_numpy(scene_depth(N_EXTRACT)).cuda()
    kd = torch.full((N_SEQ, K), -1, dtype=torch.int32, device="cuda")
    for a in range(0, N_SEQ, N_EXTRACT):                 # the whole bank's depths, from the 32 scene frames it repeats
        b = min(a + N_EXTRACT, N_SEQ)
        pipe.keypoint_depth(depth[:b - a], kp[a:b], out=kd[a:b])
    rule = MatchRule.mnn_ratio(0.9)
    kw = dict(threshold=THRESHOLD, hypotheses=HYPOTHESES, seed=SEED)

    G, Lp = lib.graph(), lib.loop()
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    dbl = C.c_double
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- retrieval beside the similarity launch
    sig = torch.zeros((N_SEQ, D), device="cuda")
    sws = torch.empty(4 * N_SEQ * D, dtype=torch.uint8, device="cuda")
    cshapes = lib.loop_candidate_shapes(N_SEQ, LOOPS["per_frame"])
    cand = {k: torch.zeros(cshapes[k][0], dtype=cshapes[k][1], device="cuda") for k in lib.LOOP_CANDIDATE_KEYS}
    simws = pipe.workspace(0, N_SEQ - 1)

    def similarity():
        lib.sim_argmax_pairs(desc, first[:N_SEQ - 1], second[:N_SEQ - 1], workspace=simws)

    def signatures():
        assert Lp.ssll_frame_signatures(ptr(desc), ptr(scores), N_SEQ, K, D, ptr(sws), ptr(sig), stream) == 0

    def candidates():
        assert Lp.ssll_loop_candidates(ptr(sig), N_SEQ, D, LOOPS["min_gap"], C.c_float(LOOPS["min_sim"]), LOOPS["per_frame"], LOOPS["suppress"],
                                       *(ptr(cand[k]) for k in lib.LOOP_CANDIDATE_KEYS), stream) == 0

    signatures(), candidates()
    torch.cuda.synchronize()
    via = pipe.find_loop_candidates(desc, scores, LOOPS["min_gap"], LOOPS["min_sim"], LOOPS["per_frame"], LOOPS["suppress"])
    assert all(torch.equal(cand[k].view(torch.int32), via[k].view(torch.int32)) for k in lib.LOOP_CANDIDATE_KEYS), "the raw calls are the pipeline's"
    med = ab_events(f"K {K}", {"similarity 612": similarity, "signatures": signatures, "candidates": candidates}, 10)
    n_cand = int(cand["count"].sum())
    emit(f"# K {K}: {n_cand} candidates in {N_SEQ * LOOPS['per_frame']} slots; of them {int(((cand['second'] - cand['first']) % N_EXTRACT == 0)[cand['first'] >= 0].sum())} "
         f"name the same extracted frame (the bank repeats {N_EXTRACT})")
    emit(f"# K {K}: signatures / similarity 612 = {med['signatures'] / med['similarity 612']:.3f}; candidates / similarity 612 = "
         f"{med['candidates'] / med['similarity 612']:.3f}")

    # ---- the edges: the spacings' pairs, then the candidate slots, verified in one RANSAC and one refinement launch
    all_first, all_second = torch.cat([first, cand["first"]]), torch.cat([second, cand["second"]])
    E = int(all_first.shape[0])
    m = pipe.match_pairs(desc, scores, first=all_first, second=all_second, rule=rule)
    est = pipe.estimate_poses(kp, kd, all_first, all_second, m, cam, **kw)
    refined = pipe.refine_poses(kp, kd, all_first, all_second, m, cam, est, THRESHOLD, HUBER, 5)
    status = refined["status"]
    kept = (cand["first"] >= 0) & (status[P:] != lib.REFINE_NOT_ATTEMPTED) & (refined["inlier_count"][P:] >= LOOPS["min_inliers"])
    absent = torch.full_like(all_first, -1)
    odo_first = torch.where(status[:P] == lib.REFINE_NOT_ATTEMPTED, absent[:P], first).contiguous()
    loop_first = torch.cat([odo_first, torch.where(kept, cand["first"], absent[P:])]).contiguous()
    T_odo, info_odo = refined["T"][:P].contiguous(), refined["info"][:P].contiguous()
    chained = lib.chain_poses(refined["T"][:N_SEQ - 1].contiguous(), N_SEQ)

    def outputs(shapes, keys):
        return {n: {key: torch.zeros(shapes[key][0], dtype=shapes[key][1], device="cuda") for key in keys} for n in GRAPH_ITER}
    banded_out = outputs(lib.pose_graph_shapes(1, N_SEQ, P), lib.POSE_GRAPH_KEYS)
    sparse_out = outputs(lib.pose_graph_sparse_shapes(1, N_SEQ, P), lib.POSE_GRAPH_SPARSE_KEYS)
    loops_out = outputs(lib.pose_graph_sparse_shapes(1, N_SEQ, E), lib.POSE_GRAPH_SPARSE_KEYS)
    bws = torch.empty(lib.pose_graph_workspace_bytes(1, N_SEQ, BAND), dtype=torch.uint8, device="cuda")
    sws2 = torch.empty(lib.pose_graph_sparse_workspace_bytes(1, N_SEQ, E), dtype=torch.uint8, device="cuda")

    def banded(n_iter):
        o = banded_out[n_iter]
        return lambda: G.sslg_pose_graph(ptr(odo_first), ptr(second), ptr(T_odo), ptr(info_odo), 1, N_SEQ, P, ptr(chained), BAND, dbl(CHI), dbl(0.0),
                                         n_iter, ptr(bws), *(ptr(o[key]) for key in lib.POSE_GRAPH_KEYS), stream)

    def sparse(n_iter, o, f, s, Tm, info, n_edges):
        return lambda: Lp.ssll_pose_graph_sparse(ptr(f), ptr(s), ptr(Tm), ptr(info), 1, N_SEQ, n_edges, ptr(chained), dbl(CHI), dbl(0.0), n_iter,
                                                 CG_ITER, dbl(CG_TOL), ptr(sws2), *(ptr(o[n_iter][key]) for key in lib.POSE_GRAPH_SPARSE_KEYS), stream)
    calls = {}
    for n in GRAPH_ITER:
        calls[f"banded {n}"] = banded(n)
        calls[f"sparse {n}"] = sparse(n, sparse_out, odo_first, second, T_odo, info_odo, P)
        calls[f"sparse+loops {n}"] = sparse(n, loops_out, loop_first, all_second, refined["T"], refined["info"], E)
    for fn in calls.values():
        assert fn() == 0
    torch.cuda.synchronize()
    med = ab_events(f"K {K}", calls, 2)

    def said(o):
        return (f"status {int(o['status'][0])}, accepted steps {int(o['iterations'][0])}, used edges {int(o['used_edges'][0])}, skipped "
                f"{int(o['skipped_edges'][0])}, failed_row {int(o['failed_row'][0])}, cost {float(o['cost_in'][0]):.6g} -> {float(o['cost'][0]):.6g}")
    emit(f"# K {K}: {P} pairs and {N_SEQ * LOOPS['per_frame']} candidate slots, {int(kept.sum())} of them kept (refinement attempted, at least "
         f"{LOOPS['min_inliers']} inliers); cg_iterations {CG_ITER}, cg_tol {CG_TOL}")
    for n in GRAPH_ITER:
        emit(f"# K {K}: banded {n}: {said(banded_out[n])}")
        emit(f"# K {K}: sparse {n}: {said(sparse_out[n])}; cg_steps {sparse_out[n]['cg_steps'][0].tolist()}")
        emit(f"# K {K}: sparse+loops {n}: {said(loops_out[n])}; cg_steps {loops_out[n]['cg_steps'][0].tolist()}")
    dC = float((sparse_out[8]["C"] - banded_out[8]["C"]).abs().max())
    emit(f"# K {K}: largest |C sparse 8 - C banded 8| over the 613 poses' entries: {dC:.3g}")
    for n in GRAPH_ITER:
        acc = {v: max(1, int(o[n]["iterations"][0])) for v, o in (("banded", banded_out), ("sparse", sparse_out), ("sparse+loops", loops_out))}
        emit(f"# K {K}: at most {n} steps, per accepted step: banded {med[f'banded {n}'] / acc['banded']:.1f} us, sparse {med[f'sparse {n}'] / acc['sparse']:.1f} us, "
             f"sparse+loops {med[f'sparse+loops {n}'] / acc['sparse+loops']:.1f} us; sparse {n} / banded {n} = {med[f'sparse {n}'] / med[f'banded {n}']:.3f}; "
             f"sparse+loops {n} / banded {n} = {med[f'sparse+loops {n}'] / med[f'banded {n}']:.3f}")
    emit("# one 256-thread workgroup each: latency figures, not throughput ones")

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
