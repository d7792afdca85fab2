#!/usr/bin/env python3
"""The pose-graph launch (sslg_pose_graph, libsslam_graph.so) beside the RANSAC and refinement launches that feed it, on the
613-frame synthetic workload of tools/pose_refine_probe.py at K = 500 (G = 28) and the five spacings 1, 5, 10, 15, 20 (3014 pairs;
32 extracted synthetic frames repeated, the depth of a synthetic 640 x 480 scene), all in one process:

  ransac 256      sslam_pose_ransac_pairs on the M4 lists of all 3014 pairs, 256 hypotheses, threshold 12 keypoint units
  refine 5        sslam_pose_refine_pairs from RANSAC's poses on the same lists, threshold 12, huber 4, 5 steps at most
  chain           sslg_chain_poses over the 612 refined spacing-1 poses
  graph N         sslg_pose_graph over the 3014 refined poses and information matrices, 613 nodes, band 20, chi 4, N steps at most

The graph launch is ONE 256-thread workgroup: the figure is a latency, not a throughput - 255 of the 256 compute units idle.
On synthetic frames the poses mean nothing as accuracy: the tokens slide over a random field, no camera moves through a scene.
The probe times the launch; the accepted steps and the status it prints say how much work the launch had, nothing else.

Protocol: that of tools/pose_refine_probe.py - raw C-ABI calls on preallocated buffers, timed with device events; every variant
warmed, then `repeats` rounds taken ALTERNATELY, one block of `reps` back-to-back calls of every variant per round between two
events on the stream; printed: median and min - max of the per-call time over the rounds, in microseconds, and the ratios.
    tools/pose_graph_probe.py [--repeats 7] [--out FILE]      (profiles/pose_graph.txt holds the output below the planted study's lines)"""
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
        emit(f"{row:8s} {v:14s} median {statistics.median(us[v]):9.1f} us   min {min(us[v]):9.1f}   max {max(us[v]):9.1f}   "
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


emit(f"# pose-graph launch beside the RANSAC and refinement launches, 613 frames, spacings {SPACINGS}; us per call, all measured; "
     f"{torch.cuda.get_device_name(0)}")
cam = evaluation.Camera()
with torch.no_grad():
    grid, K, reps = 28, 500, 3
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * grid, num_keypoints=K), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    ex = pipe.extract(torch.from_numpy(synth.token_sequence(N_EXTRACT, grid)).cuda(), None)
    idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
    desc, scores, kp = (ex[k][idx].contiguous() for k in ("descriptors", "scores", "keypoints_pixel"))
    pairs = [(i, i + s) for s in SPACINGS for i in range(N_SEQ - s)]
    P = len(pairs)
    first = torch.tensor([a for a, _ in pairs], dtype=torch.int32, device="cuda")
    second = torch.tensor([b for _, b in pairs], dtype=torch.int32, device="cuda")
    depth = torch.from_numpy(scene_depth(N_EXTRACT)).cuda()
    sx, sy = pipe.depth_scales(cam)
    kd = torch.full((N_SEQ, K), -1, dtype=torch.int32, device="cuda")
    for a in range(0, N_SEQ, N_EXTRACT):                 # the whole bank's depths, from the 32 scene frames it repeats
        b = min(a + N_EXTRACT, N_SEQ)
        pipe.keypoint_depth(depth[:b - a], kp[a:b], out=kd[a:b])

    L, G = lib.lib(), lib.graph()
    m = pipe.match_pairs(desc, scores, first=first, second=second, rule=MatchRule.mnn_ratio(0.9))
    pose, refined = pipe.alloc_pose(P, K), pipe.alloc_pose_refine(P, K)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    dbl = C.c_double
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    camera = (dbl(cam.fx), dbl(cam.fy), dbl(cam.cx), dbl(cam.cy), dbl(cam.depth_scale), dbl(sx), dbl(sy), dbl(cam.width), dbl(cam.height),
              dbl(THRESHOLD))
    shapes = lib.pose_graph_shapes(1, N_SEQ, P)
    outs = {n: {key: torch.zeros(shapes[key][0], dtype=shapes[key][1], device="cuda") for key in lib.POSE_GRAPH_KEYS} for n in GRAPH_ITER}
    ws = torch.empty(lib.pose_graph_workspace_bytes(1, N_SEQ, BAND), dtype=torch.uint8, device="cuda")
    chained = torch.zeros((1, N_SEQ, 12), dtype=torch.float64, device="cuda")
    edge_first = torch.empty_like(first)

    def ransac():
        assert L.sslam_pose_ransac_pairs(ptr(kp), ptr(kd), N_SEQ, K, ptr(first), ptr(second), P, ptr(m["matches"]), ptr(m["match_count"]),
                                         K, *camera, HYPOTHESES, C.c_uint64(SEED), *(ptr(pose[key]) for key in lib.POSE_RANSAC_KEYS),
                                         stream) == 0

    def refine():
        assert L.sslam_pose_refine_pairs(ptr(kp), ptr(kd), N_SEQ, K, ptr(first), ptr(second), P, ptr(m["matches"]), ptr(m["match_count"]),
                                         K, *camera, ptr(pose["T"]), dbl(HUBER), 5, *(ptr(refined[key]) for key in lib.POSE_REFINE_KEYS),
                                         stream) == 0

    def chain():
        assert G.sslg_chain_poses(ptr(refined["T"]), None, 1, N_SEQ, ptr(chained), stream) == 0

    def graph(n_iter):
        o = outs[n_iter]

        def call():
            assert G.sslg_pose_graph(ptr(edge_first), ptr(second), ptr(refined["T"]), ptr(refined["info"]), 1, N_SEQ, P, ptr(chained), BAND,
                                     dbl(CHI), dbl(0.0), n_iter, ptr(ws), *(ptr(o[key]) for key in lib.POSE_GRAPH_KEYS), stream) == 0
        return call

    ransac(), refine(), chain()
    edge_first.copy_(torch.where(refined["status"] == lib.REFINE_NOT_ATTEMPTED, torch.full_like(first, -1), first))
    calls = {"ransac 256": ransac, "refine 5": refine, "chain": chain}
    calls.update({f"graph {n}": graph(n) for n in GRAPH_ITER})
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ps = pipe.optimize_pose_graph(first, second, refined, refined, N_SEQ, band=BAND, huber_chi=CHI, iterations=GRAPH_ITER[-1])
    assert all(torch.equal(outs[GRAPH_ITER[-1]][key][0].view(torch.int64) if ps[key].dtype == torch.float64 else outs[GRAPH_ITER[-1]][key][0],
                           ps[key].view(torch.int64) if ps[key].dtype == torch.float64 else ps[key]) for key in ps), \
        "the raw call is the pipeline's optimize_pose_graph"
    med = ab_events(f"K {K}", calls, reps)
    o = outs[GRAPH_ITER[-1]]
    emit(f"# K {K}: {P} pairs; refinement status 0 / 1 / 2 / 3: " + " / ".join(str(int((refined['status'] == v).sum())) for v in range(4)) +
         f"; graph of {GRAPH_ITER[-1]} steps at most: status {int(o['status'][0])}, accepted steps {int(o['iterations'][0])}, used edges "
         f"{int(o['used_edges'][0])}, skipped {int(o['skipped_edges'][0])}, failed_row {int(o['failed_row'][0])}, cost {float(o['cost_in'][0]):.6g} -> "
         f"{float(o['cost'][0]):.6g}; graph of 1 step at most: status {int(outs[1]['status'][0])}, accepted {int(outs[1]['iterations'][0])}")
    for n in GRAPH_ITER:
        emit(f"# K {K}: graph {n} / ransac 256 = {med[f'graph {n}'] / med['ransac 256']:.3f}; / refine 5 = {med[f'graph {n}'] / med['refine 5']:.3f}")
    emit("# one 256-thread workgroup: a latency figure, not a throughput one")

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
