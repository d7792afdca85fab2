#!/usr/bin/env python3
"""The weighted refinement launch (sslu_pose_refine_weighted_pairs) beside the unweighted one (sslam_pose_refine_pairs), the weights
launch (sslu_match_weights) and PoseFrameStepper's step with and without weights, all in one process, on the 613-frame synthetic
workload of tools/pose_refine_probe.py (32 extracted synthetic frames repeated, the depth of a synthetic 640 x 480 scene) at
K = 500 (G = 28), over the 3014 pairs of the five spacings 1, 5, 10, 15, 20:

  refine 5        sslam_pose_refine_pairs from RANSAC's poses on the M4 lists, threshold 12, huber 4, 5 steps at most - the same code
                  as before the weighted entry existed (csrc/pose_refine_common.h, instantiated without weights); it runs twice in
                  every round (`refine 5` and `refine 5 b`), so that the spread between two runs of one launch is on the page
  weighted 5      sslu_pose_refine_weighted_pairs on the same operands with the weights sslu_match_weights made of a seeded
                  confidence head's output (expected_error, sigma0 0.5)
  weights         sslu_match_weights over the 3014 x 500 slots, reported as bytes moved over time: 16 B of match and 4 B of weight per
                  slot, 8 B of gathered confidence per listed match
  step            online.PoseFrameStepper(refine=True), captured graph, tokens in: the time of one replayed step with weights=None
                  and with weights=PoseWeights.expected_error(0.5)

On synthetic frames the poses and the confidences mean nothing as accuracy.  The probe times launches, nothing else.

Protocol: that of tools/pose_refine_probe.py - raw C-ABI calls on preallocated buffers, timed with device events; every variant
warmed, then `repeats` rounds taken ALTERNATELY, one block of `reps` back-to-back calls of every variant per round between two
events on the stream; printed: median and min - max of the per-call time over the rounds, in microseconds, and the ratios.
    tools/weighted_refine_probe.py [--repeats 7] [--out profiles/weighted_refine.txt]"""
import ctypes as C
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import confidence_cases
import synth
from sslam_amd import evaluation, lib
from sslam_amd.online import PoseFrameStepper
from sslam_amd.pipeline import ExtractorConfig, MatchRule, PoseWeights, SequencePipeline

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
SPACINGS, GRID, K, REPS = (1, 5, 10, 15, 20), 28, 500, 20
HYPOTHESES, HUBER, N_ITER, SIGMA0 = 256, 4.0, 5, 0.5
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
    return us


def scene_depth(n, h=480, w=640):
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w), np.uint16)
    for f in range(n):
        steps = rng.integers(0, 1500, (h // 32 + 1, w // 32 + 1))[yy // 32, xx // 32]
        out[f] = (7500 + 10 * f + 8.0 * xx + 4.0 * yy + steps).astype(np.uint16)
        out[f, 100 + 5 * f:120 + 5 * f] = 0
    return out


emit(f"# weighted refinement beside the unweighted launch, 613 frames, the pairs of spacings {SPACINGS}; us per call, all measured; "
     f"{torch.cuda.get_device_name(0)}")
cam = evaluation.Camera()
weights = PoseWeights.expected_error(SIGMA0)
with torch.no_grad():
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * GRID, num_keypoints=K, confidence=True), synth.selector_state(0), synth.refiner_state(0),
                            device="cuda", confidence_state=confidence_cases.head_state("x4"))
    tokens = torch.from_numpy(synth.token_sequence(N_EXTRACT, GRID)).cuda()
    ex = pipe.extract(tokens, None)
    idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
    desc, scores, kp, conf = (ex[k][idx].contiguous() for k in ("descriptors", "scores", "keypoints_pixel", "confidence"))
    first = torch.cat([torch.arange(N_SEQ - s, dtype=torch.int32, device="cuda") for s in SPACINGS])
    second = torch.cat([torch.arange(N_SEQ - s, dtype=torch.int32, device="cuda") + s for s in SPACINGS])
    P = int(first.shape[0])
    depth = torch.from_numpy(scene_depth(N_EXTRACT)).cuda()
    sx, sy = pipe.depth_scales(cam)
    kd = torch.full((N_SEQ, K), -1, dtype=torch.int32, device="cuda")
    for a in range(0, N_SEQ, N_EXTRACT):
        b = min(a + N_EXTRACT, N_SEQ)
        pipe.keypoint_depth(depth[:b - a], kp[a:b], out=kd[a:b])
    m = pipe.match_pairs(desc, scores, first=first, second=second, rule=MatchRule.mnn_ratio(0.9))
    pose = pipe.estimate_poses(kp, kd, first, second, m, cam, THRESHOLD, HYPOTHESES, SEED)
    plain = {v: pipe.alloc_pose_refine(P, K) for v in ("refine 5", "refine 5 b")}
    weighted = pipe.alloc_pose_refine(P, K, weighted=True)
    w = torch.empty((P, K), dtype=torch.float32, device="cuda")

    L, U = lib.lib(), lib.weight()
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    dbl = C.c_double
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    camera = (dbl(cam.fx), dbl(cam.fy), dbl(cam.cx), dbl(cam.cy), dbl(cam.depth_scale), dbl(sx), dbl(sy), dbl(cam.width), dbl(cam.height),
              dbl(THRESHOLD))
    lists = (ptr(kp), ptr(kd), N_SEQ, K, ptr(first), ptr(second), P, ptr(m["matches"]), ptr(m["match_count"]), K)

    def refine(o):
        def call():
            assert L.sslam_pose_refine_pairs(*lists, *camera, ptr(pose["T"]), dbl(HUBER), N_ITER, *(ptr(o[key]) for key in lib.POSE_REFINE_KEYS),
                                             stream) == 0
        return call

    def refine_weighted():
        assert U.sslu_pose_refine_weighted_pairs(*lists, *camera, ptr(pose["T"]), dbl(HUBER), N_ITER, ptr(w),
                                                 *(ptr(weighted[key]) for key in lib.POSE_REFINE_WEIGHTED_KEYS), stream) == 0

    def match_weights():
        assert U.sslu_match_weights(ptr(conf), N_SEQ, K, ptr(first), ptr(second), P, ptr(m["matches"]), ptr(m["match_count"]), K, weights.mode,
                                    dbl(weights.sigma0), ptr(w), stream) == 0

    match_weights()
    torch.cuda.synchronize()
    assert torch.equal(w, pipe.match_weights(conf, first, second, m, weights)), "the raw call is the pipeline's match_weights"
    calls = {"refine 5": refine(plain["refine 5"]), "weighted 5": refine_weighted, "refine 5 b": refine(plain["refine 5 b"]), "weights": match_weights}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ps = pipe.refine_poses(kp, kd, first, second, m, cam, pose, THRESHOLD, HUBER, N_ITER, weights=w)
    assert all(torch.equal(weighted[key].view(torch.int64) if ps[key].dtype == torch.float64 else weighted[key],
                           ps[key].view(torch.int64) if ps[key].dtype == torch.float64 else ps[key]) for key in ps), \
        "the raw call is the pipeline's refine_poses(weights=)"
    us = ab_events(f"K {K}", calls, REPS)
    med = {v: statistics.median(x) for v, x in us.items()}
    both = us["refine 5"] + us["refine 5 b"]
    spread = (max(both) - min(both)) / statistics.median(both)
    listed = int(m["match_count"].clamp(0, K).sum())
    moved = P * K * 20 + listed * 8 + P * 12
    emit(f"# {P} pairs; listed matches per pair mean {listed / P:.1f}; selected rows per pair mean: unweighted "
         f"{float(plain['refine 5']['selected_count'].float().mean()):.1f}, weighted {float(weighted['selected_count'].float().mean()):.1f}; accepted "
         f"steps per pair mean: unweighted {float(plain['refine 5']['iterations'].float().mean()):.2f}, weighted "
         f"{float(weighted['iterations'].float().mean()):.2f} of {N_ITER}; status 0 / 1 / 2 / 3 weighted: "
         + " / ".join(str(int((weighted['status'] == v).sum())) for v in range(4)))
    emit(f"# weighted 5 / refine 5 = {med['weighted 5'] / med['refine 5']:.3f}; refine 5 b / refine 5 = {med['refine 5 b'] / med['refine 5']:.3f}; "
         f"run-to-run spread of the unweighted launch (max - min over both, / median) = {spread:.3f}; accepted up to "
         f"1 + max(0.05, 3 x spread) = {1 + max(0.05, 3 * spread):.3f}")
    emit(f"# weights: {moved / 1e6:.2f} MB moved in {med['weights']:.1f} us = {moved / med['weights'] / 1e3:.1f} GB/s "
         "(sslc_take_rows' figure stands in profiles/confidence_head.txt)")

    # ---- the online step, replayed from its captured graph
    image = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
    steppers = {name: PoseFrameStepper(pipe, 48, 64, 480, 640, camera=cam, use_graph=True, tokens_in=True, threshold=THRESHOLD, hypotheses=HYPOTHESES,
                                       seed=SEED, refine=True, huber=HUBER, iterations=N_ITER, weights=wt)
                for name, wt in (("step", None), ("step weighted", weights))}
    at = {name: 0 for name in steppers}

    def step(name):
        def call():
            i = at[name] % N_EXTRACT
            steppers[name].step(image, depth[i], tokens[i])
            at[name] += 1
        return call
    us = ab_events("online", {name: step(name) for name in steppers}, REPS)
    med = {v: statistics.median(x) for v, x in us.items()}
    emit(f"# step weighted / step = {med['step weighted'] / med['step']:.3f} (one launch of {K} slots and the weighted kernel in the unweighted one's "
         "place; the frame's depth image is copied in inside the timed step)")

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
