#!/usr/bin/env python3
"""The pose-based scoring stage (sslam_pose_nn_pairs, sslam_match_score_pairs) beside the matching it scores, on the 613-frame
synthetic workload (612 pairs at spacing 1; the 613 frames are 32 extracted synthetic frames repeated, as in
tools/match_rank_probe.py) at K = 500 (G = 28) and K = 2048 (G = 60):

  similarity   sslam_sim_argmax_pairs over the 612 listed pairs, runner-up included (what M4 reads) - the yardstick
  finalize     sslam_match_finalize_rule_pairs, rule M4 (ratio 0.9), over the same pairs
  pose nn      sslam_pose_nn_pairs over the same pairs, H = K R K^-1 of small random rotations, threshold 3 px
  pose nn raw  the same with H = NULL
  score        sslam_match_score_pairs of that finalize's lists against that ground truth

Protocol: raw C-ABI calls on preallocated buffers, timed with device events - every variant warmed, then `repeats` rounds taken
ALTERNATELY, one block of `reps` back-to-back calls of every variant per round between two events on the stream; printed: median
and min - max of the per-call time over the rounds, in microseconds, and each scoring launch as a fraction of the yardstick.
    tools/pose_eval_probe.py [--repeats 7] [--out profiles/pose_eval.txt]"""
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

N_EXTRACT, N_SEQ = 32, 613
P = N_SEQ - 1
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
        emit(f"{row:8s} {v:12s} median {statistics.median(us[v]):9.1f} us   min {min(us[v]):9.1f}   max {max(us[v]):9.1f}   "
             f"({reps} calls x {repeats} rounds)")
    return {v: statistics.median(x) for v, x in us.items()}


def rotation_h(rng):
    v = rng.normal(0.0, 0.004, 3)
    t = np.linalg.norm(v)
    k = v / t
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.eye(3) + np.sin(t) * kx + (1 - np.cos(t)) * kx @ kx
    return evaluation.homography(T)


emit(f"# scoring stage beside the matching it scores, 613 frames / 612 pairs; us per call, all measured; {torch.cuda.get_device_name(0)}")
with torch.no_grad():
    for grid, K, reps in ((28, 500, 50), (60, 2048, 10)):
        pipe = SequencePipeline(ExtractorConfig(input_size=16 * grid, num_keypoints=K), synth.selector_state(0), synth.refiner_state(0),
                                device="cuda")
        ex = pipe.extract(torch.from_numpy(synth.token_sequence(N_EXTRACT, grid)).cuda(), None)
        idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
        desc, scores, kp = (ex[k][idx].contiguous() for k in ("descriptors", "scores", "keypoints_pixel"))
        first = torch.arange(P, dtype=torch.int32, device="cuda")
        second = first + 1
        rng = np.random.default_rng(grid)
        H = torch.from_numpy(np.stack([rotation_h(rng) for _ in range(P)]).reshape(P, 9)).cuda()

        L = lib.lib()
        dev = dict(device="cuda")
        nn12, nn21 = (torch.empty((P, K), dtype=torch.int32, **dev) for _ in range(2))
        s12, sec = (torch.empty((P, K), dtype=torch.float32, **dev) for _ in range(2))
        rule = MatchRule.mnn_ratio(0.9)
        m = pipe.alloc_match(P, K, rule)
        sc = pipe.alloc_pose_scores(P, K)
        ws = pipe.workspace(0, P)
        ws_bytes = ws.numel() * ws.element_size()
        ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        d = desc.shape[2]

        def similarity():
            assert L.sslam_sim_argmax_pairs(ptr(desc), K * d, N_SEQ, K, ptr(first), ptr(second), P, ptr(nn12), ptr(s12), ptr(nn21), None,
                                            ptr(sec), ptr(ws), ws_bytes, stream) == 0

        def finalize():
            assert L.sslam_match_finalize_rule_pairs(ptr(nn12), ptr(s12), ptr(sec), ptr(nn21), K, N_SEQ, ptr(first), ptr(second), P, rule.kind,
                                                     C.c_float(rule.param), ptr(m["matches"]), ptr(m["value"]), ptr(m["match_count"]), stream) == 0

        def pose_nn(h):
            assert L.sslam_pose_nn_pairs(ptr(kp), N_SEQ, K, K, K, ptr(first), ptr(second), P, None if h is None else ptr(h), C.c_double(3.0),
                                         ptr(sc["gt_matches"]), ptr(sc["gt_count"]), ptr(sc["gt_of_row"]), ptr(sc["dist_sum"]),
                                         ptr(sc["dist_median"]), stream) == 0

        def score():
            assert L.sslam_match_score_pairs(ptr(m["matches"]), ptr(m["value"]), ptr(m["match_count"]), ptr(sc["gt_of_row"]), ptr(sc["gt_count"]),
                                             K, P, ptr(sc["tp"]), ptr(sc["fp"]), ptr(sc["fn"]), ptr(sc["value_sum"]), stream) == 0

        similarity()
        finalize()
        pose_nn(H)
        score()
        torch.cuda.synchronize()
        want = pipe.match_pairs(desc, scores, first=first, second=second, rule=rule)
        assert all(torch.equal(m[k], want[k]) for k in m), "the raw calls are the pipeline's matcher"
        ps = pipe.pose_scores(kp, first, second, H, 3.0, matches=want)
        assert all(torch.equal(sc[k], ps[k]) for k in sc), "the raw calls are the pipeline's scoring stage"
        med = ab_events(f"K {K}", {"similarity": similarity, "finalize": finalize, "pose nn": lambda: pose_nn(H), "pose nn raw": lambda: pose_nn(None),
                                   "score": score}, reps)
        pose_nn(H)
        torch.cuda.synchronize()
        emit(f"# K {K}: matches per pair mean {float(m['match_count'].float().mean()):.1f}; ground-truth rows per pair mean "
             f"{float(sc['gt_count'].float().mean()):.1f}; tp per pair mean {float(sc['tp'].float().mean()):.1f}")
        for v in ("pose nn", "pose nn raw", "score"):
            emit(f"# K {K}: {v} / similarity = {med[v] / med['similarity']:.3f}")
        emit(f"# K {K}: (pose nn + score) / (similarity + finalize) = {(med['pose nn'] + med['score']) / (med['similarity'] + med['finalize']):.3f}")

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
