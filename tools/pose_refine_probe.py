#!/usr/bin/env python3
"""The refinement launch (sslam_pose_refine_pairs) beside the RANSAC launch and the similarity launch, on the 613-frame synthetic
workload of tools/pose_ransac_probe.py (612 pairs at spacing 1; 32 extracted synthetic frames repeated, the depth of a synthetic
640 x 480 scene) at K = 500 (G = 28) and K = 2048 (G = 60), all in one process:

  similarity      sslam_sim_argmax_pairs over the 612 listed pairs, runner-up included - the yardstick of the scoring probes
  ransac 256      sslam_pose_ransac_pairs on the M4 lists (MatchRule.mnn_ratio(0.9)), 256 hypotheses, threshold 12 keypoint units
  refine N        sslam_pose_refine_pairs from RANSAC's poses on the same lists, threshold 12, huber 4, N = 1, 5 and 16 steps at most

On synthetic frames the poses mean nothing as accuracy: the tokens slide over a random field, no camera moves through a scene.
The probe times the launch; the accepted steps it prints say how much work the launch had, nothing else.

Protocol: that of tools/pose_ransac_probe.py - raw C-ABI calls on preallocated buffers, timed with device events; every variant
warmed, then `repeats` rounds taken ALTERNATELY, one block of `reps` back-to-back calls of every variant per round between two
events on the stream; printed: median and min - max of the per-call time over the rounds, in microseconds, and the ratios.
    tools/pose_refine_probe.py [--repeats 7] [--out profiles/pose_refine.txt]"""
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
P = N_SEQ - 1
HYPOTHESES, HUBER, ITERATIONS = 256, 4.0, (1, 5, 16)
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


emit(f"# refinement launch beside the RANSAC and similarity launches, 613 frames / 612 pairs; us per call, all measured; {torch.cuda.get_device_name(0)}")
cam = evaluation.Camera()
with torch.no_grad():
    for grid, K, reps in ((28, 500, 20), (60, 2048, 5)):
        pipe = SequencePipeline(ExtractorConfig(input_size=16 * grid, num_keypoints=K), synth.selector_state(0), synth.refiner_state(0),
                                device="cuda")
        ex = pipe.extract(torch.from_numpy(synth.token_sequence(N_EXTRACT, grid)).cuda(), None)
        idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
        desc, scores, kp = (ex[k][idx].contiguous() for k in ("descriptors", "scores", "keypoints_pixel"))
        first = torch.arange(P, dtype=torch.int32, device="cuda")
        second = first + 1
        depth = torch.from_numpy(scene_depth(N_EXTRACT)).cuda()
        sx, sy = pipe.depth_scales(cam)
        kd = torch.full((N_SEQ, K), -1, dtype=torch.int32, device="cuda")
        for a in range(0, N_SEQ, N_EXTRACT):                 # the whole bank's depths, from the 32 scene frames it repeats
            b = min(a + N_EXTRACT, N_SEQ)
            pipe.keypoint_depth(depth[:b - a], kp[a:b], out=kd[a:b])

        L = lib.lib()
        dev = dict(device="cuda")
        nn12, nn21 = (torch.empty((P, K), dtype=torch.int32, **dev) for _ in range(2))
        s12, sec = (torch.empty((P, K), dtype=torch.float32, **dev) for _ in range(2))
        rule = MatchRule.mnn_ratio(0.9)
        m = pipe.match_pairs(desc, scores, first=first, second=second, rule=rule)
        pose = pipe.alloc_pose(P, K)
        refined = {n: pipe.alloc_pose_refine(P, K) for n in ITERATIONS}
        ws = pipe.workspace(0, P)
        ws_bytes = ws.numel() * ws.element_size()
        ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        dbl = C.c_double
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        d = desc.shape[2]
        camera = (dbl(cam.fx), dbl(cam.fy), dbl(cam.cx), dbl(cam.cy), dbl(cam.depth_scale), dbl(sx), dbl(sy), dbl(cam.width), dbl(cam.height),
                  dbl(THRESHOLD))

        def similarity():
            assert L.sslam_sim_argmax_pairs(ptr(desc), K * d, N_SEQ, K, ptr(first), ptr(second), P, ptr(nn12), ptr(s12), ptr(nn21), None,
                                            ptr(sec), ptr(ws), ws_bytes, stream) == 0

        def ransac():
            assert L.sslam_pose_ransac_pairs(ptr(kp), ptr(kd), N_SEQ, K, ptr(first), ptr(second), P, ptr(m["matches"]), ptr(m["match_count"]),
                                             K, *camera, HYPOTHESES, C.c_uint64(SEED), *(ptr(pose[key]) for key in lib.POSE_RANSAC_KEYS),
                                             stream) == 0

        def refine(n_iter):
            o = refined[n_iter]

            def call():
                assert L.sslam_pose_refine_pairs(ptr(kp), ptr(kd), N_SEQ, K, ptr(first), ptr(second), P, ptr(m["matches"]), ptr(m["match_count"]),
                                                 K, *camera, ptr(pose["T"]), dbl(HUBER), n_iter, *(ptr(o[key]) for key in lib.POSE_REFINE_KEYS),
                                                 stream) == 0
            return call

        calls = {"similarity": similarity, "ransac 256": ransac}
        calls.update({f"refine {n}": refine(n) for n in ITERATIONS})
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        ps = pipe.refine_poses(kp, kd, first, second, m, cam, pose, THRESHOLD, HUBER, 5)
        assert all(torch.equal(refined[5][key].view(torch.int64) if ps[key].dtype == torch.float64 else refined[5][key],
                               ps[key].view(torch.int64) if ps[key].dtype == torch.float64 else ps[key]) for key in ps), \
            "the raw call is the pipeline's refine_poses"
        med = ab_events(f"K {K}", calls, reps)
        emit(f"# K {K}: listed matches per pair mean {float(m['match_count'].float().mean()):.1f}; usable rows per pair mean "
             f"{float(pose['usable_count'].float().mean()):.1f}; selected rows per pair mean {float(refined[5]['selected_count'].float().mean()):.1f}; "
             "accepted steps per pair mean " + ", ".join(f"{float(refined[n]['iterations'].float().mean()):.2f} of {n}" for n in ITERATIONS) +
             "; status 0 / 1 / 2 / 3 at 5 steps: " + " / ".join(str(int((refined[5]['status'] == v).sum())) for v in range(4)))
        for n in ITERATIONS:
            emit(f"# K {K}: refine {n} / ransac 256 = {med[f'refine {n}'] / med['ransac 256']:.3f}; / similarity = "
                 f"{med[f'refine {n}'] / med['similarity']:.3f}")

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
