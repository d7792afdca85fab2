#!/usr/bin/env python3
"""The sub-cell localisation launch (sslx_subcell_keypoints, libsslam_ext.so) beside the selection launch it follows
(sslam_select_keypoints), on the same frames in the same process, and the online step with and without it:

  launches   613 frames x 500 keypoints (G = 28) and 512 frames x 2048 keypoints (G = 60): the saliency of 32 extracted synthetic
             frames repeated; `select` writes the idx that `subcell` then reads - raw C-ABI calls on preallocated buffers
  step       online.FrameStepper (tokens in, captured graph, K = 500, G = 28) on a pipeline with subcell=False and subcell=True

Protocol: that of tools/pose_refine_probe.py - every variant warmed, then `repeats` rounds taken ALTERNATELY, one
block of `reps` back-to-back calls of every variant per round between two events on the stream; printed: median and min - max of
the per-call time over the rounds, in microseconds, and the ratio of the new launch to the selection launch.
    tools/subcell_probe.py [--repeats 7] [--out profiles/subcell.txt]"""
import ctypes as C
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import synth
from sslam_amd import lib
from sslam_amd.online import FrameStepper
from sslam_amd.pipeline import ExtractorConfig, SequencePipeline

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

N_EXTRACT = 32
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
        emit(f"{row:18s} {v:14s} median {statistics.median(us[v]):9.1f} us   min {min(us[v]):9.1f}   max {max(us[v]):9.1f}   "
             f"({reps} calls x {repeats} rounds)")
    return {v: statistics.median(x) for v, x in us.items()}


emit(f"# sub-cell localisation launch beside the selection launch, and the online step with and without it; us per call, all measured; "
     f"{torch.cuda.get_device_name(0)}")
ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
with torch.no_grad():
    for grid, K, n_seq, reps in ((28, 500, 613, 50), (60, 2048, 512, 20)):
        cfg = ExtractorConfig(input_size=16 * grid, num_keypoints=K)
        pipe = SequencePipeline(cfg, synth.selector_state(0), synth.refiner_state(0), device="cuda")
        ex = pipe.extract(torch.from_numpy(synth.token_sequence(N_EXTRACT, grid)).cuda(), None)
        sal = ex["saliency"][torch.arange(n_seq, device="cuda") % N_EXTRACT].contiguous()
        dev = dict(device="cuda")
        kp, px, kps, pxs = (torch.empty((n_seq, K, 2), dtype=torch.float32, **dev) for _ in range(4))
        sc = torch.empty((n_seq, K), dtype=torch.float32, **dev)
        idx, fl = (torch.empty((n_seq, K), dtype=torch.int32, **dev) for _ in range(2))
        st = torch.empty((n_seq,), dtype=torch.int32, **dev)
        L, X = lib.lib(), lib.ext()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def select():
            assert L.sslam_select_keypoints(ptr(sal), n_seq, grid, K, cfg.nms_radius, C.c_double(cfg.min_score_percentile), ptr(kp), ptr(sc),
                                            ptr(idx), ptr(px), ptr(st), stream) == 0

        def subcell():
            assert X.sslx_subcell_keypoints(ptr(sal), n_seq, grid, ptr(idx), K, ptr(kps), ptr(pxs), ptr(fl), stream) == 0

        select()
        subcell()
        torch.cuda.synchronize()
        by_wrapper = lib.subcell_keypoints(sal, idx)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(by_wrapper, (kps, pxs, fl))), "the raw call is the wrapper's"
        med = ab_events(f"{n_seq} x {K} (G {grid})", {"select": select, "subcell": subcell}, reps)
        moved = n_seq * K * (4 + 5 * 4 + 8 + 8 + 4)
        emit(f"# {n_seq} x {K}: subcell / select = {med['subcell'] / med['select']:.3f}"
             + (" - ABOVE the selection launch" if med["subcell"] > med["select"] else "")
             + f"; refined on both axes {float((fl == 3).float().mean()):.3f} of the keypoints, on neither {float((fl == 0).float().mean()):.3f}; "
             f"{moved / 1e6:.1f} MB requested per call (idx, five saliency words, two pairs, flags) = {moved / med['subcell'] / 1e3:.1f} GB/s "
             "at the median (computed from shapes over the event time; the saliency words mostly hit in cache)")

    # the online step: tokens in, captured graph
    grid, K = 28, 500
    toks = torch.from_numpy(synth.token_sequence(8, grid)).cuda()
    imgs = torch.from_numpy(synth.image_sequence(8, 480, 640)).cuda()
    steppers = {}
    for name, on in (("step", False), ("step + subcell", True)):
        pipe = SequencePipeline(ExtractorConfig(input_size=16 * grid, num_keypoints=K, subcell=on), synth.selector_state(0),
                                synth.refiner_state(0), device="cuda")
        steppers[name] = FrameStepper(pipe, 480, 640, use_graph=True, tokens_in=True)
    count = {name: 0 for name in steppers}

    def stepper_call(name):
        def call():
            i = count[name] % 8
            count[name] += 1
            steppers[name].step(imgs[i], toks[i])
        return call

    med = ab_events("online K 500", {name: stepper_call(name) for name in steppers}, 50)
    emit(f"# online step: with subcell - without = {med['step + subcell'] - med['step']:+.1f} us at the medians "
         f"({med['step + subcell'] / med['step']:.4f} of the step); the step includes the copies of the frame and its tokens into the "
         "static buffers and the graph launch")

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
