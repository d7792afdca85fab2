#!/usr/bin/env python3
"""Descriptor width 128 against 256, one process, K = 500:

  match 612 ws    the matcher stage over 612 pairs (613 frames, spacing 1): similarity evaluated once + 64-bit key reduction
                  (sslam_sim_argmax_ws with a workspace) + the M1 finalize
  match 612 2dir  the same pairs through the two-direction form (test knob SSLAM_M1_VARIANT = 1: no workspace)
  gather_refine   613 frames of a 28 x 28 grid, 500 keypoints each, through gather + descriptor MLP (the distinct-row work list)

Yardstick of the 256 rows: the matcher does twice the FLOPs on twice the candidate bytes, so 2 x its own 128 time of the same
run; the refiner adds 384 x 128 x 2 FLOP per row to 1 572 864 (+ 6.25 %), so 1.0625 x its 128 time.  Printed beside the times.

The 613 frames are 32 synthetic frames repeated (the times do not depend on the values); the descriptors the matcher sees are
the refiner's own at each width.

Protocol (tools/backbone_batch_sweep.py): both widths are warmed first, then REPEATS rounds are taken ALTERNATELY - one timed block
per width per round - each block `reps` calls between two device synchronisations, host clock.  Printed: median and min - max of
the per-call time over the rounds, in microseconds.
    tools/desc_width_probe.py [--repeats 5] [--out profiles/desc_width_256.txt]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import synth
from sslam_amd import lib
from sslam_amd.pipeline import ExtractorConfig, SequencePipeline

args, repeats, out_path = sys.argv[1:], 5, None
while args:
    if args[0] == "--repeats" and len(args) > 1:
        repeats = int(args[1])
    elif args[0] == "--out" and len(args) > 1:
        out_path = args[1]
    else:
        raise SystemExit(__doc__)
    args = args[2:]
assert torch.cuda.is_available(), "this probe measures on the GPU only"

WIDTHS, N_EXTRACT, N_SEQ, G, K = (128, 256), 32, 613, 28, 500
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def ab(row, calls, reps, yardstick):
    """calls: {width: zero-argument callable}; alternating timed blocks of `reps` calls, `repeats` rounds."""
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {w: [] for w in calls}
    for _ in range(repeats):
        for w, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            us[w].append((time.perf_counter() - t0) / reps * 1e6)
    med = {w: statistics.median(us[w]) for w in calls}
    for w in calls:
        note = "" if w == 128 else f"   yardstick {yardstick:.4g} x D=128 = {yardstick * med[128]:9.1f} us -> {med[w] / (yardstick * med[128]):.2f} x yardstick"
        emit(f"{row:15s} D={w:3d} median {med[w]:9.1f} us   min {min(us[w]):9.1f}   max {max(us[w]):9.1f}   ({reps} calls x {repeats} rounds){note}")


with torch.no_grad():
    emit(f"# descriptor width 128 vs 256, K = {K}, {N_SEQ} frames / {N_SEQ - 1} pairs; us per call; {torch.cuda.get_device_name(0)}")
    pipes = {w: SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0, d_out=w), device="cuda") for w in WIDTHS}
    toks = torch.from_numpy(synth.token_sequence(N_EXTRACT, G)).cuda()
    imgs = torch.from_numpy(synth.image_sequence(N_EXTRACT)).cuda()
    idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
    seq, outs = {}, {}
    for w, pipe in pipes.items():
        ex = pipe.extract(toks, imgs)
        seq[w] = {k: ex[k][idx].contiguous() for k in ("descriptors", "scores", "intensity", "keypoints_patch")}
        outs[w] = pipe.alloc_match(N_SEQ - 1, K)

    def match(w):
        s = seq[w]
        return pipes[w].match(s["descriptors"], s["scores"], s["intensity"], spacing=1, out=outs[w])

    ab("match 612 ws", {w: (lambda w=w: match(w)) for w in WIDTHS}, 20, 2.0)
    emit("# matches over the 612 pairs: " + ", ".join(f"D={w} {int(outs[w]['match_count'].sum())}" for w in WIDTHS))
    with lib.knobs(SSLAM_M1_VARIANT=1):
        ab("match 612 2dir", {w: (lambda w=w: match(w)) for w in WIDTHS}, 20, 2.0)

    feat = pipes[128].features(toks)[idx].contiguous()                      # (613, 28, 28, 384): 740 MB
    desc = {w: torch.empty((N_SEQ, K, w), dtype=torch.float32, device="cuda") for w in WIDTHS}

    def refine(w):
        p = pipes[w]
        return lib.gather_refine(feat, seq[w]["keypoints_patch"], p.refiner.packed, p.refiner.n_blocks, out=desc[w], workspace=p.workspace(N_SEQ, 0))

    ab("gather_refine", {w: (lambda w=w: refine(w)) for w in WIDTHS}, 5, 1.0 + 384 * 128 * 2 / 1572864)

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
