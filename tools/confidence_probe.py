#!/usr/bin/env python3
"""The keypoint confidence head (libsslam_conf.so) at the flagship size, beside the descriptor MLP launch it follows and beside the
eager-torch form it replaces, in one process:

  gather_confidence   sslc_gather_confidence, 613 frames x 500 keypoints, D = 128, G = 28: the launch of extract(confidence=True)
  gather_refine       sslam_gather_refine_ws on the same features and keypoints: the descriptor MLP (the ratio's denominator)
  eager               the same head as torch ops on the same device: lib.gather (the (613, 500, 384) tensor written out), torch.cat
                      and the nn.Sequential of three Linear layers - what a user ran before this library; the baseline to beat
  confidence_rows     sslc_confidence_rows on the gathered tensor (the drop-in's forward)
  filter, take 128    sslc_confidence_filter at the median confidence and one 128-wide sslc_take_rows through its slots

Protocol: that of tools/subcell_probe.py - every variant warmed, then `repeats` rounds taken ALTERNATELY, one block of `reps`
back-to-back calls of every variant per round between two events on the stream; printed: median and min - max of the per-call
time over the rounds, in microseconds.  The FLOP count is arithmetic from the shapes, the matrix peak bench.py's nominal figure.
    tools/confidence_probe.py [--repeats 7] [--out profiles/confidence_head.txt]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import synth
from models.uncertainty_estimator import UncertaintyEstimator
from sslam_amd import lib
from sslam_amd.pipeline import ExtractorConfig, PackedConfidence, SequencePipeline

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

FP32_MATRIX_PEAK_TFLOPS = 157.3      # bench.py's nominal figure (v_mfma_f32_32x32x2_f32 at 2.4 GHz)
N_EXTRACT, N_SEQ, K, GRID, D = 32, 613, 500, 28, 128
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def ab_events(calls, reps):
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
        emit(f"{v:18s} median {statistics.median(us[v]):9.1f} us   min {min(us[v]):9.1f}   max {max(us[v]):9.1f}   ({reps} calls x {repeats} rounds)")
    return {v: statistics.median(x) for v, x in us.items()}


emit(f"# keypoint confidence head, {N_SEQ} frames x {K} keypoints, D = {D}, G = {GRID}; us per call, all measured; {torch.cuda.get_device_name(0)}")
with torch.no_grad():
    cfg = ExtractorConfig(input_size=16 * GRID, num_keypoints=K)
    pipe = SequencePipeline(cfg, synth.selector_state(0), synth.refiner_state(0), device="cuda")
    toks = torch.from_numpy(synth.token_sequence(N_EXTRACT, GRID)).cuda()
    ex = pipe.extract(toks, None)
    pick = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
    feat = pipe.features(toks)[pick].contiguous()
    kp, desc = ex["keypoints_patch"][pick].contiguous(), ex["descriptors"][pick].contiguous()
    torch.manual_seed(0)
    head = UncertaintyEstimator(384, D, 128).cuda().eval()
    for p in head.parameters():
        p.mul_(4.0)                      # confidences spread over (0, 1): the filter then has something to drop
    packed = PackedConfidence(head.state_dict(), "cuda").packed
    conf = torch.empty((N_SEQ, K), dtype=torch.float32, device="cuda")
    conf_rows = torch.empty_like(conf)
    desc_out = torch.empty_like(desc)
    x = torch.empty((N_SEQ, K, 384), dtype=torch.float32, device="cuda")
    ws = pipe.workspace(N_SEQ, 0)
    taken = torch.empty_like(desc)
    lib.gather_confidence(feat, kp, desc, packed, out=conf)
    slot, count, conf_out = lib.confidence_filter(conf, float(conf.median()))

    def eager():
        lib.gather(feat, kp, out=x)
        return head.mlp(torch.cat([x, desc], dim=-1))

    calls = {
        "gather_confidence": lambda: lib.gather_confidence(feat, kp, desc, packed, out=conf),
        "gather_refine": lambda: lib.gather_refine(feat, kp, pipe.refiner.packed, pipe.refiner.n_blocks, out=desc_out, workspace=ws),
        "eager": eager,
        "confidence_rows": lambda: lib.confidence_rows(x, desc, packed, out=conf_rows),
        "filter": lambda: lib.confidence_filter(conf, 0.5, out=(slot, count, conf_out)),
        "take 128": lambda: lib.take_rows(desc, slot, out=taken),
    }
    e = eager()[..., 0]
    lib.confidence_rows(x, desc, packed, out=conf_rows)
    assert torch.equal(conf.view(torch.int32), conf_rows.view(torch.int32)), "the gather form gives the rows form's bits"
    emit(f"# eager torch against the kernel on these rows: max |difference| {float((e - conf).abs().max()):.3g}; confidence "
         f"{float(conf.min()):.3g} .. {float(conf.max()):.3g}; kept at the median threshold {int(count.sum())} of {N_SEQ * K}")
    med = ab_events(calls, 20)
    flop = N_SEQ * K * 2 * ((384 + D) * 128 + 128 * 64 + 64)
    tf = flop / med["gather_confidence"] / 1e6
    emit(f"# gather_confidence: {flop / 1e9:.2f} GFLOP (from the shapes) in {med['gather_confidence']:.1f} us = {tf:.1f} TFLOP/s = "
         f"{tf / FP32_MATRIX_PEAK_TFLOPS:.3f} of the nominal fp32 matrix peak ({FP32_MATRIX_PEAK_TFLOPS} TFLOP/s)")
    emit(f"# gather_confidence / gather_refine = {med['gather_confidence'] / med['gather_refine']:.3f} "
         f"(FLOP ratio {((384 + D) * 128 + 128 * 64 + 64) / 786432:.3f})")
    emit(f"# eager / gather_confidence = {med['eager'] / med['gather_confidence']:.2f}"
         + (" - the kernel is SLOWER than eager torch" if med["eager"] < med["gather_confidence"] else "")
         + f"; eager writes and re-reads {N_SEQ * K * (384 + 384 + D) * 4 / 1e6:.0f} MB of gathered and concatenated rows")
    moved = N_SEQ * K * (4 + 128 * 4 * 2)
    emit(f"# take 128: {moved / 1e6:.1f} MB per call (slot, one row read, one written) = {moved / med['take 128'] / 1e3:.1f} GB/s at the median")

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
