#!/usr/bin/env python3
"""The validation stage (csrc/validate.hip) at the size of a validation sequence: 613 frames x 500 keypoints at 448 x 448,
612 pairs at spacing 1, one process:

  frames       the per-frame launch group: Sobel / pool over the fp32 image + the per-frame statistics
  sobel        its Sobel / pool launch alone, also as bytes over time (3 fp32 planes read once) beside A0's rate
  row lse      the row log-sum-exp launch
  rows only    sslam_sim_argmax_rows on the same pairs: the same GEMM without the exp - the parent commit's entry, the yardstick
  arg-max      the two-direction arg-max launch the stage starts from (sslam_sim_argmax, S evaluated once + key reduction)
  pairs        the per-pair finalize launch
  stage        validation_stats on the fp32 image: all of the above, as a caller pays it
  eager        the same seven terms and five metrics in eager torch on the same device tensors, batches of 4 as the trainer
               runs them (a K x K logits matrix per pair, the per-sample Python loop, .item() per batch): what a caller pays today

The 613 frames are 32 extracted synthetic frames repeated (frame i = extracted frame i mod 32); no time here depends on the values.

Protocol (tools/match_rules_probe.py): every variant is warmed first, then REPEATS rounds are taken ALTERNATELY - one timed block
of every variant per round - each block `reps` calls between two device synchronisations, host clock.  Printed: median and
min - max of the per-call time over the rounds.
    tools/validation_probe.py [--repeats 7] [--out profiles/validation_stage.txt]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import torch.nn.functional as F
import synth
from sslam_amd import lib, validation
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

N_EXTRACT, N_SEQ, SP, T = 32, 613, 1, 0.1
pipe = SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0), device="cuda")
toks = torch.from_numpy(synth.token_sequence(N_EXTRACT, 28)).cuda()
imgs = torch.from_numpy(synth.image_sequence(N_EXTRACT)).cuda()
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def ab(calls, reps):
    """calls: {variant: zero-argument callable}; alternating timed blocks of `reps` calls, `repeats` rounds -> {variant: median ms}."""
    for fn in calls.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {v: [] for v in calls}
    for _ in range(repeats):
        for v, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms[v].append((time.perf_counter() - t0) / reps * 1e3)
    for v in calls:
        emit(f"{v:10s} median {statistics.median(ms[v]):9.3f} ms   min {min(ms[v]):9.3f}   max {max(ms[v]):9.3f}   ({reps} calls x {repeats} rounds)")
    return {v: statistics.median(ms[v]) for v in calls}


def eager_terms(sal, img, desc, first, second, batch=4):
    """The trainer's losses and metrics as it evaluates them (train.py:331-406), in eager torch under no_grad."""
    w, tot, n = validation.WEIGHTS, {}, 0
    sob_x = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], device=sal.device).view(1, 1, 3, 3)
    sob_y = sob_x.transpose(2, 3).contiguous()
    for a in range(0, len(first), batch):
        f, s = first[a:a + batch], second[a:a + batch]
        s1, s2, d1, d2, im = sal[f], sal[s], desc[f], desc[s], img[f]
        B, K = d1.shape[0], d1.shape[1]
        ml = []
        for b in range(B):
            sim = d1[b] @ d2[b].t()
            nn12, nn21 = sim.argmax(1), sim.argmax(0)
            i1 = torch.nonzero(nn21[nn12] == torch.arange(K, device=sim.device)).squeeze(1)
            ml.append(torch.stack([i1, nn12[i1]], 1))
        mmax = max(m.shape[0] for m in ml)
        ml = [torch.cat([m, m.new_zeros((mmax - m.shape[0], 2))]) for m in ml]
        loss_desc = 0.0
        for b in range(B):
            logits = torch.clamp(d1[b, ml[b][:, 0]] @ d2[b].t() / T, -50, 50)
            loss_desc = loss_desc + F.cross_entropy(logits, ml[b][:, 1])
        t = dict(desc=loss_desc / B)
        t["variance"] = F.relu(0.005 - d1.reshape(B * K, -1).var(0).mean())
        t["repeat"] = F.mse_loss(s1.reshape(B, -1), s2.reshape(B, -1))
        t["peakiness"] = (s1.reshape(B, -1).var(1, unbiased=False).mean() - 0.22) ** 2
        t["activation"] = (s1.mean() - 0.35) ** 2
        gray = (0.299 * im[:, 0] + 0.587 * im[:, 1] + 0.114 * im[:, 2]).unsqueeze(1)
        mag = torch.sqrt(F.conv2d(gray, sob_x, padding=1) ** 2 + F.conv2d(gray, sob_y, padding=1) ** 2 + 1e-8)
        e = F.adaptive_avg_pool2d(mag / (mag.max() + 1e-8), s1.shape[1:]).reshape(B, -1)
        sf = s1.reshape(B, -1)
        ec, sc = e - e.mean(1, keepdim=True), sf - sf.mean(1, keepdim=True)
        t["edge"] = -((ec * sc).sum(1) / (torch.sqrt((ec ** 2).sum(1) * (sc ** 2).sum(1)) + 1e-8)).mean()
        var = ((s1[:, :, 1:] - s1[:, :, :-1]).abs().mean() + (s1[:, 1:, :] - s1[:, :-1, :]).abs().mean()) / 2
        t["sparsity"] = F.relu(0.15 - var) + F.relu((s1 > 0.6).float().mean() - 0.20) * 2.0
        total = sum(w[k] * t[k] for k in w)
        row = {k: v.item() for k, v in t.items()}
        row["total"] = total.item()
        sal_np, desc_np = s1.cpu().numpy(), d1.cpu().numpy()
        row.update(num_matches=mmax, mean_saliency=float(np.mean(sal_np)), max_saliency=float(np.max(sal_np)),
                   saliency_variance=float(np.var(sal_np)), descriptor_variance=float(np.var(desc_np)))
        for k, v in row.items():
            tot[k] = tot.get(k, 0.0) + v
        n += 1
    return {k: v / n for k, v in tot.items()}


with torch.no_grad():
    ex = pipe.extract(toks, None)
    idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
    desc, sal = ex["descriptors"][idx].contiguous(), ex["saliency"][idx].contiguous()
    img = pipe.preprocess(imgs)[idx].contiguous()
    n, k, g, size = N_SEQ, desc.shape[1], sal.shape[1], img.shape[2]
    n_pairs, stride = n - SP, k * lib.D_OUT
    out = dict(saliency=sal, descriptors=desc)
    emit(f"# validation stage, {n} frames x {k} keypoints at {size} x {size}, {n_pairs} pairs, T = {T}; ms per call; {torch.cuda.get_device_name(0)}")
    d1, d2 = desc[:n_pairs], desc[SP:]
    ws = pipe.workspace(0, n_pairs)
    pooled, emax = lib.edge_pool(img)
    nn12, s12, nn21, _, _ = lib.sim_argmax(d1, stride, k, d2, stride, k, n_pairs, workspace=ws)
    lse, ce, s00 = lib.row_lse(d1, stride, k, d2, stride, k, n_pairs, s12, T)
    rows_out = lib.sim_argmax_rows(d1, stride, k, d2, stride, k, n_pairs)

    def frames():
        lib.edge_pool(img, out=(pooled, emax))
        lib.val_frame_stats(sal, pooled, emax, desc)

    med = ab({"frames": frames,
              "sobel": lambda: lib.edge_pool(img, out=(pooled, emax)),
              "row lse": lambda: lib.row_lse(d1, stride, k, d2, stride, k, n_pairs, s12, T),
              "rows only": lambda: lib.sim_argmax_rows(d1, stride, k, d2, stride, k, n_pairs, out=rows_out),
              "arg-max": lambda: lib.sim_argmax(d1, stride, k, d2, stride, k, n_pairs, workspace=ws),
              "pairs": lambda: lib.val_pair_stats(sal[:n_pairs], sal[SP:], nn12, nn21, s12, ce, s00, T),
              "stage": lambda: pipe.validation_stats(out, img, spacing=SP, temperature=T)}, 10)
    gb = n * 3 * size * size * 4 / 1e9
    emit(f"sobel: {gb:.3f} GB of fp32 image read once in {med['sobel']:.3f} ms = {gb / med['sobel']:.2f} TB/s (A0 writes that image at 3.97 TB/s)")
    emit(f"row lse / rows only = {med['row lse'] / med['rows only']:.2f}")
    first = torch.arange(n_pairs, device="cuda")
    second = first + SP
    med2 = ab({"stage": lambda: validation.reduce_batches(pipe.validation_stats(out, img, spacing=SP, temperature=T), 4),
               "eager": lambda: eager_terms(sal, img, desc, first, second, 4)}, 1)
    emit(f"stage + compose (one read-back) against eager torch, both to the dictionary of validate(): {med2['eager'] / med2['stage']:.1f} x")
    a, b = validation.reduce_batches(pipe.validation_stats(out, img, spacing=SP, temperature=T), 4), eager_terms(sal, img, desc, first, second, 4)
    for key in ("total",) + validation.TERMS + validation.METRICS:
        emit(f"  {key:20s} stage {a[key]:+.7e}   eager fp32 {b[key]:+.7e}")

if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
