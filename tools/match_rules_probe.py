#!/usr/bin/env python3
"""The matcher stage under rule=None (M1: the parent commit's code path, untouched, re-measured here in the same process) and
under each MatchRule (M2 ratio, M4 mnn_ratio, M5 tracked), K = 500:

  step        a whole tokens-in online step (FrameStepper / RuleFrameStepper, ordinary launches): A2 .. A9 + the matcher
  step graph  the same step replayed from its captured graph
  stage 1     the matcher stage of that step alone: match() of the previous frame against this one (1 pair, two-pass form;
              tracked: the rows-only launch, half the similarity work)
  stage 5     the matcher stage of a spacings=(1, 5, 10, 15, 20) step: match_pairs() over 5 listed pairs
  match 612   match(spacing=1) over 613 frames: 612 pairs, S evaluated once + key reduction (tracked: rows only)

The 613 frames are 32 extracted synthetic frames repeated (frame i = extracted frame i mod 32): the matcher's time does not
depend on the descriptors' values beyond the number of rows the compaction writes.

Protocol (tools/backbone_batch_sweep.py): every variant of a row is warmed first, then REPEATS rounds are taken ALTERNATELY - one
timed block of every variant per round - each block `reps` calls between two device synchronisations, host clock.  Printed:
median and min - max of the per-call time over the rounds, in microseconds.
    tools/match_rules_probe.py [--repeats 7] [--out profiles/match_rules.txt]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import synth
from sslam_amd.online import RuleFrameStepper
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

RULES = {"none (M1)": None, "ratio (M2)": MatchRule.ratio(), "mnn_ratio (M4)": MatchRule.mnn_ratio(), "tracked (M5)": MatchRule.tracked()}
N_EXTRACT, N_SEQ = 32, 613
pipe = SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0), device="cuda")
toks = torch.from_numpy(synth.token_sequence(N_EXTRACT, 28)).cuda()
imgs = torch.from_numpy(synth.image_sequence(N_EXTRACT)).cuda()
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def ab(row, calls, reps):
    """calls: {variant: zero-argument callable}; alternating timed blocks of `reps` calls, `repeats` rounds."""
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {v: [] for v in calls}
    for _ in range(repeats):
        for v, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            us[v].append((time.perf_counter() - t0) / reps * 1e6)
    for v in calls:
        emit(f"{row:11s} {v:15s} median {statistics.median(us[v]):9.1f} us   min {min(us[v]):9.1f}   max {max(us[v]):9.1f}   ({reps} calls x {repeats} rounds)")


with torch.no_grad():
    ex = pipe.extract(toks, imgs)
    idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
    desc, scores, inten = (ex[k][idx].contiguous() for k in ("descriptors", "scores", "intensity"))
    emit(f"# matcher stage by rule, K = 500, MI355X; us per call; rule none = the M1 path of the parent commit, same process; {torch.cuda.get_device_name(0)}")

    for graph, row in ((False, "step"), (True, "step graph")):
        steppers = {v: RuleFrameStepper(pipe, 480, 640, use_graph=graph, tokens_in=True, rule=r) for v, r in RULES.items()}
        for st in steppers.values():
            for t in range(2):
                st.step(imgs[t], toks[t])
        ab(row, {v: (lambda st=st: st.step(imgs[2], toks[2])) for v, st in steppers.items()}, 100)

    pair = {k: ex[k][:2].contiguous() for k in ("descriptors", "scores", "intensity")}
    outs = {v: pipe.alloc_match(1, 500, r) for v, r in RULES.items()}
    ab("stage 1", {v: (lambda v=v, r=r: pipe.match(pair["descriptors"], pair["scores"], pair["intensity"], spacing=1, out=outs[v], rule=r))
                   for v, r in RULES.items()}, 200)

    first = torch.tensor([20 - s for s in (1, 5, 10, 15, 20)], dtype=torch.int32, device="cuda")
    second = torch.full((5,), 20, dtype=torch.int32, device="cuda")
    bank = {k: ex[k][:21].contiguous() for k in ("descriptors", "scores", "intensity")}
    outs5 = {v: pipe.alloc_match(5, 500, r) for v, r in RULES.items()}
    ab("stage 5", {v: (lambda v=v, r=r: pipe.match_pairs(bank["descriptors"], bank["scores"], bank["intensity"], first=first, second=second,
                                                          out=outs5[v], rule=r)) for v, r in RULES.items()}, 200)

    outs612 = {v: pipe.alloc_match(N_SEQ - 1, 500, r) for v, r in RULES.items()}
    ab("match 612", {v: (lambda v=v, r=r: pipe.match(desc, scores, inten, spacing=1, out=outs612[v], rule=r)) for v, r in RULES.items()}, 20)
    counts = {v: int(outs612[v]["match_count"].sum()) for v in RULES}
    emit("# rows kept over the 612 pairs: " + ", ".join(f"{v} {c}" for v, c in counts.items()))

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
