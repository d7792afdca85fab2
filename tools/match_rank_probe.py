#!/usr/bin/env python3
"""The ranking stage (sslam_match_rank) beside the two launches it follows, on the 613-frame synthetic workload at K = 500
(612 pairs at spacing 1; the 613 frames are 32 extracted synthetic frames repeated, as in tools/match_rules_probe.py):

  similarity   sslam_sim_argmax_ws over the 612 pairs (S evaluated once: memset + kernel + key decode) - the yardstick
  finalize     sslam_match_finalize over the same pairs
  rank 50      sslam_match_rank of that finalize's lists, best = 50 (the reference script's --max_matches default)
  rank 500     the same, best = 500: whole lists
  step ...     a whole tokens-in online step without the stage (RuleFrameStepper(rule=None): the parent's step) and with it
               (RankedFrameStepper, best = 50), as ordinary launches and replayed from the captured graph

Protocol: the library rows are raw C-ABI calls on preallocated buffers, timed with device events - every variant warmed, then
`repeats` rounds taken ALTERNATELY, one block of `reps` back-to-back calls of every variant per round between two events on the
stream; printed: median and min - max of the per-call time over the rounds, in microseconds.  The step rows are host-clock blocks
that end in a device synchronisation (the step copies its frame in from the host's side, as tools/match_rules_probe.py times it).
    tools/match_rank_probe.py [--repeats 7] [--out profiles/match_rank.txt]"""
import ctypes as C
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import synth
from sslam_amd import lib
from sslam_amd.online import RankedFrameStepper, RuleFrameStepper
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

N_EXTRACT, N_SEQ, K = 32, 613, 500
P = N_SEQ - 1
cfg = ExtractorConfig()
pipe = SequencePipeline(cfg, synth.selector_state(0), synth.refiner_state(0), device="cuda")
toks = torch.from_numpy(synth.token_sequence(N_EXTRACT, 28)).cuda()
imgs = torch.from_numpy(synth.image_sequence(N_EXTRACT)).cuda()
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def report(row, v, us, reps):
    emit(f"{row:11s} {v:24s} median {statistics.median(us):9.1f} us   min {min(us):9.1f}   max {max(us):9.1f}   ({reps} calls x {repeats} rounds)")


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
        report(row, v, us[v], reps)
    return {v: statistics.median(x) for v, x in us.items()}


def ab_host(row, calls, reps):
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
        report(row, v, us[v], reps)
    return {v: statistics.median(x) for v, x in us.items()}


with torch.no_grad():
    ex = pipe.extract(toks, imgs)
    idx = torch.arange(N_SEQ, device="cuda") % N_EXTRACT
    desc, scores, inten = (ex[k][idx].contiguous() for k in ("descriptors", "scores", "intensity"))
    emit(f"# ranking stage beside similarity and finalize, K = 500, 613 frames / 612 pairs; us per call, all measured; {torch.cuda.get_device_name(0)}")

    L = lib.lib()
    dev = dict(device="cuda")
    nn12, nn21 = (torch.empty((P, K), dtype=torch.int32, **dev) for _ in range(2))
    s12 = torch.empty((P, K), dtype=torch.float32, **dev)
    m = pipe.alloc_match(P, K)
    ranked = {b: pipe.alloc_ranked(P, b, K) for b in (50, 500)}
    ws = pipe.workspace(0, P)
    ws_bytes = ws.numel() * ws.element_size()
    assert ws_bytes >= int(L.sslam_sim_argmax_workspace_bytes(K, P)) > 0, "the single-evaluation form is the one measured"
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = C.c_float
    d1, d2, w = desc[:P], desc[1:], K * desc.shape[2]

    def similarity():
        assert L.sslam_sim_argmax_ws(ptr(d1), w, K, ptr(d2), w, K, P, ptr(nn12), ptr(s12), ptr(nn21), None, None, ptr(ws), ws_bytes, stream) == 0

    def finalize():
        assert L.sslam_match_finalize(ptr(nn12), ptr(s12), ptr(nn21), K, K, P, ptr(scores), K, ptr(scores[1:]), K, ptr(inten), ptr(inten[1:]),
                                      f(1.0 - cfg.saliency_weight), f(cfg.saliency_weight), f(cfg.min_saliency), f(cfg.min_descriptor_sim),
                                      f(cfg.min_intensity), ptr(m["matches"]), ptr(m["quality"]), ptr(m["match_count"]), stream) == 0

    def rank(b):
        r = ranked[b]
        assert L.sslam_match_rank(ptr(m["matches"]), ptr(m["quality"]), ptr(m["match_count"]), K, P, b, 0, ptr(r["matches"]), ptr(r["quality"]),
                                  ptr(r["match_count"]), ptr(r["slot"]), stream) == 0

    similarity()
    finalize()
    torch.cuda.synchronize()
    want = pipe.match(desc, scores, inten, spacing=1)
    assert all(torch.equal(m[k], want[k]) for k in m), "the raw calls are the pipeline's matcher"
    med = ab_events("launch", {"similarity": similarity, "finalize": finalize, "rank 50": lambda: rank(50), "rank 500": lambda: rank(500)}, 50)
    counts = m["match_count"]
    emit(f"# rows per pair: min {int(counts.min())}, mean {float(counts.float().mean()):.1f}, max {int(counts.max())}; kept at 50: "
         f"{int(ranked[50]['match_count'].sum())}, at 500: {int(ranked[500]['match_count'].sum())}")
    for b in (50, 500):
        emit(f"# rank {b} / similarity = {med[f'rank {b}'] / med['similarity']:.3f}, rank {b} / finalize = {med[f'rank {b}'] / med['finalize']:.2f}")

    for graph, row in ((False, "step"), (True, "step graph")):
        steppers = {"without (parent's step)": RuleFrameStepper(pipe, 480, 640, use_graph=graph, tokens_in=True),
                    "with rank, best 50": RankedFrameStepper(pipe, 480, 640, use_graph=graph, tokens_in=True, best=50)}
        for st in steppers.values():
            for t in range(2):
                st.step(imgs[t], toks[t])
        ab_host(row, {v: (lambda st=st: st.step(imgs[2], toks[2])) for v, st in steppers.items()}, 100)

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
