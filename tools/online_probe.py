import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np, torch, synth
from sslam_amd import lib
from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
from sslam_amd.online import FrameStepper
from sslam_amd.vit import DinoV3ViT
dev = torch.device("cuda", 0)
torch.manual_seed(0)
n = 6
imgs = torch.from_numpy(synth.image_sequence(n)).to(dev)
toks = torch.from_numpy(synth.token_sequence(n, 28)).to(dev)
pipe = SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0), device=dev)


def multi_spacing_leg(reps=60):
    """The pair-list matcher and FrameStepper(spacings=...).  Table 1: the 612 consecutive pairs of the 613-frame workload through
    match(spacing=1) and through match_pairs(first = arange, second = arange + 1), alternating, one device-event timing per call.
    Table 2: ms per frame, tokens in, of the five reference spacings - StreamingSequence in ring mode pushed one frame at a time,
    the multi-spacing stepper as launches and from its graph - beside the one-spacing stepper; every caller warm and in its steady
    state (all spacings present), a pass of 27 frames per timing, taken alternately.  Medians; clocks as found."""
    import statistics
    from sslam_amd.harness import StreamingSequence
    med = statistics.median
    sp = (1, 5, 10, 15, 20)
    big = pipe.extract(torch.from_numpy(synth.token_sequence(613, 28)).to(dev))
    d, sc = big["descriptors"], big["scores"]
    first = torch.arange(612, dtype=torch.int32, device=dev)
    second = first + 1
    calls = {"match(spacing=1)": lambda: pipe.match(d, sc, None, spacing=1),
             "match_pairs(arange, arange + 1)": lambda: pipe.match_pairs(d, sc, None, first=first, second=second)}
    a, b = calls.values()
    assert all(torch.equal(x, y) for x, y in zip(a().values(), b().values())), "the two calls must give the same rows"
    ms = {k: [] for k in calls}
    for r in range(5 + reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            if r >= 5: ms[k].append(e0.elapsed_time(e1))
    print("612 pairs of 500 x 500 x 128 (613 frames), sim_argmax + finalize, ms per call over %d alternating calls:" % reps)
    for k, v in ms.items():
        print("   %-34s median %.4f   min %.4f   max %.4f" % (k, med(v), min(v), max(v)))
    del big, d, sc

    m = 27
    im, tk = torch.from_numpy(synth.image_sequence(m)).to(dev), torch.from_numpy(synth.token_sequence(m, 28)).to(dev)
    ring = StreamingSequence(pipe, sp)
    callers = {"StreamingSequence ring, one frame per push (5 launch pairs)": lambda i: ring.push(tk[i:i + 1], im[i:i + 1])}
    for graph in (False, True):
        multi = FrameStepper(pipe, 480, 640, use_graph=graph, tokens_in=True, spacings=sp)
        one = FrameStepper(pipe, 480, 640, use_graph=graph, tokens_in=True)
        callers["FrameStepper spacings=%s graph %s" % (sp, graph)] = lambda i, st=multi: st.step(im[i], tk[i])
        callers["FrameStepper one spacing graph %s" % graph] = lambda i, st=one: st.step(im[i], tk[i])
    launches = {}
    for k, fn in callers.items():
        for _ in range(3):
            for i in range(m): fn(i)
        n0 = lib.launch_count(); fn(0); launches[k] = lib.launch_count() - n0
    torch.cuda.synchronize()
    ms = {k: [] for k in callers}
    for _ in range(reps):
        for k, fn in callers.items():
            t0 = time.perf_counter()
            for i in range(m): fn(i)
            torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / m * 1e3)
    print("ms per frame, tokens in, steady state, %d alternating passes of %d frames:" % (reps, m))
    for k, v in ms.items():
        print("   %-62s median %.4f   min %.4f   max %.4f   library calls per frame %d" % (k, med(v), min(v), max(v), launches[k]))


if "--multi-spacing" in sys.argv:          # this leg alone
    multi_spacing_leg()
    sys.exit(0)
want = pipe.run(imgs, tokens=toks)
def run_stepper(st, with_tokens):
    res = []
    for i in range(n):
        n0 = lib.launch_count()
        o = st.step(imgs[i], toks[i] if with_tokens else None)
        res.append(({k: (v.clone() if v is not None else None) for k, v in o.items()}, lib.launch_count() - n0))
    return res
for graph in (False, True):
    st = FrameStepper(pipe, 480, 640, use_graph=graph, tokens_in=True)
    res = run_stepper(st, True)
    ok = True
    for i, (o, nl) in enumerate(res):
        for k in ("idx", "descriptors", "intensity", "scores", "saliency"):
            ok &= torch.equal(o[k], want[k][i])
        if i:
            c = int(o["match_count"]); ok &= c == int(want["match_count"][i - 1]) and torch.equal(o["matches"][:c], want["matches"][i - 1][:c]) and torch.equal(o["quality"][:c], want["quality"][i - 1][:c])
    print("tokens-in graph", graph, "equal to batch run:", ok, "launches per step:", [nl for _, nl in res])
    def t():
        for i in range(n): st.step(imgs[i], toks[i])
    for _ in range(5): t()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(50): t()
    torch.cuda.synchronize(); print("   ms per step (async, back to back): %.4f" % ((time.perf_counter() - t0) / 50 / n * 1e3))
    t0 = time.perf_counter()
    for _ in range(50):
        for i in range(n):
            o = st.step(imgs[i], toks[i]); int(o["match_count"]) if o["match_count"] is not None else None
    print("   ms per step (caller reads the count each frame): %.4f" % ((time.perf_counter() - t0) / 50 / n * 1e3))
for prec, vit_form in (("bf16", None), ("bf16", "few_frame"), ("fp32", None)):
    torch.manual_seed(0)
    pv = SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0), device=dev, vit=DinoV3ViT().to(dev).eval(), vit_precision=prec,
                          vit_form=vit_form)
    prec = prec + (" " + vit_form if vit_form else "")
    wantv = pv.run(imgs)
    outs = {}
    for graph in (False, True):
        st = FrameStepper(pv, 480, 640, use_graph=graph)
        res = run_stepper(st, False)
        outs[graph] = res
        ok = all(torch.equal(o[k], wantv[k][i]) for i, (o, _) in enumerate(res) for k in ("idx", "descriptors", "intensity"))
        print(prec, "ViT inside, graph", graph, "equal to batch run:", ok, "launches per step:", [nl for _, nl in res])
        def t():
            for i in range(n): st.step(imgs[i])
        for _ in range(5): t()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(30): t()
        torch.cuda.synchronize(); print("   ms per step (async): %.4f" % ((time.perf_counter() - t0) / 30 / n * 1e3))
        t0 = time.perf_counter()
        for _ in range(30):
            for i in range(n):
                o = st.step(imgs[i]); int(o["match_count"]) if o["match_count"] is not None else None
        print("   ms per step (count read each frame): %.4f" % ((time.perf_counter() - t0) / 30 / n * 1e3))
    same = all(torch.equal(a[0][k], b[0][k]) for a, b in zip(outs[False], outs[True]) for k in ("idx", "descriptors", "intensity", "scores"))
    print("   graph == eager stepping:", same)

# A/B of the bf16 ViT's forms inside the step: every stepper warm first, then five repeats per (vit_form, graph) taken alternately
import statistics
torch.manual_seed(0)
dv = DinoV3ViT().to(dev).eval()
steppers = {}
for vit_form in (None, "few_frame"):
    pv = SequencePipeline(ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0), device=dev, vit=dv, vit_precision="bf16", vit_form=vit_form)
    for graph in (False, True):
        steppers[(vit_form, graph)] = FrameStepper(pv, 480, 640, use_graph=graph)
def block(st, rounds):
    for _ in range(rounds):
        for i in range(n): st.step(imgs[i])
for st in steppers.values(): block(st, 5)
torch.cuda.synchronize()
ms = {k: [] for k in steppers}
for _ in range(5):
    for k, st in steppers.items():
        block(st, 1); torch.cuda.synchronize(); t0 = time.perf_counter()
        block(st, 30); torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / 30 / n * 1e3)
print("bf16 ViT inside the step, ms per frame (async), five alternating repeats and their median:")
for (vit_form, graph), v in ms.items():
    print("   vit_form %-9s graph %-5s median %.4f   repeats %s" % (vit_form, graph, statistics.median(v), " ".join("%.4f" % x for x in v)))
multi_spacing_leg()
