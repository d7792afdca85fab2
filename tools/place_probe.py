#!/usr/bin/env python3
"""The online loop-closure entries (sslp_place_step, sslp_edge_log_step; libsslam_place.so) and the step that contains them beside
the step it extends - all in one process.

  1. THE LAUNCHES.  A place bank of capacity 4096, K = 500, d = 128, filled with planted raw sums (40 places in a cycle, plus
     noise) up to frame 613 and up to frame 4095; the timed frame shows its place again, so both picks are made.  Timed, ALTERNATELY:
       place 613 / 4095   the counter put back (one small device copy), then sslp_place_step of that frame: three launches
       similarity         sslam_sim_argmax_pairs over the 7 pairs of a step (five spacings, two candidates) at K = 500
       edge log           the counter put back, then sslp_edge_log_step of 7 slots
       copy               the small copy alone
  2. THE STEP.  ms per frame, tokens in (K = 500, G = 28, 640 x 480 frames and depth, 32 synthetic frames in a cycle, so that
     candidates exist from frame 30 on), of
       window          WindowPoseFrameStepper          five pairs: RANSAC, refinement, the window launch - the parent, untouched
       loops           LoopWindowPoseFrameStepper      the place step, seven pairs, the window launch, the edge log; capacity 4096
     as ordinary launches and from the captured graph.  The bank fills from 40 to 1440 frames while it is measured.
  3. close_loops() after 613 frames: the sparse graph over 613 nodes and 4291 slots, and its one read-back, by the host clock.
On synthetic frames the poses mean nothing as accuracy: the figures are times.

Protocol: every variant warmed, then `repeats` rounds taken alternately; a launch between device events around `reps` calls, a step
by the host clock around `frames` steps that end in a synchronise.  Printed: median and min - max over the rounds.
    tools/place_probe.py [--repeats 7] [--out FILE]      (profiles/online_loops.txt holds the output)"""
import ctypes as C
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import synth
from sslam_amd import evaluation, lib
from sslam_amd.online import LoopWindowPoseFrameStepper, WindowPoseFrameStepper
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

SPACINGS, K, D, CAP, E = (1, 5, 10, 15, 20), 500, 128, 4096, 7
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


emit(f"# sslp_place_step and sslp_edge_log_step, and the online steps; all measured; {torch.cuda.get_device_name(0)}")
ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
LP = lib.place()

# ---------------------------------------------------------------------------------------------------------------- 1. the launches
rng = np.random.default_rng(5)
places = rng.standard_normal((40, D))
raw = (50.0 + 8.0 * places[np.arange(CAP) % 40] + rng.standard_normal((CAP, D))).astype(np.float32)
scores = (0.1 + 0.9 * rng.random(K)).astype(np.float32)
scores_d = torch.from_numpy(scores).cuda()
banks, frames_in = {}, {}
for fill in (613, 4095):
    # the timed frame shows place fill % 40 again: its descriptors are that place's raw sum, shared out over the K scores, plus noise
    target = 50.0 + 8.0 * places[fill % 40]
    desc = ((target / scores.sum()) + 0.02 * rng.standard_normal((K, D))).astype(np.float32)
    frames_in[fill] = torch.from_numpy(desc).cuda()
    st = lib.alloc_place_state(CAP, D)
    st["raw"].copy_(torch.from_numpy(raw))
    st["sum"].copy_(torch.from_numpy(raw[:fill].sum(axis=0, dtype=np.float32)))
    st["t"].fill_(fill)
    banks[fill] = (st, st["t"].clone(), lib.alloc_place_out(2, D))
pws = torch.empty(lib.place_workspace_bytes(CAP), dtype=torch.uint8, device="cuda")
spare = torch.zeros((1,), dtype=torch.int32, device="cuda")


def place(fill):                                 # raw C-ABI calls: the wrappers' checks would be timed with launches this short
    st, kept, out = banks[fill]
    desc_d = frames_in[fill]

    def call():
        st["t"].copy_(kept)
        assert LP.sslp_place_step(*(ptr(st[k]) for k in lib.PLACE_STATE_KEYS), ptr(desc_d), ptr(scores_d), CAP, K, D, 30, C.c_float(0.3), 2, 5,
                                  ptr(pws), *(ptr(out[k]) for k in lib.PLACE_OUT_KEYS), stream) == 0
    return call


unit = rng.standard_normal((8, K, D)).astype(np.float32)
bank = torch.from_numpy(unit / np.linalg.norm(unit, axis=2, keepdims=True)).cuda()
pf = torch.tensor([0, 1, 2, 3, 4, 5, 6], dtype=torch.int32, device="cuda")
ps = torch.full((E,), 7, dtype=torch.int32, device="cuda")


def similarity():
    lib.sim_argmax_pairs(bank, pf, ps, want_s21=True)


log = lib.alloc_edge_log(CAP, E)
log["t"].fill_(613)
log_kept = log["t"].clone()
lo = {k: torch.zeros(shape, dtype=dt, device="cuda") for k, (shape, dt) in lib.edge_log_out_shapes(E).items()}
new = dict(first=torch.tensor([612, 608, 603, 598, 593, 40, 7], dtype=torch.int32, device="cuda"),
           T=torch.from_numpy(rng.standard_normal((E, 12))).cuda(), info=torch.from_numpy(rng.standard_normal((E, 21))).cuda(),
           status=torch.zeros(E, dtype=torch.int32, device="cuda"), inliers=torch.full((E,), 100, dtype=torch.int32, device="cuda"))


def edge_log():
    log["t"].copy_(log_kept)
    assert LP.sslp_edge_log_step(*(ptr(log[k]) for k in lib.EDGE_LOG_STATE_KEYS), ptr(new["first"]), ptr(new["T"]), ptr(new["info"]), ptr(new["status"]),
                                 ptr(new["inliers"]), E, 5, 12, 12, CAP, ptr(lo["logged"]), ptr(lo["status"]), stream) == 0


def copy():
    spare.copy_(log_kept)


calls = {"copy": copy, "place 613": place(613), "place 4095": place(4095), "similarity": similarity, "edge log": edge_log}
for fill in (613, 4095):
    calls[f"place {fill}"]()
    torch.cuda.synchronize()
    o = banks[fill][2]
    emit(f"# bank fill {fill}: status {int(o['status'])}, {int(o['count'])} picks {o['first'].tolist()} at {[round(float(x), 3) for x in o['sim']]}")
edge_log()
torch.cuda.synchronize()
emit(f"# edge log, frame 613, 7 slots: logged {lo['logged'].tolist()}, status {int(lo['status'])}")
reps = 50
for fn in calls.values():
    for _ in range(5):
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
med = {v: statistics.median(x) for v, x in us.items()}
for v in calls:
    emit(f"launch   {v:10s} median {med[v]:8.1f} us   min {min(us[v]):8.1f}   max {max(us[v]):8.1f}   ({reps} calls x {repeats} rounds)")
emit(f"launch   less the copy: place step {med['place 613'] - med['copy']:.1f} us at fill 613, {med['place 4095'] - med['copy']:.1f} us at fill 4095 "
     f"(three launches); edge log {med['edge log'] - med['copy']:.1f} us; the similarity launch of a step's 7 pairs {med['similarity']:.1f} us")

# -------------------------------------------------------------------------------------------------------------------- 2. the step
grid, n_frames, frames = 28, 32, 200
yy, xx = np.mgrid[0:480, 0:640]
depth = np.empty((n_frames, 480, 640), np.uint16)
drng = np.random.default_rng(31)
for f in range(n_frames):
    steps = drng.integers(0, 1500, (16, 21))[yy // 32, xx // 32]
    depth[f] = (7500 + 10 * f + 8.0 * xx + 4.0 * yy + steps).astype(np.uint16)
depth = torch.from_numpy(depth).cuda()
toks = torch.from_numpy(synth.token_sequence(n_frames, grid)).cuda()
image = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda")
cam, rule = evaluation.Camera(), MatchRule.mnn_ratio(0.9)
with torch.no_grad():
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * grid, num_keypoints=K), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    kw = dict(camera=cam, tokens_in=True, rule=rule, spacings=SPACINGS, threshold=12.0, huber=4.0)
    steppers = {}
    for graph in (False, True):
        mode = "graph" if graph else "launches"
        steppers[("window", mode)] = WindowPoseFrameStepper(pipe, 480, 640, 480, 640, use_graph=graph, **kw)
        steppers[("loops", mode)] = LoopWindowPoseFrameStepper(pipe, 480, 640, 480, 640, use_graph=graph, capacity=CAP, **kw)

    def run(key, n):
        st = steppers[key]
        for i in range(st.n_frames, st.n_frames + n):
            st.step(image, depth[i % n_frames], toks[i % n_frames])
        torch.cuda.synchronize()

    for key in steppers:
        run(key, 40)                                             # past the window's fill and the retrieval's min_gap
    ms = {key: [] for key in steppers}
    for _ in range(repeats):
        for key in steppers:
            t0 = time.perf_counter()
            run(key, frames)
            ms[key].append((time.perf_counter() - t0) / frames * 1e3)
    st = steppers[("loops", "graph")]
    lp, lg = st.place["out"], st.log["out"]
    emit(f"# the loop stepper's last frame ({st.n_frames} stepped): candidates {lp['first'].tolist()} at {[round(float(x), 3) for x in lp['sim']]}, "
         f"logged {lg['logged'].tolist()}, place status {int(lp['status'])}, log status {int(lg['status'])} (synthetic frames: no accuracy claim)")
    smed = {key: statistics.median(x) for key, x in ms.items()}
    for key in steppers:
        emit(f"step     {key[0]:7s} {key[1]:9s} median {smed[key]:7.3f} ms per frame   min {min(ms[key]):7.3f}   max {max(ms[key]):7.3f}   "
             f"({frames} frames x {repeats} rounds)")
    for mode in ("launches", "graph"):
        emit(f"step     {mode}: loops - window {smed[('loops', mode)] - smed[('window', mode)]:.3f} ms (the place step, two more pairs through the matcher "
             f"and the pose stage, the edge log)")

    # ------------------------------------------------------------------------------------------------------------ 3. close_loops
    st = LoopWindowPoseFrameStepper(pipe, 480, 640, 480, 640, use_graph=False, capacity=1024, **kw)
    for i in range(613):
        st.step(image, depth[i % n_frames], toks[i % n_frames])
    torch.cuda.synchronize()
    r = st.close_loops()
    took = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        st.close_loops()
        took.append((time.perf_counter() - t0) * 1e3)
    emit(f"# close_loops at 613 frames, {613 * E} slots: status {r['status']}, {r['iterations']} accepted, used {r['used_edges']}, "
         f"{len(r['loop_edges'])} loop edges, cg steps {r['cg_steps'][:max(1, r['iterations'] + 1)].tolist()}")
    emit(f"close    median {statistics.median(took):8.2f} ms   min {min(took):8.2f}   max {max(took):8.2f}   (one call x {repeats} rounds, the read-back included)")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
