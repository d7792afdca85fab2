#!/usr/bin/env python3
"""The sliding-window launch (sslw_window_step, libsslam_window.so) beside the banded pose-graph launch on the same operands, and the
online step that contains it beside the two steps it extends - all in one process.

  1. THE LAUNCH.  A planted 120-frame trajectory at the spacings 1, 5, 10, 15, 20 with 3 % outliers (tests/window_cases.py) is
     stepped to frame 60 through a window of 21 frames; the state is kept.  Timed, ALTERNATELY:
       window N        the counter and ring_C put back (two small device copies), then sslw_window_step of frame 60, N steps at most
       banded N        the same two copies (into spares), then sslg_pose_graph on the window-local operands of that frame (21 nodes,
                       105 slots, band 20), N steps at most - the dense LDS solve against the banded one that streams its factor
                       through the workspace
       copies          the two copies alone
     The two launches' C, status, iterations, costs and edge_chi2 are compared bit for bit before anything is timed.  Either
     launch is ONE 256-thread workgroup: the figure is a latency.
  2. THE STEP.  ms per frame, tokens in (K = 500, G = 28, 640 x 480 frames and depth), of
       rule            RuleFrameStepper(spacings=...)            the matcher over the five spacings
       pose            PoseFrameStepper(refine=True)             one pair: RANSAC 256 and 5 refinement steps
       window          WindowPoseFrameStepper                    five pairs: RANSAC, refinement, the window launch
     as ordinary launches and from the captured graph.  The first two are the parent's code, untouched.  On synthetic frames the
     poses mean nothing as accuracy: the figures are times.

Protocol: every variant warmed, then `repeats` rounds taken alternately; the launch between device events around `reps` calls, the
step by the host clock around `frames` steps that end in a synchronise.  Printed: median and min - max over the rounds.
    tools/window_probe.py [--repeats 7] [--out FILE]      (profiles/window_step.txt holds the output)"""
import ctypes as C
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import synth
import window_cases as wc
import window_ref as ref
from sslam_amd import evaluation, lib
from sslam_amd.online import PoseFrameStepper, RuleFrameStepper, WindowPoseFrameStepper
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

W, SPACINGS, FRAME, CHI = 21, wc.SPACINGS, 60, 4.0
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


emit(f"# sslw_window_step beside sslg_pose_graph, and the online steps; all measured; {torch.cuda.get_device_name(0)}")

# ------------------------------------------------------------------------------------------------------------------ 1. the launch
S = len(SPACINGS)
case = wc.window_case("probe", W, SPACINGS, 120, 0, outliers=0.03)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
sp = dev(case["spacings"])
state, host = lib.alloc_window_state(W, S, 120), ref.fresh_state(W, S, 120)
ws = torch.empty(lib.window_workspace_bytes(1, W, S), dtype=torch.uint8, device="cuda")
for i in range(FRAME):
    lib.window_step(state, sp, *(dev(case[k][i]) for k in ("T", "info", "status", "inliers")), None, 12, CHI, 0.0, 2, workspace=ws)
    ref.step(host, case["spacings"], case["T"][i], case["info"][i], case["status"][i], case["inliers"][i])
torch.cuda.synchronize()
assert all(np.array_equal(state[k].cpu().numpy()[0].view(np.int64 if state[k].dtype == torch.float64 else np.int32),
                          host[k].view(np.int64 if host[k].dtype == np.float64 else np.int32)) for k in ref.STATE_KEYS), "the state is the restatement's"
kept_t, kept_C = state["t"].clone(), state["ring_C"].clone()
spare_t, spare_C = torch.zeros_like(kept_t), torch.zeros_like(kept_C)
new = [dev(case[k][FRAME]) for k in ("T", "info", "status", "inliers")]
local = ref.step({k: v.copy() for k, v in host.items()}, case["spacings"], case["T"][FRAME], case["info"][FRAME], case["status"][FRAME],
                 case["inliers"][FRAME], detail=True)["local"]
loc = [dev(local[k]) for k in ("first", "second", "T", "info", "C_in")]
gws = torch.empty(lib.pose_graph_workspace_bytes(1, W, W - 1), dtype=torch.uint8, device="cuda")
wout = {n: lib.alloc_window_out(W, S) for n in (1, 2)}
gshapes = lib.pose_graph_shapes(1, W, W * S)
gout = {n: tuple(torch.zeros(gshapes[k][0], dtype=gshapes[k][1], device="cuda") for k in lib.POSE_GRAPH_KEYS) for n in (1, 2)}


LW, LG = lib.window(), lib.graph()
ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def window(n):                                   # raw C-ABI calls: the wrappers' checks would be timed with a launch this short
    def call():
        state["t"].copy_(kept_t)
        state["ring_C"].copy_(kept_C)
        assert LW.sslw_window_step(*(ptr(state[k]) for k in lib.WINDOW_STATE_KEYS), ptr(sp), *(ptr(x) for x in new), None, 1, W, S, 12,
                                   C.c_double(CHI), C.c_double(0.0), n, 120, ptr(ws), *(ptr(wout[n][k]) for k in lib.WINDOW_OUT_KEYS), stream) == 0
    return call


def banded(n):
    def call():
        spare_t.copy_(kept_t)
        spare_C.copy_(kept_C)
        assert LG.sslg_pose_graph(*(ptr(x) for x in loc[:4]), 1, W, W * S, ptr(loc[4]), W - 1, C.c_double(CHI), C.c_double(0.0), n, ptr(gws),
                                  *(ptr(x) for x in gout[n]), stream) == 0
    return call


def copies():
    spare_t.copy_(kept_t)
    spare_C.copy_(kept_C)


for n in (1, 2):
    window(n)(), banded(n)()
    torch.cuda.synchronize()
    g = dict(zip(lib.POSE_GRAPH_KEYS, gout[n]))
    assert torch.equal(bits(wout[n]["C_window"]), bits(g["C"])), "the dense solve gives the banded statement's bits"
    for k in ("status", "iterations", "used_edges", "failed_row", "cost_in", "cost", "edge_chi2"):
        assert torch.equal(bits(wout[n][k]), bits(g[k])), k
    emit(f"# frame {FRAME}, window {W}, {S} spacings: {int(g['used_edges'])} used of {W * S} slots, {int(wout[n]['dropped_edges'])} dropped; "
         f"n_iter {n}: status {int(g['status'])}, {int(g['iterations'])} accepted; window and banded agree bit for bit")

calls = {"copies": copies}
for n in (1, 2):
    calls[f"window {n}"], calls[f"banded {n}"] = window(n), banded(n)
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
for n in (1, 2):
    emit(f"launch   n_iter {n}: window {med[f'window {n}'] - med['copies']:.1f} us, banded {med[f'banded {n}'] - med['copies']:.1f} us less the copies; "
         f"banded / window {(med[f'banded {n}'] - med['copies']) / (med[f'window {n}'] - med['copies']):.2f}")

# -------------------------------------------------------------------------------------------------------------------- 2. the step
grid, K, n_frames, frames = 28, 500, 32, 200
rng = np.random.default_rng(31)
yy, xx = np.mgrid[0:480, 0:640]
depth = np.empty((n_frames, 480, 640), np.uint16)
for f in range(n_frames):
    steps = rng.integers(0, 1500, (16, 21))[yy // 32, xx // 32]
    depth[f] = (7500 + 10 * f + 8.0 * xx + 4.0 * yy + steps).astype(np.uint16)
depth = torch.from_numpy(depth).cuda()
toks = torch.from_numpy(synth.token_sequence(n_frames, grid)).cuda()
image = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda")
cam, rule = evaluation.Camera(), MatchRule.mnn_ratio(0.9)
with torch.no_grad():
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * grid, num_keypoints=K), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    steppers = {}
    for graph in (False, True):
        mode = "graph" if graph else "launches"
        steppers[("rule", mode)] = RuleFrameStepper(pipe, 480, 640, use_graph=graph, tokens_in=True, spacings=SPACINGS, rule=rule)
        steppers[("pose", mode)] = PoseFrameStepper(pipe, 480, 640, 480, 640, camera=cam, use_graph=graph, tokens_in=True, rule=rule, threshold=12.0,
                                                    refine=True, huber=4.0)
        steppers[("window", mode)] = WindowPoseFrameStepper(pipe, 480, 640, 480, 640, camera=cam, use_graph=graph, tokens_in=True, rule=rule,
                                                            spacings=SPACINGS, threshold=12.0, huber=4.0)

    def run(key, n):
        st = steppers[key]
        for i in range(n):
            if key[0] == "rule":
                st.step(image, toks[i % n_frames])
            else:
                st.step(image, depth[i % n_frames], toks[i % n_frames])
        torch.cuda.synchronize()

    for key in steppers:
        run(key, 40)                                             # past the window's fill: every later step holds 21 frames
    ms = {key: [] for key in steppers}
    for _ in range(repeats):
        for key in steppers:
            t0 = time.perf_counter()
            run(key, frames)
            ms[key].append((time.perf_counter() - t0) / frames * 1e3)
w = steppers[("window", "graph")].win["out"]
emit(f"# the window stepper's last frame: n_nodes {int(w['n_nodes'])}, admitted {w['admitted'][0].tolist()}, used {int(w['used_edges'])}, "
     f"status {int(w['status'])}, {int(w['iterations'])} accepted, lost {int(w['lost'])} (synthetic frames: no accuracy claim)")
smed = {key: statistics.median(x) for key, x in ms.items()}
for key in steppers:
    emit(f"step     {key[0]:7s} {key[1]:9s} median {smed[key]:7.3f} ms per frame   min {min(ms[key]):7.3f}   max {max(ms[key]):7.3f}   "
         f"({frames} frames x {repeats} rounds)")
for mode in ("launches", "graph"):
    emit(f"step     {mode}: window - rule {smed[('window', mode)] - smed[('rule', mode)]:.3f} ms (the pose stage over five pairs and the window), "
         f"window - pose {smed[('window', mode)] - smed[('pose', mode)]:.3f} ms")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
