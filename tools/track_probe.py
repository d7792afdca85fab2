#!/usr/bin/env python3
"""The four entries of libsslam_track.so (feature tracks, the landmark map) beside the project's usual yardstick and beside the numpy
drop-in, and the step that contains sslt_track_step beside the step it extends - all in one process.

  1. THE LAUNCH GROUPS, on a planted sequence of 613 frames x 500 keypoints (612 spacing-1 rows; 9 in 10 keypoints of a frame are
     matched to the next, so tracks are ~10 frames long on average; planted poses, depths and keypoints).  Timed, ALTERNATELY:
       links        sslt_link_pairs: five launches              ids        sslt_track_ids: 5 + 10 launches
       landmarks    sslt_landmarks: two launches, one thread per track      step       sslt_track_step: one launch (counter put back)
       landmarks 8  the same launches over the same 306 500 keypoints with every eighth row's matches dropped: no track is longer than
                    8 frames - what the launch costs once no thread walks a long chain
       similarity   sslam_sim_argmax_pairs over the 612 spacing-1 pairs at K = 500, d = 128: the yardstick
       copy         the small copy that puts the step's counters back
     and, by the host clock, the numpy drop-in of each group (sslam_amd/track_numpy.py): the only baseline a new capability has.
  2. THE STEP.  ms per frame, tokens in (K = 500, G = 28, 640 x 480 frames and depth, 32 synthetic frames in a cycle), of
       window      WindowPoseFrameStepper           the parent, untouched
       tracks      TrackWindowPoseFrameStepper      and sslt_track_step, two bank copies, three small tensor ops
     as ordinary launches and from the captured graph.
On planted and synthetic data the figures are times, not accuracy.

Protocol: every variant warmed, then `repeats` rounds taken alternately; a launch group between device events around `reps` calls, a
step by the host clock around `frames` steps that end in a synchronise.  Printed: median and min - max over the rounds.
    tools/track_probe.py [--repeats 7] [--out FILE]      (profiles/feature_tracks.txt holds the output)"""
import ctypes as C
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-slam-master_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import synth
from sslam_amd import evaluation, lib
from sslam_amd import track_numpy as tn
from sslam_amd.online import TrackWindowPoseFrameStepper, WindowPoseFrameStepper
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

N, K, D = 613, 500, 128
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


emit(f"# libsslam_track.so: links, ids, landmarks, the online step; all measured; {torch.cuda.get_device_name(0)}")
ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
LT = lib.track()

# ------------------------------------------------------------------------------------------------------------ 1. the launch groups
rng = np.random.default_rng(11)
cam = evaluation.Camera()
first, second = np.arange(N - 1, dtype=np.int32), np.arange(1, N, dtype=np.int32)
perm = np.stack([rng.permutation(K) for _ in range(N)])
world = np.stack([rng.uniform(-1.5, 1.5, (N, K)), rng.uniform(-1.0, 1.0, (N, K)), rng.uniform(1.5, 4.0, (N, K))], axis=2)
seen = rng.random((N - 1, K)) < 0.9
matches, count = np.full((N - 1, K, 2), -1, np.int64), np.zeros(N - 1, np.int32)
for f in range(N - 1):
    j = np.flatnonzero(seen[f])
    matches[f, :len(j), 0], matches[f, :len(j), 1], count[f] = perm[f, j], perm[f + 1, j], len(j)
    world[f + 1, j] = world[f, j]                                # a matched keypoint keeps its scene point; an unmatched one starts another
Cw = np.tile(np.eye(3, 4), (N, 1, 1))
Cw[:, 0, 3] = 0.002 * np.arange(N) % 0.3
kp, depth = np.zeros((N, K, 2), np.float32), np.zeros((N, K), np.int32)
for f in range(N):
    X = world[f] + Cw[f, :, 3]
    kp[f, perm[f], 0], kp[f, perm[f], 1] = cam.fx * X[:, 0] / X[:, 2] + cam.cx, cam.fy * X[:, 1] / X[:, 2] + cam.cy
    depth[f, perm[f]] = np.rint(X[:, 2] * cam.depth_scale)
weight = (0.2 + 0.8 * rng.random((N, K))).astype(np.float32)
host = dict(first=first, second=second, matches=matches, count=count, kp=kp, depth=depth, C=Cw.reshape(N, 12), weight=weight)
dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}

links = lib.link_pairs(dev["first"], dev["second"], dev["matches"], dev["count"], N, K)
ws = torch.empty(lib.track_workspace_bytes(N, K), dtype=torch.uint8, device="cuda")
ids = lib.track_ids(links["prev"], links["prev_frame"], workspace=ws)
land = lib.landmarks(dev["kp"], dev["depth"], dev["C"], cam, links["next"], links["next_frame"], ids["root_frame"], ids["root_slot"],
                     ids["n_tracks"], dev["weight"])
torch.cuda.synchronize()
nt = int(ids["n_tracks"])
stats = tn.length_statistics(ids["length"].cpu().numpy(), [nt])
emit(f"# {N} frames x {K} keypoints, {int(count.sum())} listed matches: {nt} tracks, length mean {stats['mean']:.2f} median {stats['median']:.0f} "
     f"max {stats['max']}, {100 * stats['share_ge_2']:.1f} % of length >= 2; landmarks: status 0 in {int((land['status'][:nt] == 0).sum())}, "
     f"1 in {int((land['status'][:nt] == 1).sum())}, rms median {float(land['rms'][:nt].median()):.2e} px (planted: exact poses)")

count8 = dev["count"].clone()
count8[7::8] = 0
links8 = lib.link_pairs(dev["first"], dev["second"], dev["matches"], count8, N, K)
ids8 = lib.track_ids(links8["prev"], links8["prev_frame"])
land8 = lib.landmarks(dev["kp"], dev["depth"], dev["C"], cam, links8["next"], links8["next_frame"], ids8["root_frame"], ids8["root_slot"],
                      ids8["n_tracks"], dev["weight"])
torch.cuda.synchronize()
emit(f"# every eighth row dropped: {int(ids8['n_tracks'])} tracks, the longest {int(ids8['length'].max())}")

bank = lib.alloc_track_state(N, K)
for key in lib.LINK_KEYS:
    bank[key].copy_(links[key])
bank["track_id"].copy_(ids["track_id"]), bank["age"].copy_(ids["age"])
bank["next_frame"][N - 2] = -1                                   # the timed step is frame N - 1 again: its predecessor has no successor yet
counters = torch.tensor([N - 1, nt - int((ids["age"][N - 1] == 0).sum())], dtype=torch.int32, device="cuda")      # as they stood before frame N - 1
kept = counters.clone()
t_view, id_view = counters[0:1], counters[1:2]
sout = lib.alloc_track_out(K)
row_first = torch.tensor([N - 2], dtype=torch.int32, device="cuda")
m_row, c_row = dev["matches"][N - 2:N - 1], dev["count"][N - 2:N - 1]
spare = torch.zeros((2,), dtype=torch.int32, device="cuda")
doubles = [C.c_double(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.depth_scale, 1.0, 1.0, float(cam.width), float(cam.height), 3.0)]


def g_links():                                   # raw C-ABI calls: the wrappers' checks would be timed with launches this short
    assert LT.sslt_link_pairs(ptr(dev["first"]), ptr(dev["second"]), N - 1, ptr(dev["matches"]), ptr(dev["count"]), None, K, N, K,
                              *(ptr(links[k]) for k in lib.LINK_KEYS), stream) == 0


def g_ids():
    assert LT.sslt_track_ids(ptr(links["prev"]), ptr(links["prev_frame"]), N, K, ptr(ws), *(ptr(ids[k]) for k in lib.TRACK_ID_KEYS), stream) == 0


def g_landmarks():
    assert LT.sslt_landmarks(ptr(dev["kp"]), ptr(dev["depth"]), ptr(dev["C"]), N, K, *doubles, ptr(links["next"]), ptr(links["next_frame"]),
                             ptr(ids["root_frame"]), ptr(ids["root_slot"]), ptr(ids["n_tracks"]), ptr(dev["weight"]), 2,
                             *(ptr(land[k]) for k in lib.LANDMARK_KEYS), stream) == 0


def g_landmarks8():
    assert LT.sslt_landmarks(ptr(dev["kp"]), ptr(dev["depth"]), ptr(dev["C"]), N, K, *doubles, ptr(links8["next"]), ptr(links8["next_frame"]),
                             ptr(ids8["root_frame"]), ptr(ids8["root_slot"]), ptr(ids8["n_tracks"]), ptr(dev["weight"]), 2,
                             *(ptr(land8[k]) for k in lib.LANDMARK_KEYS), stream) == 0


def g_step():
    counters.copy_(kept)
    bank["next_frame"][N - 2:N - 1].fill_(-1)
    assert LT.sslt_track_step(ptr(t_view), ptr(id_view), *(ptr(bank[k]) for k in lib.TRACK_STATE_KEYS[2:]), ptr(m_row), ptr(c_row), None,
                              ptr(row_first), K, K, N, *(ptr(sout[k]) for k in lib.TRACK_OUT_KEYS), stream) == 0


def g_copy():
    spare.copy_(kept)
    bank["next_frame"][N - 2:N - 1].fill_(-1)


unit = rng.standard_normal((N, K, D)).astype(np.float32)
desc = torch.from_numpy(unit / np.linalg.norm(unit, axis=2, keepdims=True)).cuda()


def g_similarity():
    lib.sim_argmax_pairs(desc, dev["first"], dev["second"], want_s21=True)


calls = {"copy": g_copy, "links": g_links, "ids": g_ids, "landmarks": g_landmarks, "landmarks 8": g_landmarks8, "step": g_step,
         "similarity": g_similarity}
g_step()
torch.cuda.synchronize()
emit(f"# the timed step, frame {N - 1}: status {int(sout['status'])}, {int(sout['n_new'])} new tracks, ids equal the batch entries': "
     f"{bool(torch.equal(sout['track_id'], ids['track_id'][N - 1]))}")
reps = 20
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
med = {v: statistics.median(x) for v, x in us.items()}
for v in calls:
    emit(f"launch   {v:11s} median {med[v]:9.1f} us   min {min(us[v]):9.1f}   max {max(us[v]):9.1f}   ({reps} calls x {repeats} rounds)")
emit(f"launch   the step less the copy: {med['step'] - med['copy']:.1f} us")
for v in ("links", "ids", "landmarks", "landmarks 8"):
    emit(f"launch   {v} / similarity of the 612 pairs: {med[v] / med['similarity']:.3f}")

t0 = time.perf_counter()
h_links = tn.link_pairs(first, second, matches, count, None, N, K)
t1 = time.perf_counter()
h_ids = tn.track_ids(h_links["prev"], h_links["prev_frame"])
t2 = time.perf_counter()
h_land = tn.landmarks(kp, depth, host["C"], cam, h_links["next"], h_links["next_frame"], h_ids["root_frame"], h_ids["root_slot"], h_ids["n_tracks"], weight)
t3 = time.perf_counter()
hb = tn.TrackBank(N, K)
for f in range(N):
    hb.step(matches[max(f - 1, 0)], count[max(f - 1, 0)], None, f - 1)
t4 = time.perf_counter()
same = all(np.array_equal(h_links[k], links[k].cpu().numpy()) for k in lib.LINK_KEYS) and \
    all(np.array_equal(h_ids[k], ids[k].cpu().numpy()) for k in lib.TRACK_ID_KEYS) and \
    all(h_land[k].tobytes() == land[k].cpu().numpy().tobytes() for k in lib.LANDMARK_KEYS)
emit(f"# the numpy drop-in gives the device's bytes on this workload: {same}")
emit(f"host     numpy drop-in, one run by the host clock: links {1e3 * (t1 - t0):.1f} ms, ids {1e3 * (t2 - t1):.1f} ms, landmarks {1e3 * (t3 - t2):.1f} ms, "
     f"{N} bank steps {1e3 * (t4 - t3):.1f} ms ({1e6 * (t4 - t3) / N:.0f} us a step)")
emit(f"host     device / numpy: links {med['links'] / (1e6 * (t1 - t0)):.2e}, ids {med['ids'] / (1e6 * (t2 - t1)):.2e}, "
     f"landmarks {med['landmarks'] / (1e6 * (t3 - t2)):.2e}, step {(med['step'] - med['copy']) / (1e6 * (t4 - t3) / N):.2e}")

# -------------------------------------------------------------------------------------------------------------------- 2. the step
grid, n_frames, frames = 28, 32, 200
yy, xx = np.mgrid[0:480, 0:640]
dimg = np.empty((n_frames, 480, 640), np.uint16)
drng = np.random.default_rng(31)
for f in range(n_frames):
    steps = drng.integers(0, 1500, (16, 21))[yy // 32, xx // 32]
    dimg[f] = (7500 + 10 * f + 8.0 * xx + 4.0 * yy + steps).astype(np.uint16)
dimg = torch.from_numpy(dimg).cuda()
toks = torch.from_numpy(synth.token_sequence(n_frames, grid)).cuda()
image = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda")
with torch.no_grad():
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * grid, num_keypoints=K), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    kw = dict(camera=cam, tokens_in=True, rule=MatchRule.mnn_ratio(0.9), spacings=(1, 5, 10, 15, 20), threshold=12.0, huber=4.0)
    steppers = {}
    for graph in (False, True):
        mode = "graph" if graph else "launches"
        steppers[("window", mode)] = WindowPoseFrameStepper(pipe, 480, 640, 480, 640, use_graph=graph, **kw)
        steppers[("tracks", mode)] = TrackWindowPoseFrameStepper(pipe, 480, 640, 480, 640, use_graph=graph, **kw)

    def run(key, n):
        st = steppers[key]
        for i in range(st.n_frames, st.n_frames + n):
            st.step(image, dimg[i % n_frames], toks[i % n_frames])
        torch.cuda.synchronize()

    for key in steppers:
        run(key, 40)
    ms = {key: [] for key in steppers}
    for _ in range(repeats):
        for key in steppers:
            t0 = time.perf_counter()
            run(key, frames)
            ms[key].append((time.perf_counter() - t0) / frames * 1e3)
    st = steppers[("tracks", "graph")]
    o = st.tracks["out"]
    emit(f"# the track stepper's last frame ({st.n_frames} stepped): {int(o['n_new'])} new tracks, oldest age {int(o['age'].max())}, "
         f"status {int(o['status'])} (synthetic frames: no accuracy claim)")
    smed = {key: statistics.median(x) for key, x in ms.items()}
    for key in steppers:
        emit(f"step     {key[0]:7s} {key[1]:9s} median {smed[key]:7.3f} ms per frame   min {min(ms[key]):7.3f}   max {max(ms[key]):7.3f}   "
             f"({frames} frames x {repeats} rounds)")
    for mode in ("launches", "graph"):
        emit(f"step     {mode}: tracks - window {1e3 * (smed[('tracks', mode)] - smed[('window', mode)]):.1f} us "
             f"({smed[('tracks', mode)] / smed[('window', mode)]:.4f} of the parent's step)")
    took = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = st.landmarks(threshold=12.0)
        took.append((time.perf_counter() - t0) * 1e3)
    emit(f"landmarks() at {min(st.n_frames, st.capacity)} frames: {r['n_tracks']} tracks, median {statistics.median(took):.2f} ms   min {min(took):.2f}   "
         f"max {max(took):.2f}   (one call x {repeats} rounds, the read-back included)")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
