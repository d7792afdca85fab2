"""A numpy restatement of libsslam_place.so (csrc_place/place.hip), written from the contract in include/sslam_place.h: one frame of
the growing place bank in float32 - the fused multiply-add and the wave-order sum are tests/loop_ref.py's fmaf32 and wave_sum32,
imported, not copied, since the header takes both from sslam_loop.h by name - and one frame of the edge log.  The step is stated
as the header states it, frame by frame on a running sum; that it gives row t of the batch entries run on the frames 0 .. t is what
tests/test_place_cpu.py checks, not what this file assumes.

Tolerance: NONE - both sides take the same correctly rounded operations in one order.
No torch, no GPU: importable anywhere."""
from __future__ import annotations

import numpy as np

from loop_ref import fmaf32, wave_sum32

MAX_CAPACITY, MAX_K, MAX_PER_FRAME, MAX_SLOTS = 4096, 4096, 8, 16
FRAMES_PER_GROUP = 32
STATE_KEYS = ("t", "raw", "sum")
OUT_KEYS = ("first", "second", "sim", "count", "status", "sig")
LOG_STATE_KEYS = ("t", "log_first", "log_second", "log_T", "log_info")
LOG_OUT_KEYS = ("logged", "status")
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


# ------------------------------------------------------------------------------------------------------------- the place bank
def fresh_state(capacity, d):
    """t = 0; nothing else is read before it is written (zeros here)."""
    return dict(t=np.zeros((), np.int32), raw=np.zeros((capacity, d), np.float32), sum=np.zeros(d, np.float32))


def _absent(per_frame, d):
    return dict(first=np.full(per_frame, -1, np.int32), second=np.full(per_frame, -1, np.int32), sim=np.zeros(per_frame, np.float32),
                count=np.zeros(1, np.int32), status=np.full(1, 4, np.int32), sig=np.zeros(d, np.float32))


def _unit(c):
    """c (..., d) float32 -> c / fmaxf(sqrtf(ss), 1e-12f), ss in the wave order."""
    ss = wave_sum32(c * c)
    return (c / np.fmax(np.sqrt(ss), np.float32(1e-12))[..., None]).astype(np.float32)


def step(state, desc, scores, min_gap=30, min_sim=0.3, per_frame=2, suppress=5):
    """One frame: `state` is updated in place; -> dict of OUT_KEYS as the device writes them."""
    capacity, d = state["raw"].shape
    t = int(state["t"])
    if not 0 <= t < capacity:
        return _absent(per_frame, d)
    desc, scores = np.asarray(desc, np.float32).reshape(-1, d), np.asarray(scores, np.float32).reshape(-1)
    with np.errstate(**_ERR):
        acc = np.zeros(d, np.float32)
        for kk in range(len(scores)):
            acc = fmaf32(scores[kk], desc[kk], acc)
        state["raw"][t] = acc
        state["sum"][...] = (np.zeros(d, np.float32) if t == 0 else state["sum"]) + acc
        mean = state["sum"] / np.float32(t + 1)
        sig_t = _unit(state["raw"][t] - mean)
        m = max(0, t - min_gap + 1)
        sig_j = _unit(state["raw"][:m] - mean)
        S = np.zeros(m, np.float32)
        for c in range(d):
            S = fmaf32(sig_t[c], sig_j[:, c], S)
    out = _absent(per_frame, d)
    out["status"][0], out["sig"] = 0, sig_t
    live = S >= np.float32(min_sim)
    for s in range(per_frame):
        if not live.any():
            break
        best = np.where(live, S, -np.inf).max()
        j = int(np.flatnonzero(live & (S == best))[0])
        out["first"][s], out["second"][s], out["sim"][s] = j, t, S[j]
        out["count"][0] += 1
        live[max(0, j - suppress):j + suppress + 1] = False
    state["t"][...] = t + 1
    return out


def run(desc, scores, capacity, min_gap, min_sim, per_frame, suppress, state=None):
    """Every frame of a bank (n, k, d) through step(): (list of the steps' outputs, the final state)."""
    state = fresh_state(capacity, desc.shape[2]) if state is None else state
    return [step(state, desc[i], scores[i], min_gap, min_sim, per_frame, suppress) for i in range(len(desc))], state


# --------------------------------------------------------------------------------------------------------------- the edge log
def fresh_log(capacity, n_slots):
    rows = capacity * n_slots
    return dict(t=np.zeros((), np.int32), log_first=np.full(rows, -1, np.int32), log_second=np.zeros(rows, np.int32),
                log_T=np.zeros((rows, 12)), log_info=np.zeros((rows, 21)))


def log_step(state, slot_first, T, info, status, inliers, n_odometry, min_inliers=12, loop_min_inliers=12):
    """One frame's E slots: `state` is updated in place; -> dict of LOG_OUT_KEYS."""
    E = len(slot_first)
    capacity = len(state["log_first"]) // E
    t = int(state["t"])
    if not 0 <= t < capacity:
        return dict(logged=np.zeros(E, np.int32), status=np.full(1, 4, np.int32))
    T, info = np.asarray(T, np.float64).reshape(E, 12), np.asarray(info, np.float64).reshape(E, 21)
    logged = np.zeros(E, np.int32)
    for e in range(E):
        a, need = int(slot_first[e]), (min_inliers if e < n_odometry else loop_min_inliers)
        ok = 0 <= a < t and int(status[e]) != 3 and int(inliers[e]) >= need and bool(np.isfinite(T[e]).all() and np.isfinite(info[e]).all())
        row = t * E + e
        logged[e] = ok
        state["log_first"][row], state["log_second"][row] = (a if ok else -1), t
        state["log_T"][row], state["log_info"][row] = (T[e], info[e]) if ok else (0.0, 0.0)
    state["t"][...] = t + 1
    return dict(logged=logged, status=np.zeros(1, np.int32))
