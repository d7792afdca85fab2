"""include/sslam_place.h in numpy, for evaluation.PlaceBank and evaluation.EdgeLog: a front end without a GPU steps them once per
frame on the host and gets the device entries' bits.  Float32 throughout the place bank; the one operation numpy lacks, the fused
multiply-add, is made from float64 arithmetic (_fma32).  Nothing here goes through np.dot, @ or np.sum: the header fixes every
order of summation."""
from __future__ import annotations

import numpy as np

F32 = np.float32
_QUIET = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def _fma32(a, b, c):
    """fmaf(a, b, c), float32 operands: a * b + c rounded once.  The product of two float32 is exact in float64.  The float64 sum
    s = p + c comes with its exact error e (two-sum), so the exact value is s + e with |e| at most half an ulp of s.  Rounding s to
    float32 is then right unless s sits exactly half way between two float32 values: there e, not the ties-to-even rule, says
    which side the exact value is on."""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, F32).astype(np.float64), p.shape)
    s = p + c
    v = s - p
    e = (p - (s - v)) + (c - v)
    r = s.astype(F32)
    back = r.astype(np.float64)
    gap = s - back                                                   # exact: both are float64 and close
    toward = np.where(gap > 0, F32(np.inf), F32(-np.inf)).astype(F32)
    other = np.nextafter(r, toward)                                  # the float32 neighbour on s's side
    tie = np.isfinite(s) & (gap != 0) & (2.0 * gap == other.astype(np.float64) - back)
    away = tie & (e != 0) & ((e > 0) == (gap > 0))                   # the exact value lies past the half-way point
    return np.where(away, other, r).astype(F32)


def _wave_sum(x):
    """(..., d) -> (...): within each run of 64 the lanes by xor 32, 16, 8, 4, 2, 1, then the runs in ascending order."""
    x = np.asarray(x, F32)
    w = x.reshape(x.shape[:-1] + (x.shape[-1] // 64, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    total = w[..., 0, 0]
    for i in range(1, w.shape[-2]):
        total = total + w[..., i, 0]
    return total


def _normalised(c):
    norm = np.fmax(np.sqrt(_wave_sum(c * c)), F32(1e-12))
    return (c / norm[..., None]).astype(F32)


def fresh_place(capacity: int, d: int) -> dict:
    return {"t": np.zeros((), np.int32), "raw": np.zeros((capacity, d), F32), "sum": np.zeros(d, F32)}


def place_step(state: dict, desc, scores, min_gap: int, min_sim: float, per_frame: int, suppress: int) -> dict:
    """One frame of the place bank; state is updated in place.  -> first, second, sim (per_frame,), count, status (1,), sig (d,)."""
    capacity, d = state["raw"].shape
    t = int(state["t"])
    out = {"first": np.full(per_frame, -1, np.int32), "second": np.full(per_frame, -1, np.int32), "sim": np.zeros(per_frame, F32),
           "count": np.zeros(1, np.int32), "status": np.zeros(1, np.int32), "sig": np.zeros(d, F32)}
    if t < 0 or t >= capacity:
        out["status"][0] = 4
        return out
    desc, scores = np.asarray(desc, F32).reshape(-1, d), np.asarray(scores, F32).reshape(-1)
    with np.errstate(**_QUIET):
        column = np.zeros(d, F32)
        for weight, row in zip(scores, desc):
            column = _fma32(weight, row, column)
        state["raw"][t] = column
        state["sum"][:] = column + F32(0.0) if t == 0 else state["sum"] + column
        mean = state["sum"] / F32(t + 1)
        old = max(0, t - min_gap + 1)
        sig = _normalised(state["raw"][t] - mean)
        bank = _normalised(state["raw"][:old] - mean)
        sims = np.zeros(old, F32)
        for col in range(d):
            sims = _fma32(sig[col], bank[:, col], sims)
    out["sig"] = sig
    open_ = sims >= F32(min_sim)
    for slot in range(per_frame):
        where = np.flatnonzero(open_)
        if not len(where):
            break
        j = int(where[np.argmax(sims[where])])                      # argmax returns the first of equal values: the lowest j
        out["first"][slot], out["second"][slot], out["sim"][slot] = j, t, sims[j]
        out["count"][0] += 1
        open_[max(0, j - suppress):j + suppress + 1] = False
    state["t"][...] = t + 1
    return out


def fresh_log(capacity: int, n_slots: int) -> dict:
    rows = capacity * n_slots
    return {"t": np.zeros((), np.int32), "log_first": np.full(rows, -1, np.int32), "log_second": np.zeros(rows, np.int32),
            "log_T": np.zeros((rows, 12)), "log_info": np.zeros((rows, 21))}


def log_step(state: dict, slot_first, T, info, status, inliers, n_odometry: int, min_inliers: int, loop_min_inliers: int) -> dict:
    """One frame of the edge log; state is updated in place.  -> logged (E,), status (1,)."""
    slot_first = np.asarray(slot_first).reshape(-1)
    E = len(slot_first)
    capacity = len(state["log_first"]) // E
    t = int(state["t"])
    if t < 0 or t >= capacity:
        return {"logged": np.zeros(E, np.int32), "status": np.full(1, 4, np.int32)}
    T, info = np.asarray(T, np.float64).reshape(E, 12), np.asarray(info, np.float64).reshape(E, 21)
    need = np.where(np.arange(E) < n_odometry, min_inliers, loop_min_inliers)
    keep = (slot_first >= 0) & (slot_first < t) & (np.asarray(status).reshape(-1) != 3) & (np.asarray(inliers).reshape(-1) >= need) & \
        np.isfinite(T).all(axis=1) & np.isfinite(info).all(axis=1)
    rows = slice(t * E, (t + 1) * E)
    state["log_first"][rows] = np.where(keep, slot_first, -1)
    state["log_second"][rows] = t
    state["log_T"][rows] = np.where(keep[:, None], T, 0.0)
    state["log_info"][rows] = np.where(keep[:, None], info, 0.0)
    state["t"][...] = t + 1
    return {"logged": keep.astype(np.int32), "status": np.zeros(1, np.int32)}
