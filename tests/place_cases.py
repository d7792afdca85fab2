"""Seeded cases for the restatement (tests/place_ref.py), the numpy drop-ins and the device (tests/test_gpu_place.py) of
libsslam_place.so: descriptor banks planted as a few places plus noise, so that picks exist, with the rows of the contract among
them - bit-identical frames, frames that copy earlier ones, a NaN score - and the edge log's contract rows.  Case generation uses
np.linalg freely: nothing here is what the device computes.
No torch, no GPU: importable anywhere."""
from __future__ import annotations

import functools

import numpy as np

import place_ref as ref


# ------------------------------------------------------------------------------------------------------------- the place bank
def planted_bank(n, k, d, seed, period, noise=0.35):
    """(desc (n, k, d), scores (n, k)) float32: every descriptor is a part all frames share, the frame's place (frame i shows place
    i % period) and noise, normalised; scores in (0.1, 1)."""
    rng = np.random.default_rng(7000 + seed)
    common, places = rng.standard_normal(d), rng.standard_normal((period, d))
    desc = common + 0.6 * places[np.arange(n) % period][:, None, :] + noise * rng.standard_normal((n, k, d))
    desc = (desc / np.linalg.norm(desc, axis=2, keepdims=True)).astype(np.float32)
    scores = (0.1 + 0.9 * rng.random((n, k))).astype(np.float32)
    return np.ascontiguousarray(desc), scores


def bank_case(name, desc, scores, capacity, min_gap, min_sim, per_frame, suppress, **notes):
    return dict(name=name, desc=desc, scores=scores, capacity=capacity, min_gap=min_gap, min_sim=min_sim, per_frame=per_frame, suppress=suppress,
                **notes)


def _three_frames():
    """d = 128, k = 1, capacity 3: five frames are stepped, the last two find the bank full."""
    desc, scores = planted_bank(5, 1, 128, 1, 2)
    return bank_case("capacity_3_k_1", desc, scores, 3, 1, -2.0, 1, 0)


def _seventy_frames():
    """d = 256, k = 3, 70 frames - past two groups of 32 -, eight picks a frame, no suppression.  Frame 11 is frame 10 bit for bit:
    every later frame sees the two at equal similarity and lists 10 before 11."""
    desc, scores = planted_bank(70, 3, 256, 2, 9)
    desc[11], scores[11] = desc[10], scores[10]
    return bank_case("frames_70_d_256", desc, scores, 70, 5, 0.0, 8, 0, twins=(10, 11))


def _three_hundred_frames():
    """d = 128, k = 5, 300 frames - past one stride of the pick's 256 threads -: 200 frames, then the first 100 again, bit for bit,
    so frame i >= 200 has frame i - 200 as its first pick."""
    desc, scores = planted_bank(200, 5, 128, 3, 23)
    desc, scores = np.concatenate([desc, desc[:100]]), np.concatenate([scores, scores[:100]])
    return bank_case("frames_300_copies", desc, scores, 300, 30, 0.3, 2, 5, copies=(200, 200))


def _wide_frames():
    """d = 128, k = 500 - the extraction's keypoint count -, 40 frames."""
    desc, scores = planted_bank(40, 500, 128, 4, 8)
    return bank_case("frames_40_k_500", desc, scores, 64, 5, 0.3, 2, 2)


def _nan_score():
    """One NaN score at frame 8: its raw sum is NaN, and so is the running sum from then on - as the batch mean is for any prefix
    that holds the frame.  Before it picks exist; from it on nothing is eligible, nothing is picked, and every sim is +0.0."""
    desc, scores = planted_bank(14, 4, 128, 5, 3)
    scores[8, 2] = np.nan
    return bank_case("nan_score_at_8", desc, scores, 14, 2, -1.0, 2, 0, nan_from=8)


@functools.lru_cache(maxsize=None)
def _banks():
    return {c["name"]: c for c in (_three_frames(), _seventy_frames(), _three_hundred_frames(), _wide_frames(), _nan_score())}


BANK_NAMES = ("capacity_3_k_1", "frames_70_d_256", "frames_300_copies", "frames_40_k_500", "nan_score_at_8")


def bank(name):
    return _banks()[name]


@functools.lru_cache(maxsize=None)
def bank_expected(name):
    """(the steps' outputs, the final state) of the restatement for the named bank: computed once, shared, not to be written to."""
    c = bank(name)
    return ref.run(c["desc"], c["scores"], c["capacity"], c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"])


# --------------------------------------------------------------------------------------------------------------- the edge log
def log_case(name, n_steps, n_slots, n_odometry, seed, capacity=None, min_inliers=12, loop_min_inliers=12):
    """Per step: slot_first (E,), T (E, 12), info (E, 21), status, inliers (E,).  Odometry slot e looks e + 1 frames back; a loop
    slot names a frame of the first half once t is in the second."""
    rng = np.random.default_rng(8000 + seed)
    E = n_slots
    first = np.full((n_steps, E), -1, np.int32)
    for t in range(n_steps):
        for e in range(E):
            if e < n_odometry:
                first[t, e] = t - (e + 1) if t >= e + 1 else -1
            elif t >= n_steps // 2:
                first[t, e] = rng.integers(0, n_steps // 2)
    return dict(name=name, slot_first=first, T=rng.standard_normal((n_steps, E, 12)), info=rng.standard_normal((n_steps, E, 21)),
                status=rng.integers(0, 3, (n_steps, E)).astype(np.int32), inliers=rng.integers(20, 200, (n_steps, E)).astype(np.int32),
                n_odometry=n_odometry, min_inliers=min_inliers, loop_min_inliers=loop_min_inliers, capacity=n_steps if capacity is None else capacity)


def _changed(case, name, **changes):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    out["name"] = name
    for key, (where, value) in changes.items():
        out[key][where] = value
    return out


def log_cases():
    """The contract's rows: each reason a slot is refused, slot_first >= t, the two thresholds on either side of n_odometry, a full
    log; and the shapes: one slot, sixteen slots, no odometry slot, no loop slot."""
    base = log_case("base", 10, 4, 2, 1)                       # slots 0, 1 odometry, 2, 3 loops
    return [base,
            _changed(base, "status_3", status=((7, 1), 3)),
            _changed(base, "status_3_loop", status=((7, 3), 3)),
            _changed(base, "nan_in_T", T=((6, 0, 11), np.nan)),
            _changed(base, "inf_in_info", info=((8, 2, 0), -np.inf)),
            _changed(base, "first_is_t", slot_first=((5, 2), 5)),
            _changed(base, "first_past_t", slot_first=((5, 3), 9)),
            _changed(base, "first_below_minus_1", slot_first=((6, 1), -7)),
            dict(_changed(base, "thresholds", inliers=((slice(None),), np.tile(np.array([29, 30, 49, 50], np.int32), (10, 1)))),
                 min_inliers=30, loop_min_inliers=50),
            dict(base, name="full_log", capacity=6),
            log_case("one_slot", 5, 1, 1, 2),
            log_case("sixteen_slots", 44, 16, 5, 3),           # two windows' worth of steps at the default window of 21
            log_case("loops_only", 8, 3, 0, 4),
            log_case("odometry_only", 8, 3, 3, 5)]


@functools.lru_cache(maxsize=None)
def _logs():
    return {c["name"]: c for c in log_cases()}


LOG_NAMES = tuple(c["name"] for c in log_cases())


def log(name):
    return _logs()[name]


def run_log(c, state=None):
    state = ref.fresh_log(c["capacity"], c["slot_first"].shape[1]) if state is None else state
    outs = [ref.log_step(state, c["slot_first"][t], c["T"][t], c["info"][t], c["status"][t], c["inliers"][t], c["n_odometry"], c["min_inliers"],
                         c["loop_min_inliers"]) for t in range(len(c["T"]))]
    return outs, state


@functools.lru_cache(maxsize=None)
def log_expected(name):
    """(the steps' outputs, the final state) of the restatement for the named log case: computed once, shared, not to be written to."""
    return run_log(log(name))
