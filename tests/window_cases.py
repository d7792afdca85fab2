"""Cases for the sliding-window estimator: the per-frame inputs of sslw_window_step (what sslam_pose_refine_pairs writes for the S
pairs of a frame) cut from the planted graphs of tests/pose_graph_cases.py, for the restatement (tests/window_ref.py), the numpy
drop-in and the device (tests/test_gpu_window.py).  Everything is seeded.
No torch, no GPU: importable anywhere."""
from __future__ import annotations

import functools

import numpy as np

import pose_graph_cases as pc
import window_ref as ref

SPACINGS = pc.SPACINGS


def frame_inputs(p, spacings, n_steps, seed=0):
    """T (n_steps, S, 12), info (n_steps, S, 21), status, inliers (n_steps, S) int32 from a planted graph p over the same spacings:
    the pair (t - s, t) where t >= s; before that the refinement's answer to an absent pair, status 3 with no inliers."""
    rng = np.random.default_rng(500 + seed)
    where = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(p["first"], p["second"]))}
    S = len(spacings)
    T, info = np.tile(ref.IDENTITY, (n_steps, S, 1)), np.zeros((n_steps, S, 21))
    status, inliers = np.full((n_steps, S), 3, np.int32), np.zeros((n_steps, S), np.int32)
    for t in range(n_steps):
        for k, s in enumerate(spacings):
            if t >= s:
                e = where[(t - s, t)]
                T[t, k], info[t, k], status[t, k], inliers[t, k] = p["T"][e], p["info"][e], rng.integers(0, 3), rng.integers(20, 200)
    return T, info, status, inliers


def window_case(name, window, spacings, n_steps, seed, capacity=None, outliers=0.0, start=False, min_inliers=12, chi=4.0, damping=0.0, n_iter=2):
    p = pc.planted(n_steps, spacings, seed, outliers=outliers)
    T, info, status, inliers = frame_inputs(p, spacings, n_steps, seed)
    return dict(name=name, window=window, spacings=np.array(spacings, np.int32), capacity=n_steps if capacity is None else capacity, T=T,
                info=info, status=status, inliers=inliers, C_start=p["truth"][3].copy() if start else None, min_inliers=min_inliers, chi=chi,
                damping=damping, n_iter=n_iter, truth=p["truth"], C_chain=p["C_chain"])


def shape_cases():
    """The shapes at which the ring's indexing can go wrong, each over enough steps to wrap the ring."""
    return [
        window_case("window_2_one_spacing", 2, (1,), 6, 1),
        window_case("window_4_edges_drop", 4, (1, 3), 11, 2),
        window_case("window_4_spacing_past_the_window", 4, (1, 2, 5), 10, 3),        # the spacing-5 pair is never admitted
        window_case("window_21_five_spacings", 21, SPACINGS, 30, 4, outliers=0.03),
        window_case("window_32_eight_spacings", 32, (1, 2, 3, 5, 8, 13, 21, 31), 36, 5),
    ]


def _changed(case, name, **changes):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    out["name"] = name
    for key, (where, value) in changes.items():
        out[key][where] = value
    return out


def contract_cases():
    """The contract's rows: the start pose, each reason an edge is refused, a lost frame, no iterations, a failed pivot, a short
    trajectory."""
    base = window_case("base", 4, (1, 2, 3), 9, 11)
    zero = _changed(base, "zero_info", info=((slice(None),), 0.0))
    return [base,
            window_case("start_given", 4, (1, 2, 3), 9, 11, start=True),
            _changed(base, "status_3", status=((5, 0), 3)),
            _changed(base, "few_inliers", inliers=((6, 1), 11)),
            _changed(base, "nan_in_T", T=((7, 0, 5), np.nan)),
            _changed(base, "inf_in_info", info=((4, 2, 20), np.inf)),
            _changed(base, "lost_frame", status=((5,), 3)),
            dict(base, name="no_iterations", n_iter=0),
            zero,
            dict(base, name="short_trajectory", capacity=5),
            dict(base, name="damped_plain", damping=0.5, chi=1e9, n_iter=3)]


def stacked(cases):
    """Cases of one shape as the operands of one n_windows launch: every per-step array with a window axis behind the step axis."""
    return {k: np.stack([c[k] for c in cases], axis=1) for k in ("T", "info", "status", "inliers")}


@functools.lru_cache(maxsize=None)
def _by_name():
    return {c["name"]: c for c in shape_cases() + contract_cases()}


def case(name):
    return _by_name()[name]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(the steps' outputs, the final state) of the restatement for the named case: computed once, shared, not to be written to."""
    return ref.run(case(name))
