"""A float64 numpy restatement of libsslam_window.so (csrc_window/window.hip), written from the contract in include/sslam_window.h:
the counter's range, the window, the admission of the frame's S pairs into the ring, the prediction, the slots' local nodes, the
write-back.  The solve is tests/pose_graph_ref.optimize - sslg_pose_graph's restatement - called on the window-local operands at
band = window - 1; only the bookkeeping is restated here.

Tolerance: NONE - both sides take the same correctly rounded + - * / sqrt in one order.
No torch, no GPU: importable anywhere."""
from __future__ import annotations

import numpy as np

import pose_graph_ref as pg

MAX_WINDOW, MAX_SPACINGS, MAX_WINDOWS, MAX_FRAME = 32, 8, 65535, 2 ** 31 - 2
STATE_KEYS = ("t", "ring_first", "ring_second", "ring_T", "ring_info", "ring_C", "trajectory")
OUT_KEYS = ("C_window", "base", "n_nodes", "admitted", "predicted_from", "lost", "status", "iterations", "used_edges", "dropped_edges",
            "failed_row", "cost_in", "cost", "edge_chi2")
IDENTITY = np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
_DTYPE = dict(C_window=np.float64, cost_in=np.float64, cost=np.float64, edge_chi2=np.float64)


def fresh_state(window, n_spacings, capacity):
    """One window's state: t = 0, ring_first = -1, everything else zero."""
    ws = window * n_spacings
    return dict(t=np.zeros((), np.int32), ring_first=np.full(ws, -1, np.int32), ring_second=np.zeros(ws, np.int32), ring_T=np.zeros((ws, 12)),
                ring_info=np.zeros((ws, 21)), ring_C=np.zeros((window, 12)), trajectory=np.zeros((capacity, 12)))


def local_graph(state, base):
    """The window-local operands of the solve: (first, second int32 (W S,), T, info) - step 4 of the header."""
    rf, rs = state["ring_first"].astype(np.int64), state["ring_second"].astype(np.int64)
    first = np.where(rf == -1, -1, np.where(rf < base, -2, rf - base)).astype(np.int32)
    return first, (rs - base).astype(np.int32), state["ring_T"], state["ring_info"]


def step(state, spacings, T, info, status, inliers, C_start=None, min_inliers=12, chi=4.0, damping=0.0, n_iter=2, detail=False):
    """One frame of one window: `state` is updated in place; -> dict of OUT_KEYS (status 4: of `status` alone, nothing touched).
    detail: also `local`, the operands of the solve - first, second, T, info, C_in - as sslg_pose_graph would take them."""
    t = int(state["t"])
    if not 0 <= t <= MAX_FRAME:
        return dict(status=np.int32(4))
    W, S = len(state["ring_C"]), len(spacings)
    T, info = np.asarray(T, np.float64).reshape(S, 12), np.asarray(info, np.float64).reshape(S, 21)
    base = max(0, t - W + 1)
    nn, row = t - base + 1, t % W
    admitted = np.zeros(S, np.int32)
    for k in range(S):
        a = t - int(spacings[k])
        ok = base <= a < t and int(status[k]) != 3 and int(inliers[k]) >= min_inliers and bool(np.isfinite(T[k]).all() and np.isfinite(info[k]).all())
        slot = row * S + k
        admitted[k] = ok
        state["ring_first"][slot], state["ring_second"][slot] = (a if ok else -1), t
        state["ring_T"][slot], state["ring_info"][slot] = (T[k], info[k]) if ok else (0.0, 0.0)
    ring_C = state["ring_C"]
    ks = -1
    if t == 0:
        cur = IDENTITY.copy() if C_start is None else np.asarray(C_start, np.float64).reshape(12).copy()
    else:
        for k in range(S):
            if admitted[k] and (ks < 0 or int(spacings[k]) < int(spacings[ks])):
                ks = k
        cur = pg.compose(T[ks], ring_C[(t - int(spacings[ks])) % W]) if ks >= 0 else ring_C[(t - 1) % W].copy()
    ring_C[row] = cur
    first, second, rT, rI = local_graph(state, base)
    rows = [(base + i) % W for i in range(nn)]
    local = dict(first=first, second=second, T=rT.copy(), info=rI.copy(), C_in=ring_C[rows].copy())
    r = pg.optimize(first, second, rT, rI, local["C_in"], W - 1, chi, damping, n_iter)
    C_window = np.zeros((W, 12))
    C_window[:nn] = r["C"]
    ring_C[rows] = r["C"]
    keep = [i for i in range(nn) if base + i < len(state["trajectory"])]
    state["trajectory"][[base + i for i in keep]] = r["C"][keep]
    state["t"][...] = t + 1
    out = dict(C_window=C_window, base=base, n_nodes=nn, admitted=admitted, predicted_from=ks, lost=int(t > 0 and ks < 0), status=r["status"],
               iterations=r["iterations"], used_edges=r["used_edges"], dropped_edges=r["skipped_edges"], failed_row=r["failed_row"],
               cost_in=r["cost_in"], cost=r["cost"], edge_chi2=r["edge_chi2"])
    out = {k: np.asarray(out[k], dtype=_DTYPE.get(k, np.int32)) for k in OUT_KEYS}
    if detail:
        out["local"] = local
    return out


def run(case, state=None):
    """Every step of a case of tests/window_cases.py on a fresh state (or `state`): (list of the steps' outputs, the final state)."""
    state = fresh_state(case["window"], len(case["spacings"]), case["capacity"]) if state is None else state
    outs = [step(state, case["spacings"], case["T"][i], case["info"][i], case["status"][i], case["inliers"][i], case["C_start"],
                 case["min_inliers"], case["chi"], case["damping"], case["n_iter"]) for i in range(len(case["T"]))]
    return outs, state
