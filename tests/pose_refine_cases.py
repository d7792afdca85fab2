"""Seeded case lists for sslam_pose_refine_pairs (tests/test_pose_refine_cpu.py, tests/test_gpu_pose_refine.py), built on the
planted pairs of tests/pose_ransac_cases.py (its builders and its specs, imported - the same kinds of list: absent pairs, count 0 /
negative / above n1, bad indices, depth holes, 2 and 3 usable rows, coincident points, all outliers, a pure rotation, a pure
translation, the 448-pixel units).  A case here is one of those lists plus a KIND of initial pose, a threshold, a Huber delta and
an iteration count:

  ransac    T_in = the RANSAC restatement's own output for the pair (so the GPU test does not depend on the RANSAC kernel)
  prior     T_in = the planted motion turned by 2 degrees and moved 5 cm - a motion model's prediction; the threshold is wide (60 px)
  identity  T_in = [I | 0] under a wide threshold (40 px): a pose with few inliers; some pairs select under 3 rows (status 3)
  nan       the RANSAC output with one entry replaced by NaN or an infinity in every other pair (status 3 there)

MARGIN.  Every run of every case - the base run and the variations VARIATIONS lists - keeps the restatement MARGIN = 1e-6 (px, or m
for Z') clear of: the distance against the threshold at the selection and at the final rescoring, d against huber in every pass,
Z' against 0, and every pivot against 0.  Two decisions cannot keep an absolute margin everywhere, and where they cannot is fixed
here, before any device ran:
  pivots    a pair flagged `singular` (fewer than three distinct points among its selected rows) has a rank-deficient H whose last
            pivots are rounding noise around 0; the CPU test asserts instead that np.linalg.matrix_rank of the independent H is
            below 6 there.  Every other pivot keeps MARGIN (the smallest in the lists is above 100).
  cost      cost_trial against cost keeps MARGIN RELATIVE to the larger of the two, in the base runs, which stop after n_iter = 1
            (ransac, nan) or 2 (prior, identity) steps, away from convergence.  A cost is a sum of at most 4096 non-negative
            terms 26 additions deep: its rounding error is below 30 * 2^-53 = 3.3e-15 relative, 3e8 times smaller.  The variations
            with n_iter 5 and 16 run until a trial no longer lowers the cost; that last comparison is between two costs equal to
            rounding and can keep no margin by construction.  Both sides take the same correctly rounded operations in the same
            order, so they take the same decision; the bit-for-bit comparison of `iterations` and `status` is what checks it.
A seed whose base run does not hold the margins is replaced by the next one.  Cases are built once per process and never modified.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import pose_ransac_cases as rc
import pose_ransac_ref as rr
import pose_refine_ref as fr

MARGIN = 1e-6
RECOVER_DEG, RECOVER_M = rc.RECOVER_DEG, rc.RECOVER_M
SEED = rc.SEEDS[0]

# name -> (pose_ransac_cases' list, kind, threshold (None: the list's own), huber (None: threshold / 3), n_iter of the base run)
CASES = {
    "k3": ("k3", "ransac", None, None, 1),
    "k5_dup": ("k5_dup", "ransac", None, None, 1),
    "k64_p70": ("k64_p70", "ransac", None, None, 1),
    "k64_p70_prior": ("k64_p70", "prior", 60.0, 20.0, 2),
    "k64_p70_identity": ("k64_p70", "identity", 40.0, 10.0, 2),
    "k64_p70_nan": ("k64_p70", "nan", None, None, 1),
    "k255": ("k255", "ransac", None, None, 1),
    "k256": ("k256", "prior", 60.0, 20.0, 2),
    "k257": ("k257", "ransac", None, None, 1),
    "k300_n257": ("k300_n257", "prior", 60.0, 20.0, 2),
    "k1024": ("k1024", "ransac", None, None, 1),
    "k1025": ("k1025", "prior", 60.0, 20.0, 2),
    "k4096": ("k4096", "ransac", None, None, 1),
    "k64_loose": ("k64_loose", "ransac", None, None, 1),
}
# the lists pose_ransac_cases does not have: exactly 255, 256, 1024 and 4096 usable rows (no holes: every listed row is usable), the
# thread stride, the LDS chunk and the cap; these names take the place of its lists of the same name, which have depth holes
EXTRA_LISTS = {
    "k255": (255, 255, [dict(outliers=0.2), dict(outliers=0.0, kind="rotation")], 64, (1.0, 1.0)),
    "k256": (256, 256, [dict(outliers=0.2), dict(outliers=0.5)], 64, rc.SCALE_448),
    "k1024": (1024, 1024, [dict(outliers=0.5)], 64, rc.SCALE_448),
    "k4096": (4096, 4096, [dict(outliers=0.05)], 64, rc.SCALE_448),
}
NAMES = tuple(CASES)
# (case, overrides) run beside the base runs: the iteration counts, and huber below and above every residual (a huber that small
# makes the cost an L1 fit, which drives some residuals to zero within a few steps: those two runs stop after 2 and 1)
VARIATIONS = (
    ("k64_p70", dict(n_iter=0)), ("k64_p70", dict(n_iter=5)), ("k64_p70", dict(n_iter=16)),
    ("k64_p70_prior", dict(n_iter=16)), ("k64_p70_identity", dict(n_iter=16)), ("k1025", dict(n_iter=16)), ("k300_n257", dict(n_iter=5)),
    ("k64_loose", dict(n_iter=5)), ("k64_loose", dict(huber=1e-3, n_iter=2)), ("k64_p70_identity", dict(huber=1e-3, n_iter=1)), ("k64_loose", dict(huber=1e5, n_iter=5)),
    ("k257", dict(huber=1e3, n_iter=5)),
)


def _turn():
    """The prior's error: 2 degrees about (1, 1, 1) and 5 cm, applied on the left of the planted motion."""
    return rr.rotation([1.0, 1.0, 1.0], np.deg2rad(2.0)), np.array([0.03, -0.02, 0.0346410161513775])


def _initial(kind, c, ransac_T):
    P = len(c["first"])
    if kind == "ransac":
        return ransac_T.copy()
    if kind == "identity":
        return np.tile(rc.IDENT, (P, 1))
    if kind == "prior":
        dR, dt = _turn()
        out = np.empty((P, 12))
        for p in range(P):
            m = c["planted"][p].reshape(3, 4)
            out[p] = np.hstack([dR @ m[:, :3], (dR @ m[:, 3] + dt)[:, None]]).reshape(12)
        return out
    if kind == "nan":
        out = ransac_T.copy()
        for p in range(1, P, 2):
            out[p, (5 * p) % 12] = (np.nan, np.inf, -np.inf)[p % 3]
        return out
    raise ValueError(kind)


def _list(source, rng_seed):
    if source in EXTRA_LISTS:
        k, n1, specs, n_hyp, scale = EXTRA_LISTS[source]
        return rc._case(source, k, n1, specs, n_hyp, scale, rng_seed)
    k, n1, specs, n_hyp, scale = rc.CASES[source][:5]
    return rc._case(source, k, n1, specs, n_hyp, scale, rng_seed, *rc.CASES[source][5:])


def run(c, detail=False, **override):
    """The restatement on a case (huber / n_iter / threshold / T_in overridden if given): the list of refine() dicts."""
    a = dict(threshold=c["threshold"], huber=c["huber"], n_iter=c["n_iter"], T_in=c["T_in"])
    a.update(override)
    return fr.refine_pairs(c["bank"], c["depth_bank"], c["first"], c["second"], c["matches"], c["count"], c["cam"], a["threshold"], a["huber"],
                           a["n_iter"], a["T_in"], c["scale_x"], c["scale_y"], detail)


def singular(c, p) -> bool:
    """Fewer than three distinct points among the usable rows of a present pair: no 6-parameter pose is determined."""
    if not rc.present(c, p):
        return False
    a, b = c["first"][p], c["second"][p]
    rows = rr.usable_rows(c["bank"][a], c["bank"][b], c["depth_bank"][a], c["depth_bank"][b], c["matches"][p], c["count"][p], c["cam"],
                          c["scale_x"], c["scale_y"])
    return 0 < len(rows["slot"]) and len(np.unique(rows["Xa"], axis=0)) < 3


def check_margins(c, with_cost=True, **override) -> dict:
    """The least margins over the pairs of a run (keys of pose_refine_ref.margins; cost relative, see the module's docstring)."""
    a = dict(threshold=c["threshold"], huber=c["huber"])
    a.update({key: v for key, v in override.items() if key in a})
    least = dict(edge=np.inf, huber=np.inf, z=np.inf, cost=np.inf, pivot=np.inf)
    for p, r in enumerate(run(c, detail=True, **override)):
        m = fr.margins(r["log"], a["threshold"], a["huber"])
        if c["singular"][p]:
            m["pivot"] = np.inf
        m["cost"] = np.inf
        if with_cost and r["log"] is not None and r["log"]["cost_gap"]:
            costs = [r["cost_in"]]                        # the cost every trial was compared with
            for gap in r["log"]["cost_gap"]:
                if np.isfinite(gap):
                    m["cost"] = min(m["cost"], abs(gap) / max(costs[-1], costs[-1] + gap))
                if gap < 0:
                    costs.append(costs[-1] + gap)
        least = {key: min(least[key], m[key]) for key in least}
    return least


def margins_ok(m) -> bool:
    return all(v >= MARGIN for v in m.values())


@lru_cache(maxsize=None)
def case(name: str):
    source, kind, threshold, huber, n_iter = CASES[name]
    rng_seed = 7000 + NAMES.index(name)
    while True:
        c = _list(source, rng_seed)
        if rc.margins_ok(rc.check_margins(c, SEED)):
            ransac = rr.stacked(rr.ransac_pairs(c["bank"], c["depth_bank"], c["first"], c["second"], c["matches"], c["count"], c["cam"],
                                                c["threshold"], c["n_hyp"], SEED, c["scale_x"], c["scale_y"]))
            c = dict(c, name=name, kind=kind, ransac=ransac)
            c["threshold"] = c["threshold"] if threshold is None else threshold
            c["huber"] = c["threshold"] / 3 if huber is None else huber
            c["n_iter"] = n_iter
            c["T_in"] = _initial(kind, c, ransac["T"])
            c["singular"] = [singular(c, p) for p in range(len(c["first"]))]
            if margins_ok(check_margins(c)):
                return c
        rng_seed += 100


@lru_cache(maxsize=None)
def expected(name: str, variation: tuple = ()):
    """The restatement's outputs for a case, base run or variation (a tuple of (key, value) overrides), as the device's arrays."""
    return fr.stacked(run(case(name), **dict(variation)))
