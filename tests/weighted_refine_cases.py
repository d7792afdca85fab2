"""Seeded case lists for the two entries of libsslam_weight.so (tests/test_weighted_refine_cpu.py, tests/test_gpu_weighted_refine.py).
The lists, the initial-pose kinds, the thresholds and the iteration counts are tests/pose_refine_cases.py's, imported and not
modified: every one of its cases (the smallest shapes at which the kernel can go wrong: 3 and 5 keypoints, the 70-pair list under
its four kinds, the thread stride 255 / 256 / 257, n1 < K, the LDS chunk edge 1024 / 1025 - where the weight's source changes from
LDS to global memory -, the cap 4096, the loose all-outlier list) crossed with a KIND of weight array (P, n1) fp32:

  ones           every weight 1.0f
  random         fp32 in [2^-10, 1]
  quarter        the same draw x 2^-2
  eight          the same draw x 2^3
  holes          the draw with 30 % of the slots exactly +0.0f; on k3 slot 0 of every pair, and on pair 0 of every k64_p70 case
                 every slot but two, so that fewer than 3 rows are selected there (status 3)
  bad            the draw with NaN, +inf, -inf, -1, -0.0 and a subnormal scattered in (each on about 4 % of the slots)
  conf_product   the match_weights restatement, mode product, on a seeded confidence bank (n_bank, K): fp32 in [0.3, 1] with exact
  conf_expected  0.0, exact 1.0, SSLC_CONF_MIN and its two fp32 neighbours scattered in; mode expected_error at sigma0 = 0.5

MARGIN.  pose_refine_cases' rules carry over to the weighted runs, with its exemptions: every run keeps the restatement
MARGIN = 1e-6 clear of the threshold (selection and rescoring), of huber in every pass, of Z' = 0 and of a zero pivot; the cost gap
RELATIVE, in the base runs only; a pair with fewer than three distinct points among its usable rows of selectable weight is exempt
from the pivot margin.  The weight test g > 0 && g - g == 0 is exact in fp32 and needs no margin.  A weight seed whose base run
does not hold the margins is replaced by the next one (at most MAX_SEEDS times).  Arrays are built once per process and are
read-only."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import pose_ransac_cases as rc
import pose_ransac_ref as rr
import pose_refine_cases as pc
import pose_refine_ref as fr
import weighted_refine_ref as wr

MARGIN = pc.MARGIN
NAMES = pc.NAMES
KINDS = ("ones", "quarter", "eight", "random", "holes", "bad", "conf_product", "conf_expected")
VARIATIONS = pc.VARIATIONS
SIGMA0 = 0.5
CONF_MIN = np.float32(1.17549435e-38)      # SSLC_CONF_MIN
MAX_SEEDS = 50
SUBNORMAL = np.float32(1e-41)
STARVED_PAIR = 0                           # the pair of the k64_p70 cases that `holes` leaves two selectable slots


def _draw(rng, shape):
    return rng.uniform(2.0 ** -10, 1.0, shape).astype(np.float32)


def confidence_bank(c, seed):
    """(n_bank, K) fp32 confidences for a case: [0.3, 1] with the exact and the edge values scattered in."""
    rng = np.random.default_rng(seed)
    shape = c["bank"].shape[:2]
    conf = rng.uniform(0.3, 1.0, shape).astype(np.float32)
    special = np.array([0.0, 1.0, CONF_MIN, np.nextafter(CONF_MIN, np.float32(0)), np.nextafter(CONF_MIN, np.float32(1))], np.float32)
    pick = rng.integers(0, 50, shape)       # 0 .. 4: one of the special values, about 2 % each
    for i, v in enumerate(special):
        conf[pick == i] = v
    return conf


def _weights(c, kind, seed):
    P, n1 = c["matches"].shape[:2]
    rng = np.random.default_rng(seed)
    base = _draw(rng, (P, n1))
    if kind == "ones":
        return np.ones((P, n1), np.float32)
    if kind == "random":
        return base
    if kind == "quarter":
        return base * np.float32(0.25)
    if kind == "eight":
        return base * np.float32(8.0)
    if kind == "holes":
        w = np.where(rng.uniform(size=(P, n1)) < 0.3, np.float32(0.0), base).astype(np.float32)
        if c["name"] == "k3":
            w[:, 0] = 0.0
        if c["name"].startswith("k64_p70"):
            w[STARVED_PAIR, 2:] = 0.0
        return w
    if kind == "bad":
        w = base.copy()
        pick = rng.integers(0, 25, (P, n1))
        for i, v in enumerate((np.nan, np.inf, -np.inf, -1.0, -0.0, SUBNORMAL)):
            w[pick == i] = np.float32(v)
        return w
    mode = {"conf_product": wr.PRODUCT, "conf_expected": wr.EXPECTED_ERROR}[kind]
    return wr.match_weights(confidence_bank(c, seed), c["first"], c["second"], c["matches"], c["count"], mode, SIGMA0)


def run(c, weight, detail=False, **override):
    """The weighted restatement on a case (huber / n_iter / threshold / T_in overridden if given): the list of refine() dicts."""
    a = dict(threshold=c["threshold"], huber=c["huber"], n_iter=c["n_iter"], T_in=c["T_in"])
    a.update(override)
    return wr.refine_pairs(c["bank"], c["depth_bank"], c["first"], c["second"], c["matches"], c["count"], weight, c["cam"], a["threshold"],
                           a["huber"], a["n_iter"], a["T_in"], c["scale_x"], c["scale_y"], detail)


def singular(c, weight, p) -> bool:
    """Fewer than three distinct points among the usable rows of selectable weight of a present pair."""
    if not rc.present(c, p):
        return False
    a, b = c["first"][p], c["second"][p]
    rows = rr.usable_rows(c["bank"][a], c["bank"][b], c["depth_bank"][a], c["depth_bank"][b], c["matches"][p], c["count"][p], c["cam"],
                          c["scale_x"], c["scale_y"])
    if len(rows["slot"]) == 0:
        return False
    keep = wr.weight_ok(weight[p][rows["slot"]])
    return len(np.unique(rows["Xa"][keep], axis=0)) < 3


def margins_of(c, weight, results, with_cost=True, **override) -> dict:
    """pose_refine_cases.check_margins on the results of a weighted run(detail=True)."""
    a = dict(threshold=c["threshold"], huber=c["huber"])
    a.update({key: v for key, v in override.items() if key in a})
    least = dict(edge=np.inf, huber=np.inf, z=np.inf, cost=np.inf, pivot=np.inf)
    for p, r in enumerate(results):
        m = fr.margins(r["log"], a["threshold"], a["huber"])
        if c["singular"][p] or singular(c, weight, p):
            m["pivot"] = np.inf
        m["cost"] = np.inf
        if with_cost and r["log"] is not None and r["log"]["cost_gap"]:
            costs = [r["cost_in"]]
            for gap in r["log"]["cost_gap"]:
                if np.isfinite(gap):
                    m["cost"] = min(m["cost"], abs(gap) / max(costs[-1], costs[-1] + gap))
                if gap < 0:
                    costs.append(costs[-1] + gap)
        least = {key: min(least[key], m[key]) for key in least}
    return least


def check_margins(c, weight, with_cost=True, **override) -> dict:
    return margins_of(c, weight, run(c, weight, detail=True, **override), with_cost, **override)


def margins_ok(m) -> bool:
    return all(v >= MARGIN for v in m.values())


def _base_seed(name, kind):
    # quarter, eight and random share one draw: the scaling tests compare them
    return 9000 + 10 * NAMES.index(name) + (3 if kind in ("quarter", "eight", "random") else KINDS.index(kind))


@lru_cache(maxsize=None)
def _built(name: str, kind: str):
    """(weight, expected base run, margins) of a case under a weight kind: the first seed whose base run keeps the margins.  The
    three kinds that share a draw step their seed together: a seed must hold for all three."""
    c = pc.case(name)
    seed = _base_seed(name, kind)
    group = ("quarter", "eight", "random") if kind in ("quarter", "eight", "random") else (kind,)
    for _ in range(MAX_SEEDS):
        built = {}
        for k in group:
            w = _weights(c, k, seed)
            w.setflags(write=False)
            res = run(c, w, detail=True)
            built[k] = (w, wr.stacked(res), margins_of(c, w, res))
        if all(margins_ok(b[2]) for b in built.values()):
            return built
        seed += 1000
    raise AssertionError(f"no weight seed of {name} / {kind} keeps the margins")


def weights(name: str, kind: str) -> np.ndarray:
    return _built(name, "random" if kind in ("quarter", "eight") else kind)[kind][0]


def margins(name: str, kind: str) -> dict:
    return _built(name, "random" if kind in ("quarter", "eight") else kind)[kind][2]


@lru_cache(maxsize=None)
def expected(name: str, kind: str, variation: tuple = ()):
    """The restatement's outputs for a case under a weight kind, base run or variation, as the device's arrays."""
    if not variation:
        return _built(name, "random" if kind in ("quarter", "eight") else kind)[kind][1]
    return wr.stacked(run(pc.case(name), weights(name, kind), **dict(variation)))


@lru_cache(maxsize=None)
def weight_case(shape_name: str):
    """Operands of sslu_match_weights beyond the refinement's lists: name -> dict(conf, first, second, matches, count)."""
    n_bank, K, n1, P = {"k1": (2, 1, 1, 3), "k300_n257": (5, 300, 257, 9), "k4096": (3, 4096, 4096, 4)}[shape_name]
    rng = np.random.default_rng(9900 + K)
    conf = rng.uniform(0.0, 1.0, (n_bank, K)).astype(np.float32)
    first = rng.integers(0, n_bank, P).astype(np.int32)
    second = rng.integers(0, n_bank, P).astype(np.int32)
    matches = rng.integers(0, K, (P, n1, 2)).astype(np.int64)
    count = rng.integers(1, n1 + 1, P).astype(np.int32)
    if shape_name == "k1":                       # one slot per pair: a match, an absent pair, an index of -1
        conf[:, 0] = (1.0, 0.5)
        first[:], second[:], count[:] = (0, -1, 1), (1, 0, 0), 1
        matches[:, 0] = ((0, 0), (0, 0), (-1, 0))
    else:
        conf[:, :5] = [0.0, 1.0, CONF_MIN, np.nextafter(CONF_MIN, np.float32(0)), np.nextafter(CONF_MIN, np.float32(1))]
        count[:4] = (n1, 0, -5, n1 + 7)          # the whole list, none, a negative count, one above n1
    if shape_name == "k4096":
        first[3] = n_bank                        # an index past the bank: an absent pair
        matches[0, 0] = (0, 0)
    if shape_name == "k300_n257":
        first[4], second[5] = -1, n_bank         # absent pairs
        count[6:] = n1
        matches[6, 0::7, 0] = -1                 # indices -1 and K
        matches[7, 1::5, 1] = K
        matches[8, 2::3] = (K, -1)
    out = dict(conf=conf, first=first, second=second, matches=matches, count=count, n_bank=n_bank, K=K, n1=n1)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
