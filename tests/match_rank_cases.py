"""What tests/test_match_rank_api.py (CPU) and tests/test_gpu_match_rank.py share: the ranking stage's reference in numpy, the
reference-held match lists of tests/golden/, and the value patterns of the raw-entry tests.  Helpers only.

The order (include/sslam_hip.h, sslam_match_rank): better value first, equal values in ascending input slot; better is larger, or
smaller with `ascending`; -0.0 == +0.0; NaN rows last in either direction, in slot order.  numpy's stable argsort of -v (of v when
ascending) is that order: it compares floats, so the zeros tie, and it sorts NaNs to the end whatever the sign of the key."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M1_FILES = ("e2e", "match_wide", "e2e_g40", "e2e_g60")      # (matches, quality) of the reference's own match_with_quality
RULE_FILES = ("matchers", "d256")                            # the reference's M2 lists (ij, sim) and M4 lists (matches, dist)
N_SWEEP = (1, 2, 63, 64, 65, 255, 256, 257, 500, 1000, 2048, 4096)
MAX_N1 = 4096


def rank_order(v: np.ndarray, ascending: bool) -> np.ndarray:
    v = np.asarray(v, np.float32)
    return np.argsort(v if ascending else -v, kind="stable")


def rank_ref(matches, value, count, best, ascending=False):
    """matches (P, n1, 2) int64, value (P, n1) fp32, count (P,) -> (matches (P, best, 2), value (P, best), count (P,) int32,
    slot (P, best) int32): per pair the first min(count, best) rows of the stable order of its first count rows (count clamped to
    [0, n1]), the rest zero."""
    matches, value = np.asarray(matches), np.asarray(value, np.float32)
    n_pairs, n1 = value.shape
    om = np.zeros((n_pairs, best, 2), np.int64)
    ov = np.zeros((n_pairs, best), np.float32)
    oc = np.zeros((n_pairs,), np.int32)
    os_ = np.zeros((n_pairs, best), np.int32)
    for p in range(n_pairs):
        c = min(max(int(count[p]), 0), n1)
        order = rank_order(value[p, :c], ascending)[:best]
        kept = len(order)
        om[p, :kept], ov[p, :kept], os_[p, :kept], oc[p] = matches[p, order], value[p, order], order, kept
    return om, ov, oc, os_


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def m1_pairs() -> list:
    """[(tag, matches (c, 2) int64, quality (c,) fp32)]: every M1 list the four files hold (60 of them)."""
    out = []
    for f in M1_FILES:
        g = _gold(f)
        for key in sorted(g.files):
            if key.endswith("_matches") and key[:-len("matches")] + "quality" in g.files:
                out.append((f"{f}:{key[:-len('_matches')]}", g[key].astype(np.int64), g[key[:-len("matches")] + "quality"]))
    return out


def rule_lists(kind: str) -> list:
    """kind "m2": [(tag, ij (c, 2) int64, sim (c,))]; kind "m4": [(tag, matches, dist)] - the reference's lists in both files."""
    a, b = ("_m2_ij", "_m2_sim") if kind == "m2" else ("_m4_matches", "_m4_dist")
    out = []
    for f in RULE_FILES:
        g = _gold(f)
        for key in sorted(g.files):
            if key.endswith(a):
                out.append((f"{f}:{key[:-len(a)]}", g[key].astype(np.int64), np.ascontiguousarray(g[key[:-len(a)] + b], np.float32)))
    return out


def padded(matches, value, n1=None):
    """One list as the fixed-capacity arrays of one pair: (1, n1, 2), (1, n1), (1,) with a zeroed tail."""
    c = len(value)
    n1 = c if n1 is None else n1
    m = np.zeros((1, n1, 2), np.int64)
    v = np.zeros((1, n1), np.float32)
    m[0, :c], v[0, :c] = matches, value
    return m, v, np.array([c], np.int32)


def slot_matches(n_pairs: int, n1: int) -> np.ndarray:
    """matches whose rows name their own (pair, slot): a gathered row shows where it came from."""
    m = np.empty((n_pairs, n1, 2), np.int64)
    m[..., 0] = np.arange(n1)[None, :]
    m[..., 1] = np.arange(n_pairs)[:, None] * 10007 + 3 * np.arange(n1)[None, :] + 1
    return m


def random_values(seed: int, n_pairs: int, n1: int) -> np.ndarray:
    """Qualities drawn from few enough levels that ties are common: the slot order is exercised at every size."""
    r = np.random.default_rng(seed)
    return (r.integers(0, max(2, n1 // 3), (n_pairs, n1)).astype(np.float32) / np.float32(7.0)).astype(np.float32)


def value_patterns(n1: int) -> dict:
    """name -> (n1,) fp32.  n1 >= 300 puts ties across lane 63 | 64 and slot 255 | 256."""
    r = np.random.default_rng(n1)
    i = np.arange(n1)
    sub = np.float32(1e-45)
    pats = {
        "all_equal": np.full(n1, 0.75, np.float32),
        "descending": (n1 - i).astype(np.float32),
        "ascending": i.astype(np.float32),
        "two_values": np.where((i // 3) % 2 == 0, np.float32(0.25), np.float32(0.5)).astype(np.float32),
        "blocks": np.where((i // 64) % 2 == 0, np.float32(-1.5), np.float32(2.5)).astype(np.float32),
        "zeros": np.where(i % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32),
        "zeros_between": r.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), n1),
        "infs": r.choice(np.array([-np.inf, np.inf, 0.5, -0.5, 3e38, -3e38], np.float32), n1),
        "subnormals": r.choice(np.array([sub, -sub, 3 * sub, 0.0, -0.0, 1.1754944e-38, -1.1754942e-38], np.float32), n1),
    }
    nan = r.standard_normal(n1).astype(np.float32)
    bits = nan.view(np.uint32).copy()
    where = r.random(n1) < 0.3
    bits[where] = np.where(r.random(where.sum()) < 0.5, np.uint32(0x7fc00001), np.uint32(0xffc00000)) + r.integers(0, 5, where.sum()).astype(np.uint32)
    if n1 >= 2:
        bits[0], bits[n1 - 1] = 0xffffffff, 0x7fffffff          # the two NaNs whose plain monotone image would be 0 / all ones
    pats["nans"] = bits.view(np.float32)
    pats["all_nan"] = np.full(n1, np.nan, np.float32)
    return pats
