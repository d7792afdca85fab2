"""What tests/test_select_range_inputs.py (CPU) and tests/test_gpu_select_range.py share: saliency maps and parameters that run
sslam_select_keypoints over the whole range include/sslam_hip.h declares - every nms_radius 0..8, grids from 1 x 1 to 64 x 64 - and
a plain numpy restatement of the selection rule that says which arm of the kernel a case reaches.

The restatement (restate) is the reference's rule written once more with array operations: thresholds, NMS survivors, counts, the
five arms.  It classifies the cases WITHOUT the device and without the oracle; the CPU test then holds it against the oracle, index
for index, so a case list that stopped reaching an arm fails there and not on the GPU.

A case is a dict: tag, sal (frames, G, G) fp32, K, radius, pct.
"""
import numpy as np

GRIDS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 28, 33, 64)
RADII = tuple(range(9))
PCTS = (0.0, 0.1, 0.5, 0.73, 1.0)
K_NAMES = ("one", "seventh", "half", "all_but_one", "all")
KINDS = ("uniform", "quantised", "bumps", "band", "constant", "one_above_floor", "twin_max")
ARMS = ("topk", "pct", "pad", "none")      # nv >= K; 0 < nv < K filled from a lower percentile / from the raw order; nv == 0
LOWER = (0.40, 0.30, 0.20, 0.10)


def _rng(*key):
    return np.random.Generator(np.random.PCG64([9100] + [int(k) for k in key]))


def k_choices(n: int) -> tuple:
    """K for K_NAMES on a grid of n cells: 1, about n / 7, n / 2, n - 1, n - never above n, never below 1."""
    return (1, max(1, n // 7), max(1, n // 2), max(1, n - 1), n)


def make_map(kind: str, g: int, frames: int, rng) -> np.ndarray:
    """(frames, g, g) fp32.  The first four kinds are those of test_fuzz_select_keypoints."""
    sal = rng.random((frames, g, g)).astype(np.float32)
    if kind == "uniform":
        return sal
    if kind == "quantised":                         # plateaus and exact ties everywhere
        return (np.floor(sal * rng.integers(2, 9)) / 8).astype(np.float32)
    if kind == "bumps":                             # few, wide maxima
        yy, xx = np.mgrid[0:g, 0:g].astype(np.float32)
        return np.stack([np.sin(xx * rng.random() + f) * np.cos(yy * rng.random() - f) * 0.5 + 0.5 for f in range(frames)]).astype(np.float32)
    if kind == "band":                              # what an untrained selector emits
        return (0.5 + 0.01 * (sal - 0.5)).astype(np.float32)
    if kind == "constant":                          # every cell survives the NMS and equals every quantile; the second frame lies
        levels = np.array([0.6, 0.03, 0.5], np.float32)      # below both floors
        return np.broadcast_to(levels[np.arange(frames) % 3, None, None], (frames, g, g)).copy()
    if kind == "one_above_floor":                   # one cell above the 0.1 floor, the rest below the 0.05 floor too
        sal = (sal * np.float32(0.045)).astype(np.float32)
        for f in range(frames):
            sal[f].flat[int(rng.integers(0, g * g))] = np.float32(0.7)
        return sal
    assert kind == "twin_max"                       # the global maximum in two neighbouring cells: both survive v == mx
    sal = (sal * np.float32(0.9)).astype(np.float32)
    for f in range(frames):
        y, x = int(rng.integers(0, g)), int(rng.integers(0, max(1, g - 1)))
        sal[f, y, x] = np.float32(0.95)
        sal[f, y, min(x + 1, g - 1)] = np.float32(0.95)
    return sal


def sweep_cases(g: int) -> list:
    """The grid sweep at one G: every radius 0..8 with every map kind; K, percentile and the frame count rotate so that every
    radius meets every K choice, every percentile and both frame counts (asserted by the CPU test).  K <= n throughout."""
    gi, n = GRIDS.index(g), g * g
    out = []
    for r in RADII:
        for ki, kind in enumerate(KINDS):
            kn = (ki + r + gi) % 5
            frames = 1 if (ki + r + gi) % 2 == 0 else 3
            out.append(dict(tag=f"g{g}_r{r}_{kind}_{K_NAMES[kn]}", sal=make_map(kind, g, frames, _rng(1, g, r, ki)), K=k_choices(n)[kn],
                            radius=r, pct=PCTS[(2 * ki + r + 3 * gi) % 5], k_name=K_NAMES[kn], kind=kind))
    if g == 64:                                     # the largest launch the entry takes: K = 4096 under the widest window
        out.append(dict(tag="g64_r8_uniform_4096", sal=make_map("uniform", 64, 3, _rng(2)), K=4096, radius=8, pct=0.5, k_name="all",
                        kind="uniform"))
    return out


def status_cases() -> list:
    """K beyond what the grid holds.  K = 4096 always flags the frame; K = n + 1 flags it only where no cell passes the threshold
    (with nv survivors the pad asks the raw order for n + 1 - nv <= n cells).  Three frames each: uniform, all below both floors, and
    twin maxima - every one of the K slots is compared, the repeat of the best point included."""
    out = []
    for g in (1, 2, 5):
        for r in (0, 8):
            for K in (g * g + 1, 4096):
                sal = np.concatenate([make_map("uniform", g, 1, _rng(3, g, r)), make_map("uniform", g, 1, _rng(4, g, r)) * np.float32(0.04),
                                      make_map("twin_max", g, 1, _rng(5, g, r))]).astype(np.float32)
                out.append(dict(tag=f"status_g{g}_r{r}_K{K}", sal=sal, K=K, radius=r, pct=0.5))
    return out


def _planted(g: int, r: int, q: float, seed: int) -> np.ndarray:
    """A uniform(0.2, 1) map whose corner block [0, r]^2 is lowered below every lower threshold, except the corner cell itself: it
    gets a value between two order statistics around the quantile q, so it survives the NMS (nothing in its window is larger) below
    the 0.5 threshold.  The block holds under a tenth of the cells at every size used here, so the 0.10 quantile stays above it."""
    rng = _rng(6, g, r, seed)
    m = (0.2 + 0.8 * rng.random((g, g))).astype(np.float32)
    m[: r + 1, : r + 1] = (0.06 + 0.04 * rng.random((r + 1, r + 1))).astype(np.float32)
    s = np.sort(m.ravel())
    k = int(q * (g * g - 1))
    m[0, 0] = np.float32((np.float64(s[k]) + np.float64(s[k + 1])) / 2)
    return m


def arm_cases() -> list:
    """For each radius 5..8: one hand-made case per arm of select_keypoints_kernel (the percentile arm twice, at the 0.40 and at the
    0.10 set), and the status flag.  Which arm each reaches is asserted by the CPU test from restate(), never from the device."""
    out = []
    for r in (5, 6, 7, 8):
        u17 = make_map("uniform", 17, 1, _rng(7, r))
        out.append(dict(tag=f"arm_topk_r{r}", sal=u17, K=1, radius=r, pct=0.5, arm="topk"))
        out.append(dict(tag=f"arm_pad_r{r}", sal=u17, K=17 * 17 // 2, radius=r, pct=0.5, arm="pad"))
        out.append(dict(tag=f"arm_none_r{r}", sal=u17 * np.float32(0.0999), K=40, radius=r, pct=0.5, arm="none"))
        out.append(dict(tag=f"arm_status_r{r}", sal=u17[:, :5, :5].copy(), K=4096, radius=r, pct=0.5, arm="pad", status=1))
        for q, tsel in ((0.45, 1), (0.15, 4)):
            m = _planted(33, r, q, tsel)
            nv = restate(m, 1, r, 0.5)["nv"]
            out.append(dict(tag=f"arm_pct{tsel}_r{r}", sal=m[None], K=nv + 1, radius=r, pct=0.5, arm="pct", tsel=tsel))
    return out


# ------------------------------------------------------------------------------------------------ the rule, restated
def quantile32(asc: np.ndarray, q: float) -> np.float32:
    """torch.quantile(linear) of an ascending fp32 array in fp32: rank = fp32(q) * (n - 1), the fused lerp of either side (the
    product is exact in float64, so one rounding to fp32 - the double rounding of the sum aside - is the fused result)."""
    n = asc.size
    rank = np.float32(np.float32(q) * np.float32(n - 1))
    lo, hi = np.floor(rank), np.ceil(rank)
    w = np.float32(rank - lo)
    a, b = asc[int(lo)], asc[int(hi)]
    diff = np.float32(b - a)
    if w < np.float32(0.5):
        return np.float32(np.float64(w) * np.float64(diff) + np.float64(a))
    return np.float32(np.float64(b) - np.float64(diff) * np.float64(np.float32(1) - w))


def nms(m: np.ndarray, radius: int) -> np.ndarray:
    """Keep the cells that equal the maximum of their (2 r + 1)^2 window clipped to the grid, zero the others."""
    if radius == 0:
        return m.copy()
    g = m.shape[0]
    pad = np.full((g + 2 * radius, g + 2 * radius), -np.inf, np.float32)
    pad[radius:radius + g, radius:radius + g] = m
    mx = np.full_like(m, -np.inf)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            np.maximum(mx, pad[dy:dy + g, dx:dx + g], out=mx)
    return m * (m == mx).astype(np.float32)


def _top(values: np.ndarray, cells: np.ndarray, k: int) -> np.ndarray:
    """The first k of `cells` by value descending, then cell index ascending."""
    return cells[np.lexsort((cells, -values))][:k]


def restate(m: np.ndarray, K: int, radius: int, pct: float) -> dict:
    """One frame: arm, tsel (1..4 = the 0.40 .. 0.10 set that filled the remainder, else 0), nv, status, idx (K,), scores (K,)."""
    m = np.ascontiguousarray(m, np.float32)
    n = m.size
    raw, asc = m.ravel(), np.sort(m.ravel())
    cells = np.arange(n)
    thr = max(quantile32(asc, pct), np.float32(0.1))
    sv = nms(m, radius).ravel()
    valid = sv > thr
    nv, tsel, status = int(valid.sum()), 0, 0
    if nv >= K:
        arm, idx = "topk", _top(sv[valid], cells[valid], K)
        sc = sv[idx]
    elif nv > 0:
        idx, sc = cells[valid], sv[valid]
        remaining = K - nv
        for t, p in enumerate(LOWER):
            extra = (sv > max(quantile32(asc, p), np.float32(0.05))) & ~valid
            if int(extra.sum()) >= remaining:
                e = _top(sv[extra], cells[extra], remaining)
                arm, tsel, idx, sc = "pct", t + 1, np.concatenate([idx, e]), np.concatenate([sc, sv[e]])
                break
        else:
            e = _top(raw, cells, min(remaining, n))
            arm, status, idx, sc = "pad", int(remaining > n), np.concatenate([idx, e]), np.concatenate([sc, raw[e]])
    else:
        arm, status, idx = "none", int(K > n), _top(raw, cells, min(K, n))
        sc = raw[idx]
    if len(idx) < K:                                # only under status 1: the first slot of the best score, repeated
        b = int(np.argmax(sc))
        idx = np.concatenate([idx, np.full(K - len(idx), idx[b])])
        sc = np.concatenate([sc, np.full(K - len(sc), sc[b], np.float32)])
    return dict(arm=arm, tsel=tsel, nv=nv, status=status, idx=idx.astype(np.int32), scores=sc.astype(np.float32))


# ------------------------------------------------------------------------------------------------ the reference fixture
GOLDEN_GRIDS = (1, 2, 3, 5, 9, 17, 28)
GOLDEN_RADII = (4, 5, 6, 7, 8)
GOLDEN_COUNT = 70


def golden_case(s: int):
    """Case s of tests/golden/select_range.npz (make_golden_select_range.py runs the reference's selector on it): a tie-free map -
    uniform / a band around 0.5 / everything below 0.3 - with G, radius, K <= n and the percentile walking through their sets."""
    g = GOLDEN_GRIDS[s % 7]
    radius = GOLDEN_RADII[(s // 7 + s) % 5]
    n = g * g
    rng = _rng(8, s)
    while True:
        u = rng.random((g, g))
        m = (u if s % 3 == 0 else 0.5 + 0.02 * (u - 0.5) if s % 3 == 1 else 0.3 * u).astype(np.float32)
        if np.unique(m).size == m.size:
            break
    K = (1, max(1, n // 7), max(1, n // 2), n)[(s // 3) % 4]
    return m, K, radius, (0.0, 0.5, 1.0, 0.1, 0.73)[(s // 2) % 5]
