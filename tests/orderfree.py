"""Order-free inputs: operands on which a bf16 kernel has to equal the exact fp32 oracle BIT FOR BIT.

bf16 operands make a kernel incomparable to the oracle only because fp32 partial sums round differently in a different order.
Here every operand is a small dyadic number that survives the rounding to bf16, and every product and every partial sum of
every output - in ANY order of accumulation - is an integer multiple of one granularity below 2^24 of them: exactly
representable in fp32.  The accumulation order then stops mattering, the fp32 epilogues (canonical sigmoid; v / max(sqrtf(ss),
1e-12)) are the oracle's own, and the result has no tolerance.

Each builder proves its own claim in integer arithmetic on the reference side alone (numpy; no kernel, no oracle): it computes
the largest sum of |terms| / granularity over all outputs of every layer, asserts it is below 2^24, asserts that every operand
equals its own bf16 rounding, and returns the exact result that any correct implementation must produce.

numpy only, like synth.py: the same bytes are regenerated wherever the tests run.
"""
from __future__ import annotations

import numpy as np

from oracle.ora_bf16 import bf16_round

LIMIT = 1 << 24          # integers of magnitude < 2^24 are exact in fp32, and so is every partial sum bounded by that


def _rng(seed: int) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(seed))


def _is_bf16(a) -> bool:
    a = np.ascontiguousarray(a, np.float32)
    return np.array_equal(bf16_round(a).view(np.uint32), a.view(np.uint32))


def _imatmul(a, b):
    """Integer-valued matrices, product in float64 (exact: every sum asserted below 2^24 is far below 2^53)."""
    return a.astype(np.float64) @ b.astype(np.float64)


# ------------------------------------------------------------------------------------------------------ saliency CNN
F_SEL = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], np.float32)      # features: units of 2^-1


def selector_state(seed: int, hidden: int = 256) -> dict:
    """conv.0.weight = k/64, k in -4..4 at 25 % density; conv.0.bias = j/64; conv.2.weight = k/32; conv.2.bias = 0.25."""
    rng = _rng(91_000 + seed)
    k1 = rng.integers(-4, 5, size=(hidden, 384, 3, 3)) * (rng.random((hidden, 384, 3, 3)) < 0.25)
    return {"conv.0.weight": (k1 / 64.0).astype(np.float32),
            "conv.0.bias": (rng.integers(-8, 9, size=hidden) / 64.0).astype(np.float32),
            "conv.2.weight": (rng.integers(-4, 5, size=(1, hidden, 1, 1)) / 32.0).astype(np.float32),
            "conv.2.bias": np.array([0.25], np.float32)}


def selector_features(seed: int, grid: int, frames: int) -> np.ndarray:
    return _rng(92_000 + seed).choice(F_SEL, size=(frames, grid, grid, 384)).astype(np.float32)


def selector_exact(feat: np.ndarray, sd: dict):
    """-> (logits float32, exact by construction; dict of the two bounds in units of the layer's granularity).

    conv3x3: features in units of 2^-1, weights 2^-6, bias 2^-6 -> terms in units of 2^-7;
    conv1x1: hidden (ReLU) in units of 2^-7, weights 2^-5, bias 2^-2 -> terms in units of 2^-12."""
    assert _is_bf16(feat) and _is_bf16(sd["conv.0.weight"]), "operands must survive bf16 rounding"
    n, g, _, c = feat.shape
    fi = np.zeros((n, g + 2, g + 2, c), np.float32)
    fi[:, 1:-1, 1:-1] = feat * 2.0
    wi = np.rint(sd["conv.0.weight"] * 64.0).astype(np.float32)           # (hs, c, 3, 3) integers
    bi = np.rint(sd["conv.0.bias"] * 64.0) * 2.0                         # units of 2^-7
    assert np.array_equal(wi / 64.0, sd["conv.0.weight"]) and np.array_equal(bi / 128.0, sd["conv.0.bias"])
    hs = wi.shape[0]
    hid = np.zeros((n, g, g, hs), np.float64) + bi
    mag = np.zeros((n, g, g, hs), np.float64) + np.abs(bi)
    for ky in range(3):
        for kx in range(3):
            win = fi[:, ky:ky + g, kx:kx + g]
            hid += _imatmul(win, wi[:, :, ky, kx].T)
            mag += _imatmul(np.abs(win), np.abs(wi[:, :, ky, kx]).T)
    conv_bound = int(mag.max())
    assert conv_bound < LIMIT, conv_bound
    hid = np.maximum(hid, 0.0)                                           # integers, units of 2^-7
    w2 = np.rint(sd["conv.2.weight"].reshape(-1) * 32.0)
    assert np.array_equal(w2 / 32.0, sd["conv.2.weight"].reshape(-1)) and float(sd["conv.2.bias"][0]) == 0.25
    logit = hid @ w2 + 1024.0                                            # units of 2^-12
    pw_bound = int((hid @ np.abs(w2)).max() + 1024)
    assert pw_bound < LIMIT, pw_bound
    assert hid.max() < LIMIT
    return (logit / 4096.0).astype(np.float32).reshape(n, g, g), {"conv3x3": conv_bound, "conv1x1": pw_bound}


def selector_case(seed: int, grid: int, frames: int, hidden: int = 256):
    """-> (feat (frames, G, G, 384), state dict, exact logits (frames, G, G), bounds)."""
    sd, feat = selector_state(seed, hidden), selector_features(seed, grid, frames)
    logits, bounds = selector_exact(feat, sd)
    return feat, sd, logits, bounds


# ---------------------------------------------------------------------------------------------------- descriptor MLP
def refiner_state(seed: int) -> dict:
    """Depth-0 DescriptorRefiner: integer weights in {-1, 0, 1} (4 % / 3 % dense) and integer biases.  With the integer inputs
    below every activation is an integer: hidden <= 256 after ReLU (its bf16 tile copy is exact), outputs and their squares
    integers (the normalisation's sum of 128 squares is exact)."""
    rng = _rng(93_000 + seed)

    def sparse(shape, density):
        return (rng.integers(0, 2, size=shape) * 2 - 1) * (rng.random(shape) < density)

    return {"input_proj.weight": sparse((384, 384), 0.04).astype(np.float32),
            "input_proj.bias": rng.integers(-8, 9, size=384).astype(np.float32),
            "output_proj.weight": sparse((128, 384), 0.03).astype(np.float32),
            "output_proj.bias": rng.integers(-8, 9, size=128).astype(np.float32)}


def refiner_features(seed: int, grid: int, frames: int) -> np.ndarray:
    """Multiples of 4 in -8..8: any bilinear blend with weights from {1, 1/2, 1/4} is an integer in -8..8."""
    return (_rng(94_000 + seed).integers(-2, 3, size=(frames, grid, grid, 384)) * 4).astype(np.float32)


def _unnormalised(v, grid):
    """grid_sample's coordinate round trip in fp32, as the oracle and the kernels evaluate it."""
    gm1 = np.float32(grid - 1)
    half = gm1 / np.float32(2.0)
    vn = np.float32(2.0) * v.astype(np.float32) / gm1 - np.float32(1.0)
    return (vn + np.float32(1.0)) * half


def refiner_keypoints(seed: int, grid: int, frames: int, K: int) -> np.ndarray:
    """(frames, K, 2) keypoints at integer and half-integer patch coordinates from -0.5 to G - 0.5 (the outermost read the zero
    padding), kept only where the normalise / un-normalise round trip returns the coordinate exactly: the bilinear weights
    are then exactly 0, 1/4, 1/2 or 1."""
    cand = np.arange(-1, 2 * grid, dtype=np.float32) * np.float32(0.5)
    cand = cand[_unnormalised(cand, grid) == cand]
    assert cand.size >= grid, (grid, cand.size)
    assert np.any(cand != np.floor(cand)), "no half-integer coordinate survives at this grid"
    rng = _rng(95_000 + seed)
    return cand[rng.integers(0, cand.size, size=(frames, K, 2))].astype(np.float32)


def gather_exact(feat: np.ndarray, kp: np.ndarray) -> np.ndarray:
    """Bilinear gather (zero padding) of order-free features at order-free keypoints, in float64: integers in -8..8."""
    n, g = feat.shape[0], feat.shape[1]
    pad = np.zeros((n, g + 3, g + 3, feat.shape[-1]), np.float64)       # index i + 1; coordinates reach -1 .. G
    pad[:, 1:g + 1, 1:g + 1] = feat
    x, y = kp[..., 0].astype(np.float64), kp[..., 1].astype(np.float64)
    x0, y0 = np.floor(x), np.floor(y)
    w, nn = x - x0, y - y0
    assert set(np.unique(np.concatenate([w.ravel(), nn.ravel()]))) <= {0.0, 0.5}
    xi, yi = x0.astype(int) + 1, y0.astype(int) + 1
    f = np.arange(n)[:, None]
    out = (pad[f, yi, xi] * ((1 - nn) * (1 - w))[..., None] + pad[f, yi, xi + 1] * ((1 - nn) * w)[..., None]
           + pad[f, yi + 1, xi] * (nn * (1 - w))[..., None] + pad[f, yi + 1, xi + 1] * (nn * w)[..., None])
    assert np.array_equal(out, np.rint(out)) and np.abs(out).max() <= 8
    return out.astype(np.float32)


def refiner_exact(x: np.ndarray, sd: dict):
    """x (rows, 384) integer-valued -> (pre-normalisation outputs (rows, 128) float32, unit descriptors float32, bounds).
    All granularities are 1."""
    for k in ("input_proj.weight", "output_proj.weight"):
        assert _is_bf16(sd[k]) and np.array_equal(sd[k], np.rint(sd[k]))
    assert _is_bf16(x) and np.array_equal(x, np.rint(x))
    w1, b1 = sd["input_proj.weight"], sd["input_proj.bias"]
    w2, b2 = sd["output_proj.weight"], sd["output_proj.bias"]
    in_bound = int((_imatmul(np.abs(x), np.abs(w1).T) + np.abs(b1)).max())
    assert in_bound < LIMIT, in_bound
    hid = np.maximum(_imatmul(x, w1.T) + b1, 0.0)
    assert hid.max() <= 256 and _is_bf16(hid), hid.max()                # the bf16 activation tile holds it exactly
    out_bound = int((_imatmul(hid, np.abs(w2).T) + np.abs(b2)).max())
    assert out_bound < LIMIT, out_bound
    o = _imatmul(hid, w2.T) + b2
    ss = (o * o).sum(-1, keepdims=True)
    norm_bound = int(ss.max())
    assert norm_bound < LIMIT, norm_bound
    o32, ss32 = o.astype(np.float32), ss.astype(np.float32)
    desc = o32 / np.maximum(np.sqrt(ss32), np.float32(1e-12))           # fp32 sqrt and division: correctly rounded, as the kernels'
    return o32, desc, {"input_proj": in_bound, "output_proj": out_bound, "norm_squares": norm_bound, "hidden_max": int(hid.max())}


def refiner_case(seed: int, grid: int, frames: int, K: int):
    """-> (feat, keypoints (frames, K, 2), state dict, gathered x (frames*K, 384), pre-normalisation outputs, descriptors, bounds)."""
    sd, feat = refiner_state(seed), refiner_features(seed, grid, frames)
    kp = refiner_keypoints(seed, grid, frames, K)
    x = gather_exact(feat, kp).reshape(frames * K, 384)
    o, desc, bounds = refiner_exact(x, sd)
    return feat, kp, sd, x, o, desc, bounds
