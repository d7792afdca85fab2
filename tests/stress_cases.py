"""Inputs that leave the band the default synthetic weights keep the fp32 kernels in (numpy only, shared by
tests/test_stress_inputs.py on the CPU and tests/test_gpu_trained_ranges.py on the device):

* a pass-through selector whose logit IS a number the test chose, and a list of logits that walks the whole range of the
  canonical exp (the clamp at -87 / 88, the scale factor 2^n at both ends, the subnormal saliency floor, rintf ties);
* steep selectors (conv.2.weight x 60 / x 200): saturated maps with plateaus of exactly 1.0f, as a trained selector emits;
* refiner rows and weights for the arms of 1/sqrtf(var + 1e-5f), fmaxf(sqrtf(ss), 1e-12f) and the divide: zero, subnormal and
  huge rows, dead hidden rows, zero / tiny / overflowing outputs;
* tokens whose channels are constant, ill-conditioned or tiny, for BatchNorm.
"""
from __future__ import annotations

import numpy as np

import synth

LN2 = float(np.log(2.0))
TIE_N = (-126, -125, -100, -64, -24, -1, 0, 1, 24, 64, 100, 126, 127)     # rintf((n + 1/2) ln2 * log2e) sits on a tie


def passthrough_selector(hidden: int = 256) -> dict:
    """Selector weights under which the logit of a cell is feat[cell, 0] - feat[cell, 1], exactly: hidden unit 0 copies
    channel 0 of the centre tap, unit 1 copies channel 1, conv.2 takes their difference; everything else is zero."""
    w1 = np.zeros((hidden, synth.C_FEAT, 3, 3), np.float32)
    w1[0, 0, 1, 1] = w1[1, 1, 1, 1] = 1.0
    w2 = np.zeros((1, hidden, 1, 1), np.float32)
    w2[0, 0], w2[0, 1] = 1.0, -1.0
    return {"conv.0.weight": w1, "conv.0.bias": np.zeros(hidden, np.float32),
            "conv.2.weight": w2, "conv.2.bias": np.zeros(1, np.float32)}


def passthrough_feat(logits: np.ndarray, grid: int, frames: int) -> np.ndarray:
    """(frames, grid, grid, 384) features that passthrough_selector turns into `logits` (frames * grid * grid of them)."""
    l = np.asarray(logits, np.float32).reshape(frames, grid, grid)
    feat = np.zeros((frames, grid, grid, synth.C_FEAT), np.float32)
    feat[..., 0] = np.where(l > 0, l, np.float32(0))
    feat[..., 1] = np.where(l < 0, -l, np.float32(0))
    return feat


def _neighbours(v: float) -> list:
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]


def logit_fixed_points() -> np.ndarray:
    pts = [0.0, -0.0, 1e-30, -1e-30, 103.97, -103.97]
    for v in (87.0, -87.0, 88.0, -88.0):
        pts += [v] + _neighbours(v)
    for n in TIE_N:                               # the two floats nearest to (n + 1/2) ln 2, one on each side of it
        t = (n + 0.5) * LN2
        a = np.float32(t)
        b = np.nextafter(a, np.float32(np.inf) if float(a) < t else np.float32(-np.inf))
        pts += [a, b]
    return np.array(pts, np.float32)


def logit_list(n: int, seed: int = 0) -> np.ndarray:
    """n finite fp32 logits: the fixed points above, the rest uniform in [-110, 110], in a seeded random order (so that the
    fixed points land anywhere in a tile)."""
    fixed = logit_fixed_points()
    assert n >= fixed.size
    rng = synth._rng(90_000 + seed)
    out = np.concatenate([fixed, synth._uniform(rng, (n - fixed.size,), 110.0)])
    out = out[rng.permutation(n)]
    assert np.isfinite(out).all()
    return out


def steep_selector(seed: int, hidden: int, scale: float) -> dict:
    return synth.selector_state(seed, hidden=hidden, w2_scale=scale)


REFINER_BASE_ROWS = 70


def refiner_rows(n: int, seed: int = 0) -> np.ndarray:
    """(n, 384) fp32 N(0, 1) rows with the stress rows below; rows beyond the first 70 repeat them with the sign flipped on
    every odd repeat.  The first k rows are the same for every n >= k."""
    rng = synth._rng(91_000 + seed)
    x = synth._normal(rng, (REFINER_BASE_ROWS, synth.C_FEAT))
    x[1] = np.float32(0.0)
    x[7] = np.float32(-0.0)
    x[2] *= np.float32(2.0 ** -140)               # every entry subnormal (or flushed to zero by the rounding here)
    x[8] *= np.float32(2.0 ** -120)
    x[3] *= np.float32(2.0 ** 40)
    x[4] *= np.float32(2.0 ** 60)
    x[5] = x[6]
    reps = -(-n // REFINER_BASE_ROWS)
    out = np.concatenate([x if r % 2 == 0 else -x for r in range(reps)])[:n]
    return np.ascontiguousarray(out, np.float32)


HUGE_ROWS = (3, 4)        # rows of refiner_rows that a bias of -1e3 does not kill


def refiner_variants(depth: int) -> dict:
    """name -> refiner state dict at `depth` residual blocks: the plain synthetic state and five edits of it."""
    base = synth.refiner_state(3, n_blocks=depth)

    def edit(**kw):
        sd = dict(base)
        for k, v in kw.items():
            sd[k.replace("__", ".")] = np.full_like(base[k.replace("__", ".")], v)
        return sd
    return {
        "plain": base,
        "dead": edit(input_proj__bias=-1e3),                              # relu(input_proj) == 0 for every ordinary row
        "zero_out": edit(output_proj__weight=0.0, output_proj__bias=0.0),
        "bias_1e-30": edit(output_proj__weight=0.0, output_proj__bias=1e-30),   # sum of squares underflows to 0
        "bias_1e-20": edit(output_proj__weight=0.0, output_proj__bias=1e-20),   # subnormal squares, norm below the 1e-12 floor
        "bias_3e19": edit(output_proj__weight=0.0, output_proj__bias=3e19),     # squares overflow: the norm is +inf
    }


def refiner_depth(sd: dict) -> int:
    return len({k.split(".")[1] for k in sd if k.startswith("residual_blocks.")})


def bn_tokens_case(cells: int, frames: int, n_prefix: int = 5, seed: int = 0) -> np.ndarray:
    """(frames, n_prefix + cells, 384) tokens in the style of synth.tokens with four altered channels."""
    rng = synth._rng(92_000 + seed)
    tok = synth._normal(rng, (frames, n_prefix + cells, synth.C_FEAT), 3.0, 0.5)
    tok[..., 0] = np.float32(7.5)                                          # constant: variance exactly 0
    tok[..., 1] = (1e4 + 1e-3 * rng.standard_normal(tok.shape[:2])).astype(np.float32)   # ill-conditioned
    tok[..., 2] *= np.float32(2.0 ** -70)                                  # variance far below eps
    tok[0, :, 3] = np.float32(-2.25)                                       # constant in frame 0 only
    return tok


def bn_affine(seed: int):
    """Non-trivial gamma, beta, running mean and running variance, as in test_bn_tokens."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gamma = (1 + 0.1 * rng.standard_normal(synth.C_FEAT)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(synth.C_FEAT)).astype(np.float32)
    rmean = (0.2 * rng.standard_normal(synth.C_FEAT)).astype(np.float32)
    rvar = (1 + 0.3 * rng.random(synth.C_FEAT)).astype(np.float32)
    return gamma, beta, rmean, rvar
