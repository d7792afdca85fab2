"""Checker of the bf16 THROUGHPUT mode (BASELINE.json configs[1] "bf16 conv stack").

TEST INFRASTRUCTURE ONLY, like the rest of oracle/: imported by tests/ (and nothing else), never by the product package.

The mode's definition = the reference's algorithm (saliency CNN: semantic-slam/models/keypoint_selector.py:45-67; descriptor
MLP: semantic-slam/models/descriptor_refiner.py:58-126) with every GEMM operand rounded to bf16 (round-to-nearest-even) and
the products accumulated exactly (float64 here, fp32 on the GPU): what separates a correct kernel from this restatement is
fp32 accumulation-order noise only.  It is pinned against the exact oracle / the reference's own golden outputs by
tests/test_oracle_golden.py::test_bf16_mode_checker_tracks_the_exact_oracle (a drift bound: bf16 operands move the saliency
by < 3e-2 and keep descriptor cosines > 0.999) - the bf16 mode is not bit-comparable to the fp32 reference by construction.
"""
from __future__ import annotations

import numpy as np


def bf16_round(a):
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def saliency_bf16_ref(feat, sd):
    """conv3x3 (bf16 operands, float64 accumulate) + ReLU + conv1x1 + sigmoid (keypoint_selector.py:45-67)."""
    n, g, _, c = feat.shape
    x = np.zeros((n, g + 2, g + 2, c), np.float64)
    x[:, 1:-1, 1:-1] = bf16_round(feat)
    w = bf16_round(sd["conv.0.weight"]).astype(np.float64)          # (hs, c, 3, 3)
    hid = np.zeros((n, g, g, w.shape[0]), np.float64) + sd["conv.0.bias"].astype(np.float64)
    for ky in range(3):
        for kx in range(3):
            hid += x[:, ky:ky + g, kx:kx + g] @ w[:, :, ky, kx].T
    hid = np.maximum(hid.astype(np.float32), 0).astype(np.float64)
    logit = hid @ sd["conv.2.weight"].reshape(-1).astype(np.float64) + float(sd["conv.2.bias"].reshape(-1)[0])
    return (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)


def refine_bf16_ref(x, sd, n_blocks=2):
    """The bf16 kernel's formulation in float64: bf16 GEMM operands, LayerNorm folded into the next GEMM
    (descriptor_refiner.py:58-126 algebraically; refine_bf16.hip header)."""
    f8 = np.float64

    def lin(a, W, b):
        return bf16_round(a.astype(np.float32)).astype(f8) @ bf16_round(W).astype(f8).T + b.astype(f8)

    def ln_lin(a, gam, bet, W, b):
        a32 = a.astype(np.float32).astype(f8)
        mean = a32.mean(-1, keepdims=True)
        var = np.maximum((a32 * a32).mean(-1, keepdims=True) - mean * mean, 0)
        rstd = 1.0 / np.sqrt(var + 1e-5)
        wg = bf16_round((W * gam[None, :]).astype(np.float32)).astype(f8)
        c = b.astype(f8) + W.astype(f8) @ bet.astype(f8)
        return rstd * (bf16_round(a.astype(np.float32)).astype(f8) @ wg.T - mean * wg.sum(1)[None, :]) + c[None, :]

    X = np.maximum(lin(x, sd["input_proj.weight"], sd["input_proj.bias"]), 0)
    for i in range(n_blocks):
        p = f"residual_blocks.{i}."
        h = np.maximum(ln_lin(X, sd[p + "norm1.weight"], sd[p + "norm1.bias"], sd[p + "fc1.weight"], sd[p + "fc1.bias"]), 0)
        X = np.maximum(ln_lin(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"], sd[p + "fc2.weight"], sd[p + "fc2.bias"]) + X, 0)
    o = lin(X, sd["output_proj.weight"], sd["output_proj.bias"])
    return (o / np.maximum(np.sqrt((o * o).sum(-1, keepdims=True)), 1e-12)).astype(np.float32)


def refine_bf16_f32acc(x, sd, n_blocks=2, order=0, after_input_proj=None):
    """refine_bf16_ref with every accumulator, row statistic and epilogue held in fp32, as the kernel holds them - in an order
    of its own, NOT the device's: what it measures is how far fp32 accumulation alone moves the mode away from the float64
    checker (bf16 roundings of the activations that flip, and what a flip costs), so that a test can take its bounds from the
    reference side alone.  Two orders, to see how much the figures depend on one:
      order 0: k ascending in steps of 16 (one rounding of the accumulator per step), row sums pairwise;
      order 1: k descending in the same steps (the MFMA instruction takes 16 k at a time: one rounding of the accumulator per
               instruction is the granularity of the hardware), row sums from the last column: chains of 32 columns, then a
               chain over the chains (the kernel reduces a row through a tree of depth ~8 over lanes and waves; one chain over
               all 384 columns is outside the family of orders the hardware can take and doubles every figure).
    Within a step the products are summed in float64 (exact for practical purposes), so the result does not depend on the
    BLAS underneath.  after_input_proj: optional function applied to the fp32 ReLU output of input_proj, (rows, 384), before
    it is written to the bf16 tile - for tests that emulate a fault there."""
    f4, f8 = np.float32, np.float64
    step = 16
    starts = list(range(0, 384, step))
    if order:
        starts.reverse()

    def rowsum(a):                                                   # (rows, n) fp32 -> (rows, 1) fp32
        if order == 0:
            return a.sum(-1, keepdims=True, dtype=f4)
        part = np.cumsum(a[:, ::-1].reshape(a.shape[0], -1, 32), axis=2, dtype=f4)[:, :, -1]
        return np.cumsum(part, axis=1, dtype=f4)[:, -1:]

    def gemm(a, wq, start):                                          # bf16 operands, fp32 accumulator rounded once per k-step
        aq = bf16_round(a).astype(f8)
        acc = np.broadcast_to(start.astype(f4), (a.shape[0], wq.shape[0])).copy()
        for k in starts:
            acc = (acc.astype(f8) + aq[:, k:k + step] @ wq[:, k:k + step].T).astype(f4)
        return acc

    def ln_lin(a, gam, bet, W, b):                                   # a: fp32 activations of the previous layer
        mean = rowsum(a) / f4(384.0)
        var = np.maximum(rowsum(a * a) / f4(384.0) - mean * mean, f4(0.0))
        rstd = f4(1.0) / np.sqrt(var + f4(1e-5))
        wg = bf16_round((W * gam[None, :]).astype(f4))
        c = (b.astype(f8) + W.astype(f8) @ bet.astype(f8)).astype(f4)
        cs = wg.astype(f8).sum(1).astype(f4)
        acc = gemm(a, wg.astype(f8), np.zeros(W.shape[0], f4))
        return rstd * (acc - mean * cs[None, :]) + c[None, :]

    X = np.maximum(gemm(np.asarray(x, f4), bf16_round(sd["input_proj.weight"]).astype(f8), sd["input_proj.bias"]), f4(0.0))
    if after_input_proj is not None:
        X = np.asarray(after_input_proj(X), f4)
    for i in range(n_blocks):
        p = f"residual_blocks.{i}."
        h = np.maximum(ln_lin(X, sd[p + "norm1.weight"], sd[p + "norm1.bias"], sd[p + "fc1.weight"], sd[p + "fc1.bias"]), f4(0.0))
        X = np.maximum(ln_lin(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"], sd[p + "fc2.weight"], sd[p + "fc2.bias"]) + X, f4(0.0))
    o = gemm(X, bf16_round(sd["output_proj.weight"]).astype(f8), sd["output_proj.bias"])
    return o / np.maximum(np.sqrt(rowsum(o * o)), f4(1e-12))


def saliency_bf16_f32acc(feat, sd, order=0):
    """saliency_bf16_ref with the conv accumulator and the 1x1 layer held in fp32, in an order of its own (NOT the device's):
    one rounding of the accumulator per 16 channels of a tap (the MFMA instruction's granularity), steps ascending (order 0) or
    descending (order 1); the 256 products of the 1x1 layer summed pairwise or as one chain."""
    n, g, _, c = feat.shape
    x = np.zeros((n, g + 2, g + 2, c), np.float64)
    x[:, 1:-1, 1:-1] = bf16_round(feat)
    w = bf16_round(sd["conv.0.weight"]).astype(np.float64)
    steps = [(ky, kx, c0) for c0 in range(0, c, 16) for ky in range(3) for kx in range(3)]
    if order:
        steps.reverse()
    acc = np.zeros((n, g, g, w.shape[0]), np.float32) + sd["conv.0.bias"].astype(np.float32)
    for ky, kx, c0 in steps:
        acc = (acc.astype(np.float64) + x[:, ky:ky + g, kx:kx + g, c0:c0 + 16] @ w[:, c0:c0 + 16, ky, kx].T).astype(np.float32)
    p = np.maximum(acc, np.float32(0)) * sd["conv.2.weight"].reshape(-1).astype(np.float32)
    logit = (np.cumsum(p, axis=-1, dtype=np.float32)[..., -1] if order else p.sum(-1, dtype=np.float32)) + np.float32(sd["conv.2.bias"].reshape(-1)[0])
    return (1.0 / (1.0 + np.exp(-logit.astype(np.float64)))).astype(np.float32)


def refine_error_structure(desc, ref, tile=64):
    """Where a descriptor array (rows, 128) departs from the float64 checker: the figures a correct kernel keeps at a few fp32
    ulps (medians per 64-row tile, per output column, per 32-column slab of one wave) and the rare-event figures (share of rows
    with a difference above 1e-5 - a flipped bf16 rounding - overall, in the worst tile and in the worst group of four
    consecutive tiles; the largest difference)."""
    d = np.abs(np.asarray(desc, np.float64) - np.asarray(ref, np.float64))
    rows = d.shape[0]
    hit = d.max(-1) > 1e-5
    n_tiles = (rows + tile - 1) // tile
    return {"tile_median": max(float(np.median(d[t * tile:(t + 1) * tile])) for t in range(n_tiles)),
            "column_median": float(np.median(d, axis=0).max()),
            "slab_median": max(float(np.median(d[:, s * 32:(s + 1) * 32])) for s in range(d.shape[1] // 32)),
            "rows_hit": float(hit.mean()),
            "tile_rows_hit": max(float(hit[t * tile:(t + 1) * tile].mean()) for t in range(n_tiles)),
            "tile4_rows_hit": max(float(hit[t * tile:(t + 4) * tile].mean()) for t in range(0, n_tiles, 4)),
            "max": float(d.max())}
