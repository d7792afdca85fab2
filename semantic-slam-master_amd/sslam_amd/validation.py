"""Checkpoint validation: the reference's SemanticSLAMTrainer.validate() (train.py:451-499) from the statistics of the HIP
validation stage (SequencePipeline.validation_stats; csrc/validate.hip).

The trainer scores a checkpoint by running _forward_pass (train.py:292-408) under no_grad over batches of B frame pairs and
averaging, per batch, the seven terms of losses/self_supervised.py, their weighted total and five metrics.  Every one of
those is a function of a few numbers per frame and per pair; the device produces these numbers, and `compose` - a small host
function in float64 - puts them together for any batch size:

  per frame a (the FIRST frame of a pair: the trainer evaluates the single-frame terms on saliency1 / desc1 / rgb1)
    peakiness   (mean_b var_b - target)^2                                  var_b the biased variance of the saliency map
    activation  (mean_b mean_b - target)^2
    sparsity    relu(0.15 - (sum_b dx_b / (B G (G-1)) + sum_b dy_b / (B (G-1) G)) / 2) + relu(sum_b high_b / (B G^2) - 0.20) penalty
    edge        -mean_b corr_b,  corr_b = c A_b / (c sqrt(E_b Ss_b) + 1e-8),  c = 1 / (max_b m_b + 1e-8)
                (a constant saliency map has A = Ss = 0: corr = 0, never NaN)
    variance    relu(min_variance - mean_d var_d), var_d the unbiased variance of dimension d over the B K rows: the frames'
                (mean, centred sum of squares) combined by the pairwise update
  per pair (a, b)
    repeat      mean_b mse_b
    desc        mean_b (ce_sum_b + (Mmax - n_b) pad_ce_b) / Mmax,  Mmax = max_b n_b: the trainer zero-pads the match lists
                to the longest of the batch (train.py:437-447) and the loss counts the (0, 0) rows as matches
  metrics       num_matches = Mmax, mean_saliency, max_saliency, saliency_variance (np.var over the batch),
                descriptor_variance (np.var over all B K D elements, D = the descriptor width of the statistics: 128 or 256)

The reference's branch for a batch without any match (train.py:439-440, self_supervised.py:71) is not built: the global
maximum of a similarity matrix of finite descriptors is always a mutual nearest neighbour, so every pair has n >= 1.

Defaults are the reference's configuration values (configs/train_config.yaml:52-79 and train.py:91), passed as numbers.
"""
from __future__ import annotations

import numpy as np

from . import lib
from .pipeline import _np

TERMS = ("desc", "variance", "repeat", "peakiness", "activation", "edge", "sparsity")
METRICS = ("num_matches", "mean_saliency", "max_saliency", "saliency_variance", "descriptor_variance")
# configs/train_config.yaml:53-60
WEIGHTS = dict(desc=8.0, repeat=0.3, variance=0.5, peakiness=0.1, activation=0.05, edge=0.3, sparsity=0.3)
# target_variance :70, sparsity_target :73 (the trainer hands it to ActivationLoss, train.py:99-101), DescriptorVarianceLoss
# min_variance train.py:91, the constants of SpatialSparsityLoss.forward (self_supervised.py:305-310) and sparsity_penalty :79
TARGETS = dict(peakiness_variance=0.22, activation_mean=0.35, min_variance=0.005, sparsity_variation=0.15, high_ratio=0.20,
               sparsity_penalty=2.0)
TEMPERATURE = 0.10      # desc_temperature :63
BATCH = 4               # training.batch_size :84

_FRAME_KEYS = ("sal_mean", "sal_var", "sal_max", "sal_dx", "sal_dy", "sal_high", "sal_ss", "edge_a", "edge_e", "edge_max",
               "desc_mean", "desc_m2")
_PAIR_KEYS = ("first", "repeat", "n_matches", "ce_sum", "pad_ce")


def _check_batch(batch) -> int:
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"batch must be an integer >= 1, got {batch!r}")
    return int(batch)


def combine_moments(mean, m2, rows: int):
    """Frames' per-dimension (mean, centred sum of squares) over `rows` rows each, (B, D) float64 -> those of the B * rows rows
    together, by the pairwise update n = na + nb, d = mean_b - mean_a, mean = mean_a + d nb / n, M2 = M2a + M2b + d^2 na nb / n."""
    n, mu, q = float(rows), mean[0].copy(), m2[0].copy()
    for b in range(1, len(mean)):
        d = mean[b] - mu
        tot = n + rows
        mu = mu + d * (rows / tot)
        q = q + m2[b] + d * d * (n * rows / tot)
        n = tot
    return mu, q, n


def compose(stats: dict, batch: int = BATCH, weights: dict | None = None, targets: dict | None = None) -> dict:
    """stats: what SequencePipeline.validation_stats returned (device tensors; read back here, once), or the same keys as
    host arrays.  The pairs are taken `batch` at a time in list order, as a DataLoader without shuffling collates them.
    Returns a dict of float64 arrays with one entry per batch: the seven components under the trainer's names, `total`, and
    the five metrics.  ValueError: batch < 1, a pair count that is no multiple of `batch` (validate() handles a short last
    batch), an absent (-1) pair, which has no loss."""
    batch = _check_batch(batch)
    w = dict(WEIGHTS, **(weights or {}))
    t = dict(TARGETS, **(targets or {}))
    missing = [k for k in _FRAME_KEYS + _PAIR_KEYS + ("grid", "num_keypoints") if k not in stats]
    if missing:
        raise ValueError(f"stats lack {missing}: pass the dictionary of validation_stats")
    g, k = int(stats["grid"]), int(stats["num_keypoints"])
    fr = {key: _np(stats[key]).astype(np.float64) for key in _FRAME_KEYS}
    first = _np(stats["first"]).astype(np.int64)
    pr = {key: _np(stats[key]).astype(np.float64) for key in ("repeat", "n_matches", "ce_sum", "pad_ce")}
    n_pairs, n_frames = first.shape[0], fr["sal_mean"].shape[0]
    if n_pairs == 0 or n_pairs % batch:
        raise ValueError(f"{n_pairs} pairs do not make whole batches of {batch}: ragged last batch")
    if "second" in stats:
        second = _np(stats["second"]).astype(np.int64)
        if ((second < 0) | (second >= n_frames)).any():
            raise ValueError("an absent pair (index outside the bank) has no loss: list present pairs only")
    if ((first < 0) | (first >= n_frames)).any():
        raise ValueError("an absent pair (index outside the bank) has no loss: list present pairs only")
    nb = n_pairs // batch
    out = {key: np.empty(nb, np.float64) for key in TERMS + ("total",) + METRICS}
    cells = float(g * g)
    for i in range(nb):
        sl = slice(i * batch, (i + 1) * batch)
        a = first[sl]
        n, mmax = pr["n_matches"][sl], pr["n_matches"][sl].max()
        out["desc"][i] = np.mean((pr["ce_sum"][sl] + (mmax - n) * pr["pad_ce"][sl]) / mmax)
        mu, q, rows = combine_moments(fr["desc_mean"][a], fr["desc_m2"][a], k)
        out["variance"][i] = max(0.0, t["min_variance"] - float(np.mean(q / (rows - 1.0)))) if rows > 1 else float("nan")
        out["repeat"][i] = pr["repeat"][sl].mean()
        out["peakiness"][i] = (fr["sal_var"][a].mean() - t["peakiness_variance"]) ** 2
        out["activation"][i] = (fr["sal_mean"][a].mean() - t["activation_mean"]) ** 2
        c = 1.0 / (fr["edge_max"][a].max() + 1e-8)
        out["edge"][i] = -np.mean(c * fr["edge_a"][a] / (c * np.sqrt(fr["edge_e"][a] * fr["sal_ss"][a]) + 1e-8))
        if g > 1:
            variation = (fr["sal_dx"][a].sum() + fr["sal_dy"][a].sum()) / (batch * g * (g - 1.0)) / 2.0
        else:
            variation = float("nan")      # the mean of an empty gradient, as in the reference
        ratio = fr["sal_high"][a].sum() / (batch * cells)
        out["sparsity"][i] = max(0.0, t["sparsity_variation"] - variation) + max(0.0, ratio - t["high_ratio"]) * t["sparsity_penalty"]
        out["total"][i] = sum(w[key] * out[key][i] for key in TERMS)
        out["num_matches"][i] = mmax
        sm = fr["sal_mean"][a].mean()
        out["mean_saliency"][i] = sm
        out["max_saliency"][i] = fr["sal_max"][a].max()
        out["saliency_variance"][i] = fr["sal_var"][a].mean() + np.mean((fr["sal_mean"][a] - sm) ** 2)
        gm = mu.mean()
        out["descriptor_variance"][i] = (q.sum() + rows * ((mu - gm) ** 2).sum()) / (rows * mu.shape[0])
    return out


def _slice_pairs(stats: dict, a: int, b: int) -> dict:
    out = dict(stats)
    for key in _PAIR_KEYS + ("second",):
        if key in out:
            out[key] = out[key][a:b]
    return out


def validate(pipe, images_u8, spacing: int = 1, batch: int = BATCH, temperature: float = TEMPERATURE, weights: dict | None = None,
             targets: dict | None = None, first=None, second=None, tokens=None) -> dict:
    """The dictionary SemanticSLAMTrainer.validate() returns - `total`, the seven components and the five metrics, each the
    mean over the batches - for the frames images_u8 (N, H, W, 3) uint8 and the pairs (i, i + spacing), or the listed pairs
    first / second, `batch` pairs per batch with a last short batch kept, like a DataLoader without drop_last.
    `pipe` is a SequencePipeline built with vit= (images in), or tokens= gives the ViT tokens (N, 5 + G*G, 384) of the frames, as
    SequencePipeline.run takes them; extraction, matching and the validation stage run on the device,
    and the one read-back is that of the per-frame and per-pair numbers."""
    batch = _check_batch(batch)
    lib.check_temperature(temperature)
    out = pipe.extract(pipe.tokens_from_images(images_u8) if tokens is None else tokens, None)
    if first is not None or second is not None:
        stats = pipe.validation_stats(out, images_u8, first=first, second=second, temperature=temperature)
    else:
        stats = pipe.validation_stats(out, images_u8, spacing=spacing, temperature=temperature)
    return reduce_batches(stats, batch, weights, targets)


def reduce_batches(stats: dict, batch: int = BATCH, weights: dict | None = None, targets: dict | None = None) -> dict:
    """compose over whole batches plus one short last batch, averaged over the batches with equal weight (train.py:489-497)."""
    batch = _check_batch(batch)
    n_pairs = int(stats["first"].shape[0])
    whole = n_pairs // batch * batch
    parts = []
    if whole:
        parts.append(compose(_slice_pairs(stats, 0, whole), batch, weights, targets))
    if n_pairs > whole:
        parts.append(compose(_slice_pairs(stats, whole, n_pairs), n_pairs - whole, weights, targets))
    if not parts:
        raise ValueError("no pairs to validate")
    return {key: float(np.concatenate([p[key] for p in parts]).mean()) for key in ("total",) + TERMS + METRICS}
