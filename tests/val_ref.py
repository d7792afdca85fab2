"""Float64 numpy statement of the validation stage: the per-frame and per-pair statistics and their composition into the
trainer's seven loss terms, weighted total and five batch metrics.  Written from the formulas of the stage's specification
(DESIGN §4c), with every batch quantity evaluated DIRECTLY on the concatenated batch - no streaming update, no per-frame
partials - so that it checks the composition of sslam_amd.validation as well as the kernels."""
from __future__ import annotations

import numpy as np

WEIGHTS = dict(desc=8.0, repeat=0.3, variance=0.5, peakiness=0.1, activation=0.05, edge=0.3, sparsity=0.3)
TARGETS = dict(peakiness_variance=0.22, activation_mean=0.35, min_variance=0.005, sparsity_variation=0.15, high_saliency=0.6,
               high_ratio=0.20, sparsity_penalty=2.0)
TERMS = ("desc", "variance", "repeat", "peakiness", "activation", "edge", "sparsity")
METRICS = ("num_matches", "mean_saliency", "max_saliency", "saliency_variance", "descriptor_variance")
FLOOR = 2.0 ** -20


def tolerance(ref64, ref32=None, scale=None):
    """The one rule for every scalar: max(4 |ref32 - ref64|, 2^-20 max(1, |ref64|)); `scale` replaces |ref64| for an
    intermediate whose natural scale is larger than its value (named where it is used)."""
    s = np.maximum(1.0, np.abs(ref64) if scale is None else scale)
    t = FLOOR * s
    return t if ref32 is None else np.maximum(t, 4.0 * np.abs(np.asarray(ref32, np.float64) - ref64))


def f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------------------ statistics
def sims(d1, d2):
    """d1 d2^T in float64, every element by the same summation (no BLAS blocking): bit-identical rows - the duplicated
    keypoints of the real selector - give bit-identical similarities, so exact ties stay exact and arg-max takes the first."""
    a, b = f64(d1), f64(d2)
    return np.concatenate([(a[i:i + 32, None, :] * b[None, :, :]).sum(axis=-1) for i in range(0, len(a), 32)])


def logits(d1, d2, temperature):
    return np.clip(sims(d1, d2) / float(temperature), -50.0, 50.0)


def row_lse(d1, d2, temperature):
    """lse_i = log sum_j exp(x_ij) for every row of d1 (K1, 128) against d2 (K2, 128)."""
    x = logits(d1, d2, temperature)
    m = x.max(axis=1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=1))


def mutual(d1, d2):
    """(nn12, nn21, mask of the mutual nearest neighbours): first maxima, no thresholds."""
    s = sims(d1, d2)
    nn12, nn21 = s.argmax(axis=1), s.argmax(axis=0)
    return nn12, nn21, nn21[nn12] == np.arange(s.shape[0])


def pair_stats(sal_a, sal_b, d1, d2, temperature):
    x = logits(d1, d2, temperature)
    lse = row_lse(d1, d2, temperature)
    nn12, _, mask = mutual(d1, d2)
    idx = np.nonzero(mask)[0]
    return dict(repeat=float(np.mean((f64(sal_a) - f64(sal_b)) ** 2)), n_matches=int(mask.sum()),
                ce_sum=float(np.sum(lse[idx] - x[idx, nn12[idx]])), pad_ce=float(lse[0] - x[0, 0]))


def sobel_pool(img):
    """img (3, S, S) -> (P (G, G) block means of the Sobel magnitude, its maximum m); zero padding at the border."""
    c = f64(img)
    gray = 0.299 * c[0] + 0.587 * c[1] + 0.114 * c[2]
    s = gray.shape[0]
    p = np.zeros((s + 2, s + 2))
    p[1:-1, 1:-1] = gray
    gx = (p[:-2, 2:] - p[:-2, :-2]) + 2.0 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    gy = (p[2:, :-2] - p[:-2, :-2]) + 2.0 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    mag = np.sqrt(gx * gx + gy * gy + 1e-8)
    g = s // 16
    return mag.reshape(g, 16, g, 16).mean(axis=(1, 3)), float(mag.max())


def frame_stats(sal, img=None, desc=None):
    s = f64(sal)
    out = dict(sal_mean=float(s.mean()), sal_var=float(s.var()), sal_max=float(s.max()),
               sal_dx=float(np.abs(s[:, 1:] - s[:, :-1]).sum()), sal_dy=float(np.abs(s[1:, :] - s[:-1, :]).sum()),
               sal_high=float((np.asarray(sal) > np.float32(0.6)).sum()), sal_ss=float(((s - s.mean()) ** 2).sum()))
    if img is not None:
        P, m = sobel_pool(img)
        dp, ds = P - P.mean(), s - s.mean()
        out.update(pooled=P, edge_max=m, edge_mean=float(P.mean()), edge_a=float((dp * ds).sum()), edge_e=float((dp * dp).sum()))
    if desc is not None:
        d = f64(desc)
        out.update(desc_mean=d.mean(axis=0), desc_m2=((d - d.mean(axis=0)) ** 2).sum(axis=0))
    return out


def sobel_magnitude(img):
    """img (3, S, S) -> the (S, S) Sobel magnitude that sobel_pool pools: where the frame maximum sits."""
    c = f64(img)
    gray = 0.299 * c[0] + 0.587 * c[1] + 0.114 * c[2]
    s = gray.shape[0]
    p = np.zeros((s + 2, s + 2))
    p[1:-1, 1:-1] = gray
    gx = (p[:-2, 2:] - p[:-2, :-2]) + 2.0 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    gy = (p[2:, :-2] - p[:-2, :-2]) + 2.0 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    return np.sqrt(gx * gx + gy * gy + 1e-8)


def mutual_rows(nn12, nn21):
    """The mask of the rows i with 0 <= nn12[i] < len(nn21) and nn21[nn12[i]] == i, for ANY two integer arrays (n1,), (n2,):
    an index outside the second side names no row and is not mutual."""
    nn12, nn21 = np.asarray(nn12, np.int64), np.asarray(nn21, np.int64)
    ok = (nn12 >= 0) & (nn12 < len(nn21))
    mask = np.zeros(len(nn12), bool)
    idx = np.nonzero(ok)[0]
    mask[idx] = nn21[nn12[idx]] == idx
    return mask


def pair_sums(ce, nn12, nn21, s12_0, s00, temperature):
    """What val_pair_stats sums for one pair from given arrays: n_matches and ce_sum over mutual_rows(nn12, nn21), and
    pad_ce = ce[0] + (clamp(s12[0] / T) - clamp(s00 / T)) - in float64, for hand-made index arrays as for the device's own."""
    mask = mutual_rows(nn12, nn21)
    t = float(temperature)
    pad = float(f64(ce)[0] + (np.clip(float(s12_0) / t, -50.0, 50.0) - np.clip(float(s00) / t, -50.0, 50.0)))
    return dict(n_matches=int(mask.sum()), ce_sum=float(f64(ce)[mask].sum()), pad_ce=pad, mask=mask)


# ----------------------------------------------------------------------------------------------------------- composition
def batch_terms(sal1, sal2, images, d1, d2, temperature=0.1, weights=WEIGHTS, targets=TARGETS):
    """One batch as the trainer sees it: sal1, sal2 (B, G, G), images (B, 3, S, S), d1, d2 (B, K, 128) -> the seven terms,
    `total` and the five metrics, in float64."""
    B = len(sal1)
    T = targets
    s1 = f64(sal1)
    ps = [pair_stats(sal1[b], sal2[b], d1[b], d2[b], temperature) for b in range(B)]
    mmax = max(p["n_matches"] for p in ps)
    out = {}
    out["desc"] = float(np.mean([(p["ce_sum"] + (mmax - p["n_matches"]) * p["pad_ce"]) / mmax for p in ps]))
    flat = f64(d1).reshape(-1, f64(d1).shape[-1])
    out["variance"] = max(0.0, T["min_variance"] - float(flat.var(axis=0, ddof=1).mean()))
    out["repeat"] = float(np.mean([p["repeat"] for p in ps]))
    out["peakiness"] = (float(np.mean([s1[b].var() for b in range(B)])) - T["peakiness_variance"]) ** 2
    out["activation"] = (float(s1.mean()) - T["activation_mean"]) ** 2
    pm = [sobel_pool(images[b]) for b in range(B)]
    c = 1.0 / (max(m for _, m in pm) + 1e-8)
    corr = []
    for b in range(B):
        dp, ds = pm[b][0] - pm[b][0].mean(), s1[b] - s1[b].mean()
        corr.append(c * (dp * ds).sum() / (c * np.sqrt((dp * dp).sum() * (ds * ds).sum()) + 1e-8))
    out["edge"] = -float(np.mean(corr))
    variation = (np.abs(s1[:, :, 1:] - s1[:, :, :-1]).mean() + np.abs(s1[:, 1:, :] - s1[:, :-1, :]).mean()) / 2.0
    ratio = float((np.asarray(sal1) > np.float32(T["high_saliency"])).mean())
    out["sparsity"] = max(0.0, T["sparsity_variation"] - float(variation)) + max(0.0, ratio - T["high_ratio"]) * T["sparsity_penalty"]
    out["total"] = float(sum(weights[k] * out[k] for k in TERMS))
    out.update(num_matches=float(mmax), mean_saliency=float(s1.mean()), max_saliency=float(s1.max()),
               saliency_variance=float(s1.var()), descriptor_variance=float(flat.var()))
    return out


def validate(saliency, images, desc, first, second, batch=4, temperature=0.1, weights=WEIGHTS, targets=TARGETS):
    """The mean over batches of `batch` pairs (a last short batch kept) of batch_terms: what the trainer's validate() returns."""
    first, second = np.asarray(first), np.asarray(second)
    rows = []
    for a in range(0, len(first), batch):
        f, s = first[a:a + batch], second[a:a + batch]
        rows.append(batch_terms(saliency[f], saliency[s], images[f], desc[f], desc[s], temperature, weights, targets))
    return {k: float(np.mean([r[k] for r in rows])) for k in rows[0]}


def stats_dict(saliency, images, desc, first, second, temperature=0.1):
    """The dictionary SequencePipeline.validation_stats returns, in float64 on the host: what compose takes."""
    fs = [frame_stats(saliency[i], images[i], desc[i]) for i in range(len(saliency))]
    ps = [pair_stats(saliency[a], saliency[b], desc[a], desc[b], temperature) for a, b in zip(first, second)]
    out = {k: np.array([f[k] for f in fs]) for k in ("sal_mean", "sal_var", "sal_max", "sal_dx", "sal_dy", "sal_high", "sal_ss",
                                                     "edge_a", "edge_e", "edge_mean", "edge_max", "desc_mean", "desc_m2", "pooled")}
    out.update({k: np.array([p[k] for p in ps]) for k in ("repeat", "n_matches", "ce_sum", "pad_ce")})
    out.update(first=np.asarray(first, np.int32), second=np.asarray(second, np.int32), grid=saliency.shape[1],
               num_keypoints=desc.shape[1], temperature=float(temperature))
    return out


# ---------------------------------------------------------------------------------------------------------- golden cases
GOLDEN_MEAN = np.array([0.485, 0.456, 0.406], np.float32).reshape(1, 3, 1, 1)
GOLDEN_STD = np.array([0.229, 0.224, 0.225], np.float32).reshape(1, 3, 1, 1)


def golden_case(z, name):
    """One case of tests/golden/val_losses.npz as a bank of 8 frames (the four first frames, then the four second frames) and
    the pair lists (b, 4 + b): saliency (8, G, G), fp32 images (8, 3, S, S) - the second frames' images are never read by a
    term; the first frames' are repeated - descriptors (8, K, 128)."""
    img = ((z[f"{name}_u8"].astype(np.float32) / np.float32(255.0)) - GOLDEN_MEAN) / GOLDEN_STD
    return dict(saliency=np.concatenate([z[f"{name}_sal1"], z[f"{name}_sal2"]]), images=np.concatenate([img, img]),
                desc=np.concatenate([z[f"{name}_d1"], z[f"{name}_d2"]]), first=np.arange(4, dtype=np.int32),
                second=np.arange(4, 8, dtype=np.int32), temperature=float(z[f"{name}_temperature"]),
                order=[str(k) for k in z["order"]])
