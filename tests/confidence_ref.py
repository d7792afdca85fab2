"""The keypoint confidence head of libsslam_conf.so (include/sslam_conf.h) restated in numpy, operation by operation in the header's
order: the CPU side of every bit-for-bit comparison in tests/test_gpu_confidence.py, and what tests/test_confidence_cpu.py holds
against the reference's own outputs (tests/golden/confidence.npz).  The fused multiply-add is the correctly rounded float32 one
built from float64 (fmaf32 of tests/loop_ref.py); the gather and the sigmoid are the oracle's (ora.gather, ora.sigmoid).
No torch, no GPU.
"""
import numpy as np

from loop_ref import fmaf32
from oracle import ora

DINO_DIM, HIDDEN_DIM, WIDTHS, FILTER_MAX_K = 384, 128, (128, 256), 4096
STATE_KEYS = ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias")


def weight_list(sd):
    """The six float32 arrays of a head's state_dict (numpy arrays or tensors), in STATE_KEYS' order."""
    return [np.ascontiguousarray(np.asarray(sd[k].detach().cpu() if hasattr(sd[k], "detach") else sd[k]), np.float32) for k in STATE_KEYS]


def linear_chain(x, w, b):
    """(rows, k) x (n, k), (n) -> (rows, n): per output ONE fma chain in increasing k, starting from the bias."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    acc = np.broadcast_to(np.asarray(b, np.float32), (x.shape[0], w.shape[0])).copy()
    for k in range(x.shape[1]):
        acc = fmaf32(x[:, k:k + 1], w[None, :, k], acc)
    return acc


def relu(v):
    """v > 0 ? v : +0.0f (a NaN and -0.0f give +0.0f)."""
    return np.where(v > 0, v, np.float32(0.0)).astype(np.float32)


def sigmoid(v):
    """The canonical sigmoid of the project, element by element."""
    v = np.asarray(v, np.float32)
    return np.array([ora.sigmoid(t) for t in v.ravel()], np.float32).reshape(v.shape)


CONF_MIN = np.float32(1.17549435e-38)      # SSLC_CONF_MIN: the least normal float32


def output(logit):
    """logit -> confidence: the canonical sigmoid, a subnormal result (its floor 6.05e-39 at saturated negative logits) written as +0."""
    s = sigmoid(logit)
    return np.where(s < CONF_MIN, np.float32(0.0), s).astype(np.float32)


def logits(x, desc, weights):
    """x (rows, 384), desc (rows, d), weights as weight_list -> the float32 logit of every row."""
    w1, b1, w2, b2, w3, b3 = weights
    row = np.concatenate([np.asarray(x, np.float32), np.asarray(desc, np.float32)], axis=1)
    assert row.shape[1] == w1.shape[1]
    h1 = relu(linear_chain(row, w1, b1))
    h2 = relu(linear_chain(h1, w2, b2))
    return linear_chain(h2, w3, b3)[:, 0]


def confidence_rows(x, desc, weights):
    """sslc_confidence_rows: x (..., 384), desc (..., d) -> confidence (...)."""
    x, desc = np.asarray(x, np.float32), np.asarray(desc, np.float32)
    lead = x.shape[:-1]
    return output(logits(x.reshape(-1, x.shape[-1]), desc.reshape(-1, desc.shape[-1]), weights)).reshape(lead)


def gather_confidence(feat, kp, desc, weights):
    """sslc_gather_confidence: feat (n, G, G, 384), kp (n, K, 2), desc (n, K, d) -> (n, K)."""
    return confidence_rows(ora.gather(feat, kp), desc, weights)


def confidence_f64(x, desc, weights):
    """The same head in float64, plain matrix products: the yardstick both the reference and the restatement are measured against."""
    w1, b1, w2, b2, w3, b3 = [np.asarray(w, np.float64) for w in weights]
    row = np.concatenate([np.asarray(x, np.float64), np.asarray(desc, np.float64)], axis=-1)
    h = np.maximum(row @ w1.T + b1, 0)
    h = np.maximum(h @ w2.T + b2, 0)
    return 1.0 / (1.0 + np.exp(-(h @ w3.T + b3)[..., 0]))


def confidence_filter(conf, threshold):
    """sslc_confidence_filter: conf (n, K) -> slot (n, K) int32, count (n) int32, conf_out (n, K) float32."""
    conf = np.asarray(conf, np.float32)
    n, K = conf.shape
    thr = np.float32(threshold)
    slot, count, out = np.zeros((n, K), np.int32), np.zeros(n, np.int32), np.zeros((n, K), np.float32)
    for f in range(n):
        with np.errstate(invalid="ignore"):
            kept = np.flatnonzero(conf[f] >= thr)
        if len(kept) == 0:
            kept = np.array([np.argmax(np.where(np.isnan(conf[f]), -np.inf, conf[f]))])       # the first of equal maxima
        c = len(kept)
        count[f] = c
        slot[f, :c] = kept
        slot[f, c:] = kept[-1]
        out[f, :c] = conf[f, kept]
    return slot, count, out


def take_rows(src, slot):
    """sslc_take_rows: src (n, K, ...) and slot (n, K) -> dst[f, j] = src[f, slot[f, j]]; a slot outside 0 .. K - 1 gives zero words."""
    src, slot = np.asarray(src), np.asarray(slot)
    K = src.shape[1]
    ok = (slot >= 0) & (slot < K)
    dst = np.take_along_axis(src, np.where(ok, slot, 0).reshape(slot.shape + (1,) * (src.ndim - 2)).astype(np.int64), axis=1)
    dst[~ok] = 0
    return dst


def filter_padded(arrays, conf, threshold):
    """filter_keypoints_by_confidence's return, from the device entries' outputs: each array of `arrays` (n, K, ...) taken through
    slot and cut to the largest count, and the confidence (n, M, 1)."""
    slot, count, out = confidence_filter(conf, threshold)
    m = int(count.max())
    return [take_rows(a, slot)[:, :m] for a in arrays], out[:, :m, None]


def calibration_loss(conf, err, eps=1e-6):
    """compute_calibration_loss in float64: mean((conf - (1 - err / (max err + eps)))^2); conf (B, N, 1), err (B, N)."""
    conf, err = np.asarray(conf, np.float64), np.asarray(err, np.float64)
    target = 1.0 - (err / (err.max() + eps))[..., None]
    return float(np.mean((conf - target) ** 2))


def expected_error_loss(conf, err):
    """compute_expected_error_loss in float64: mean |1 / (conf + 1e-6) - 1 - err|."""
    conf, err = np.asarray(conf, np.float64), np.asarray(err, np.float64)
    return float(np.mean(np.abs(1.0 / (conf[..., 0] + 1e-6) - 1.0 - err)))
