"""Seeded heads and inputs of the confidence-head tests, shared by tests/golden/make_golden_confidence.py (which runs the reference
on them and stores its outputs in tests/golden/confidence.npz) and by the tests (which regenerate them): the fixture holds the
reference's results only.  No torch, no GPU.
"""
import numpy as np

DINO_DIM, HIDDEN_DIM = 384, 128
B, N = 2, 64
# head -> (descriptor_dim, seed, scale): `default` is drawn as nn.Linear draws its default init (weights and biases uniform in
# +-1 / sqrt(fan_in)); `x4` is such a draw with every parameter multiplied by 4: its logits spread over +-14
HEADS = {"default": (128, 11, 1.0), "x4": (128, 12, 4.0), "wide": (256, 13, 1.0)}
FILTER_HEAD = "x4"          # the head whose confidences the stored filter outputs were computed from
TIE_SLOT = (0, 5)           # the stored confidence the `tie` threshold equals
STATE_KEYS = ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias")


def head_state(name):
    """The state_dict of a head as float32 numpy arrays."""
    d, seed, scale = HEADS[name]
    rng = np.random.default_rng(seed)
    h = HIDDEN_DIM
    out = {}
    for key, (n_out, n_in) in zip(("mlp.0", "mlp.2", "mlp.4"), ((h, DINO_DIM + d), (h // 2, h), (1, h // 2))):
        bound = 1.0 / np.sqrt(n_in)
        out[key + ".weight"] = (rng.uniform(-bound, bound, (n_out, n_in)) * scale).astype(np.float32)
        out[key + ".bias"] = (rng.uniform(-bound, bound, n_out) * scale).astype(np.float32)
    return out


def head_inputs(name):
    """(features (B, N, 384) standard normal, descriptors (B, N, d) of unit length, keypoints (B, N, 2) in 0 .. 27) float32."""
    d, seed, _ = HEADS[name]
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal((B, N, DINO_DIM)).astype(np.float32)
    desc = rng.standard_normal((B, N, d))
    desc = (desc / np.linalg.norm(desc, axis=-1, keepdims=True)).astype(np.float32)
    kp = rng.uniform(0, 27, (B, N, 2)).astype(np.float32)
    return x, desc, kp


def error_array():
    """(B, N) non-negative errors for the two losses."""
    return np.random.default_rng(77).exponential(1.5, (B, N)).astype(np.float32)


def thresholds(conf):
    """name -> threshold for the stored filter outputs, from the reference's confidences (B, N) of FILTER_HEAD."""
    conf = np.asarray(conf, np.float32)
    return {"half": np.float32(0.5), "median": np.float32(np.median(conf)), "tie": conf[TIE_SLOT], "none": np.float32(2.0)}
