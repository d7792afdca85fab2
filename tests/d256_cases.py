"""Inputs of the descriptor-width-256 tests, shared by the fixture generator (tests/golden/make_golden_d256.py), the CPU oracle
test and the GPU tests.  numpy only, everything from seeds: tests/golden/d256.npz stores the reference's OUTPUTS alone."""
import numpy as np

import synth

D = 256
REFINER_SEED = 3
PAIRS = {"p200x190": (31, 200, 190, 12), "p500x480": (32, 500, 480, 20)}      # tag: (seed, n1, n2, duplicated rows)
M3_CASES = ((41, 0.2), (42, 0.6), (43, 1.5), (44, 0.9))                       # (seed, noise): B = 4 pairs of 200 x 200
GATHER_GRID, GATHER_K = 8, 66


def refiner_state(n_blocks: int = 2) -> dict:
    return synth.refiner_state(REFINER_SEED, d_out=D, n_blocks=n_blocks)


def pair(seed: int, n: int, m: int, dup: int, noise: float = 0.25, d: int = D):
    """synth.descriptor_pair at width d: two sets with known correspondences, duplicated rows (exact ties), scores, intensities."""
    d1 = synth.unit_descriptors(seed, n, d, dup)
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    perm = (rng.permutation(max(n, m)) % n)[:m]
    d2 = d1[perm] + noise * rng.standard_normal((m, d)).astype(np.float32) / np.sqrt(d).astype(np.float32)
    d2 = (d2 / np.linalg.norm(d2.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    if dup:
        d2[m - dup // 2:] = d2[: dup // 2]
    s1 = (0.2 + 0.8 * rng.random(n)).astype(np.float32)
    s2 = (0.2 + 0.8 * rng.random(m)).astype(np.float32)
    return d1, d2, s1, s2, rng.random(n).astype(np.float32), rng.random(m).astype(np.float32)


# the reference's M1 under its default, its command-line, a tight and an empty threshold set, with and without intensity
RUNS = {
    "default": lambda i1, i2: dict(),
    "cli": lambda i1, i2: dict(saliency_weight=0.3, min_saliency=0.5, min_descriptor_sim=0.7, intensity1=i1, intensity2=i2,
                               min_intensity=0.15),
    "tight": lambda i1, i2: dict(min_saliency=0.75, min_descriptor_sim=0.9, intensity1=i1, intensity2=i2, min_intensity=0.6),
    "none": lambda i1, i2: dict(min_descriptor_sim=2.0),
}
M2_RATIO, M4_RATIO, M5_THRESHOLD = 0.8, 0.9, 0.8


def mlp_rows() -> np.ndarray:
    """(70, 384) rows that are not grid samples."""
    return synth._normal(np.random.Generator(np.random.PCG64(61)), (70, 384), 2.0)


def gather_tokens() -> np.ndarray:
    return synth.tokens(5, GATHER_GRID)


def gather_keypoints() -> np.ndarray:
    """(1, 66, 2) patch coordinates of one 8 x 8 frame: corners, fractional and out-of-range points; the second half repeats the
    first bit for bit (the selector's pad)."""
    rng = np.random.Generator(np.random.PCG64(62))
    kq = (rng.random((GATHER_K // 2, 2)) * (GATHER_GRID + 1.0) - 1.0).astype(np.float32)
    g = GATHER_GRID - 1
    kq[:6] = np.array([[0, 0], [g, g], [g, 0], [0, g], [g - 0.5, g], [-0.25, 3]], np.float32)
    return np.concatenate([kq, kq])[None]
