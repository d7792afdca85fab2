"""What tests/test_sim_sign_inputs.py (CPU) and tests/test_gpu_sim_signs.py share: descriptor sets on which NO similarity, or only
some, is positive.  sim_argmax_kernel zero-fills the candidate rows past the last one and masks them only in the last stage; query
lanes past the last query are multiplied by 0.  While every row and column of the similarity matrix has a positive maximum a slip
in any of these cannot show, because a zero never wins; here a zero would.

Sets (unit rows, width 128 or 256; u, w, w1, w2 are orthonormal axes, rows scatter around their centre by cone noise):
  all_negative   d1 around +u, d2 around -u: every similarity is near -0.9
  mixed          d1 around +u, every third row around +w; d2 around -(u + w) / sqrt 2, every fifth row - in a stage before the last
                 where there is one - around (u - w) / sqrt 2: the +w rows and the unflipped columns hold negative entries only,
                 the others have a positive winner
  last_stage     rows of the last stage of 64 of either set lean away from the axis: the best candidate of every row, and of
                 every column, lies in the last stage, and it is negative
  zero_rows      d2 negative on the first quarter of the coordinates, d1 positive there - except every other row, positive on
                 the last quarter instead: whole rows of the matrix are exactly +0.0f next to negative ones
  zero_cols      the same with the roles of d1 and d2 exchanged: whole columns are exactly +0.0f
"""
import numpy as np

from oracle import ora

WIDTHS = (128, 256)
SHAPES = ((1, 1), (1, 65), (65, 1), (33, 70), (64, 64), (65, 65), (129, 65), (130, 193))
KINDS = ("all_negative", "mixed", "last_stage", "zero_rows", "zero_cols")
STAGE = 64          # candidates per stage of sim_argmax_kernel (CB)
NOISE = 0.25


def last_stage_start(n: int) -> int:
    return STAGE * ((n - 1) // STAGE)


def _unit(x):
    return (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


def _cone(rng, centre, n, d):
    """n unit rows around the rows of `centre` ((d,) or (n, d))."""
    return _unit(np.broadcast_to(centre, (n, d)) + NOISE * rng.standard_normal((n, d)) / np.sqrt(d))


def _block_rows(rng, n, d, lo, hi, sign):
    x = np.zeros((n, d), np.float32)                # +0.0 outside the block
    x[:, lo:hi] = sign * (0.5 + rng.random((n, hi - lo)))
    return _unit(x)


def descriptor_set(kind: str, n1: int, n2: int, d: int, seed: int = 0):
    """(d1 (n1, d), d2 (n2, d)) fp32, unit rows."""
    rng = np.random.Generator(np.random.PCG64([9200, KINDS.index(kind), n1, n2, d, seed]))
    axes = np.linalg.qr(rng.standard_normal((d, 4)))[0].T            # four orthonormal axes
    u, w, w1, w2 = axes
    if kind == "all_negative":
        return _cone(rng, u, n1, d), _cone(rng, -u, n2, d)
    if kind == "mixed":
        c1 = np.where((np.arange(n1) % 3 == 2)[:, None], w, u)
        flip = (np.arange(n2) % 5 == 1) & (np.arange(n2) < max(last_stage_start(n2), 2))
        c2 = np.where(flip[:, None], (u - w) / np.sqrt(2), -(u + w) / np.sqrt(2))
        return _cone(rng, c1, n1, d), _cone(rng, c2, n2, d)
    if kind == "last_stage":
        c1 = np.where((np.arange(n1) >= last_stage_start(n1))[:, None], 0.6 * u + 0.8 * w1, u)
        c2 = np.where((np.arange(n2) >= last_stage_start(n2))[:, None], -0.6 * u + 0.8 * w2, -u)
        return _cone(rng, c1, n1, d), _cone(rng, c2, n2, d)
    q = d // 4
    if kind == "zero_rows":
        d1 = _block_rows(rng, n1, d, 0, q, 1.0)
        odd = np.arange(n1) % 2 == 1
        d1[odd] = _block_rows(rng, int(odd.sum()), d, d - q, d, 1.0)
        return d1, _block_rows(rng, n2, d, 0, q, -1.0)
    assert kind == "zero_cols"
    d2 = _block_rows(rng, n2, d, 0, q, -1.0)
    odd = np.arange(n2) % 2 == 1
    d2[odd] = _block_rows(rng, int(odd.sum()), d, d - q, d, -1.0)
    return _block_rows(rng, n1, d, 0, q, 1.0), d2


def batch(n1: int, n2: int, d: int, n_pairs: int):
    """n_pairs sets of one shape, the kinds in turn: (D1 (n_pairs, n1, d), D2 (n_pairs, n2, d), kinds)."""
    kinds = [KINDS[p % len(KINDS)] for p in range(n_pairs)]
    sets = [descriptor_set(k, n1, n2, d, seed=p) for p, k in enumerate(kinds)]
    return np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]), kinds


_ORACLE = {}


def oracle(kind: str, n1: int, n2: int, d: int, seed: int = 0, swap: bool = False):
    """(nn12, s12, nn21, s21, second12) of one set by oracle/ora.py - computed once, shared, never written to.  The runner-up is
    the row's maximum with the winner removed (the path match_rules_cases.oracle_rule's matchers take): -inf where n2 == 1.
    swap: the set with d2 as the queries (a pair list may name the two frames in either order)."""
    key = (kind, n1, n2, d, seed, swap)
    if key not in _ORACLE:
        d1, d2 = descriptor_set(kind, n1, n2, d, seed)
        if swap:
            d1, d2 = d2, d1
        nn12, s12, nn21, s21 = ora.sim_argmax(d1, d2)
        S = ora.sim_matrix(d1, d2)
        S[np.arange(d1.shape[0]), nn12] = -np.inf
        out = (nn12, s12, nn21, s21, S.max(axis=1))
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------------ thresholds met exactly
N_EDGE = 70


def edge_pair():
    """The 70 x 70 pair of the threshold tests (synth.descriptor_pair: known correspondences, no duplicated rows) with its
    oracle arg-max arrays and the mutual rows."""
    import synth
    d1, d2, s1, s2, i1, i2 = synth.descriptor_pair(4100, N_EDGE, N_EDGE, 0)
    nn12, s12, nn21, s21 = ora.sim_argmax(d1, d2)
    mutual = np.flatnonzero(nn21[nn12] == np.arange(N_EDGE))
    return dict(d1=d1, d2=d2, s1=s1, s2=s2, i1=i1, i2=i2, nn12=nn12, s12=s12, nn21=nn21, mutual=mutual)


def three_positions(v) -> tuple:
    """(one ulp below, v, one ulp above) in fp32."""
    v = np.float32(v)
    return np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))


def m1_thresholds(e: dict, i: int) -> dict:
    """The very fp32 values match_finalize_kernel compares row i against: condition -> threshold met exactly."""
    j = int(e["nn12"][i])
    two = np.float32(2)
    return dict(sim=e["s12"][i], sal=np.float32(np.float32(e["s1"][i] + e["s2"][j]) / two),
                int=np.float32(np.float32(e["i1"][i] + e["i2"][j]) / two))


def m4_quotient(e: dict, i: int) -> np.float32:
    """fl(second / fl(best + 1e-8f)) of row i: the rounded quotient sslam_match_finalize_rule compares under M4."""
    row = ora.sim_matrix(e["d1"][i:i + 1], e["d2"])[0]
    row[e["nn12"][i]] = -np.inf
    return np.float32(np.float32(row.max()) / np.float32(e["s12"][i] + np.float32(1e-8)))


def edge_rows(e: dict) -> list:
    """The first, the middle and the last mutual row."""
    return [int(i) for i in e["mutual"][[0, len(e["mutual"]) // 2, -1]]]


WIDE_OPEN = dict(sal=-1.0, sim=-2.0, int=-1.0)      # thresholds no row of edge_pair() fails
