"""Planted inputs of sslx_subcell_keypoints for tests/test_gpu_subcell.py (and, without a GPU, tests/test_subcell_cpu.py): every
edge and corner cell, plateaus, one-sided ties, non-maxima and the pad arm's repeats, NaN and infinities as centre and as
neighbour, idx outside the grid, denormal differences.  check_decisions() holds each case to what it says of itself: a case that
is not listed as an exact tie decides nowhere within rounding of a threshold.  No torch, no GPU.
"""
import numpy as np

import subcell_ref as ref

F = np.float32
DMIN = np.float32(1.401298464324817e-45)        # the smallest fp32 denormal


def _all_cells(n, g):
    return np.tile(np.arange(g * g, dtype=np.int32), (n, 1))


def cases():
    """-> list of dict(name, sal (n, G, G) fp32, idx (n, K) int32, ties: bool, finite: bool).  ties: the case holds exact ties on
    purpose (a == 0, b == 0, den == 0 or |off| == 0.5 somewhere); finite: every value of sal is finite."""
    rng = np.random.default_rng(20260)
    out = []

    def add(name, sal, idx, ties=False, finite=True):
        out.append(dict(name=name, sal=np.ascontiguousarray(sal, F), idx=np.ascontiguousarray(idx, np.int32), ties=ties, finite=finite))

    # every edge and every corner cell, and every interior one, of a field without ties
    add("edges_and_corners", rng.random((2, 5, 5), dtype=F), _all_cells(2, 5))
    add("bump_every_cell", np.stack([ref.bump_field(5, 2.3, 1.7, 1.0), ref.bump_field(5, 1.2, 3.4, 1.0)]), _all_cells(2, 5))
    # plateaus: den == 0 on both axes, everywhere
    add("plateau", np.full((1, 4, 4), 0.25, F), _all_cells(1, 4), ties=True)
    # one-sided ties: a ridge two cells wide, so that the cell equals one neighbour and exceeds the other: off = -0.5 / +0.5 exactly
    ridge = np.full((1, 6, 6), 0.125, F)
    ridge[0, 2:4, :] = 0.75          # rows 2 and 3 equal: y ties;  x is a plateau along the ridge
    ridge[0, :, 2:4] += F(0.0625)    # columns 2 and 3 raised alike: x ties too, at the crossing both
    add("one_sided_ties", ridge, _all_cells(1, 6), ties=True)
    # non-maxima, and the pad arm's repeats: K above the number of cells, the same cells over and over (a saddle and slopes among them)
    slope = (np.arange(9, dtype=F).reshape(1, 3, 3) * F(0.1)).astype(F)
    add("pad_repeats", slope, np.array([[4] * 7 + [8] * 7 + [0, 4, 4, 5, 3, 4]], np.int32))
    saddle = np.array([[[0.1, 0.9, 0.2], [0.3, 0.5, 0.25], [0.15, 0.8, 0.05]]], F)       # a maximum along x, a minimum along y
    add("saddle", saddle, _all_cells(1, 3))
    # NaN, +inf, -inf as the centre (cell 12 of a 5 x 5 grid) and so as a neighbour of cells 7, 11, 13, 17; and huge finite values
    special = []
    for v in (np.nan, np.inf, -np.inf):
        f = ref.bump_field(5, 2.2, 1.9, 1.0)
        f[2, 2] = v
        special.append(f)
    both = ref.bump_field(5, 2.2, 1.9, 1.0)
    both[2, 1], both[2, 3] = np.inf, np.inf                     # both x neighbours infinite
    special.append(both)
    allinf = np.full((5, 5), np.inf, F)
    special.append(allinf)
    add("nan_and_inf", np.stack(special), np.tile(np.array([12, 7, 11, 13, 17, 6, 18], np.int32), (5, 1)), finite=False)
    huge = np.full((1, 3, 3), -3.0e38, F)
    huge[0, 1, 1] = 3.0e38                                       # c - m overflows to +inf: inf - inf = NaN, not refined
    add("overflow", huge, _all_cells(1, 3), finite=False)
    # idx outside [0, G*G): -1 and G*G, the int32 extremes, between valid cells
    g = 4
    add("idx_out_of_range", rng.random((2, g, g), dtype=F),
        np.array([[5, -1, g * g, 6, -2 ** 31, 2 ** 31 - 1, 9, g * g - 1], [-1, -1, 10, g * g + 1, 0, 5, 2 ** 30, 6]], np.int32))
    # denormal differences: all of them exact in fp32, none flushed
    den = np.zeros((3, 3, 3), F)
    den[0] = DMIN                                                # a field of denormals: c = 3, m = 1, p = 2 (x), m = p = 2 (y) times DMIN
    den[0, 1, 1], den[0, 1, 0], den[0, 1, 2], den[0, 0, 1], den[0, 2, 1] = 3 * DMIN, DMIN, 2 * DMIN, 2 * DMIN, 2 * DMIN
    tiny = F(2.0 ** -126)
    den[1] = tiny                                                # normals whose differences are denormal
    den[1, 1, 1], den[1, 1, 2], den[1, 0, 1] = tiny * F(1.5), tiny * F(1.25), tiny * F(1.25)
    den[2] = F(1.0) - F(2.0 ** -23)                              # differences of one and two ulp below 1.0
    den[2, 1, 1], den[2, 1, 0], den[2, 2, 1] = F(1.0), F(1.0) - F(2.0 ** -24), F(1.0) - F(2.0 ** -24)
    add("denormal_differences", den, np.tile(np.array([4, 4], np.int32), (3, 1)))
    # -0.0 beside +0.0: equal values, a plateau of mixed signs
    zeros = np.zeros((1, 3, 3), F)
    zeros[0, 1, 0], zeros[0, 0, 1] = F(-0.0), F(-0.0)
    add("signed_zeros", zeros, _all_cells(1, 3), ties=True)
    return out


def check_decisions(case):
    """A case whose `ties` is False decides nowhere within rounding of a threshold: per keypoint and per refinable axis, the exact
    (float64) a, b and den are non-zero, the exact |off| is below 0.5, and every test falls the same way in float64 as in fp32.
    A case listed as a tie must hold one.  Cases with non-finite values are not judged (their decisions are NaN tests)."""
    if not case["finite"]:
        return
    sal, idx = case["sal"], case["idx"]
    n, g = sal.shape[0], sal.shape[1]
    found_tie = False
    for f in range(n):
        for cell in idx[f]:
            if not 0 <= cell < g * g:
                continue
            y, x = divmod(int(cell), g)
            for lo, hi, border in (((y, x - 1), (y, x + 1), x in (0, g - 1)), ((y - 1, x), (y + 1, x), y in (0, g - 1))):
                if border:
                    continue
                c, m, p = sal[f, y, x], sal[f][lo], sal[f][hi]
                a64, b64 = float(c) - float(m), float(c) - float(p)          # exact: differences of fp32 values in float64
                a32, b32 = F(c - m), F(c - p)
                den64, den32 = a64 + b64, F(a32 + b32)
                assert (a64 >= 0, b64 >= 0) == (bool(a32 >= 0), bool(b32 >= 0)), (case["name"], f, cell)
                if a64 >= 0 and b64 >= 0:                  # den is only looked at for a maximum; it is 0 exactly when a = b = 0
                    assert (den64 > 0) == bool(den32 > 0), (case["name"], f, cell)
                tie = a64 == 0 or b64 == 0
                if not tie and a64 > 0 and b64 > 0:
                    off64 = (a64 - b64) / (2 * den64)
                    assert abs(off64) < 0.5, (case["name"], f, cell)
                found_tie |= tie
                assert case["ties"] or not tie, f"{case['name']}: frame {f} cell {cell} holds an exact tie the case does not list"
    assert found_tie == case["ties"], f"{case['name']}: listed as {'a tie' if case['ties'] else 'no tie'}"
