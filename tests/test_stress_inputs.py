"""The stress inputs of tests/stress_cases.py and the CPU oracle on them, proved before any GPU is involved (no GPU needed):
the canonical sigmoid over its whole range against float64, the pass-through and steep selectors, the refiner at every depth
and in every arm of its two square roots against a float64 restatement (itself checked against the reference's own modules
through tests/golden/trained_ranges.npz), and BatchNorm on constant / ill-conditioned / tiny channels against float64.
tests/test_gpu_trained_ranges.py then holds the HIP kernels to the oracle bit for bit on the same inputs."""
import os

import numpy as np
import pytest

import stress_cases as sc
import synth
from oracle import ora

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_ranges.npz")
F32_MAX = float(np.finfo(np.float32).max)
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)          # 2^-126


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture
def report(capsys):
    """Print a measured figure past pytest's capture, so that a plain `pytest -q` run shows it."""
    def _print(*a):
        with capsys.disabled():
            print("\n   ", *a, end="")
    return _print


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ora_sigmoid(x):
    return np.array([ora.sigmoid(v) for v in np.asarray(x, np.float32).ravel()], np.float32)


# ------------------------------------------------------------------------------------------------------- sigmoid
def test_logit_list_holds_its_fixed_points():
    l = sc.logit_list(98, 0)
    assert l.dtype == np.float32 and l.shape == (98,) and np.isfinite(l).all() and np.abs(l).max() <= 110.0
    for v in sc.logit_fixed_points():
        assert (bits(l) == bits(np.float32(v))).any(), v                # +0 and -0 both, by bit pattern
    for v in (87.0, 88.0):
        for s in (1, -1):
            assert np.float32(s * v) in l and np.nextafter(np.float32(s * v), np.float32(0)) in l
            assert np.nextafter(np.float32(s * v), np.float32(s * np.inf)) in l
    for n in sc.TIE_N:                                                      # one float on each side of (n + 1/2) ln 2
        t = (n + 0.5) * sc.LN2
        near = l[np.abs(l.astype(np.float64) - t) <= abs(np.spacing(np.float32(t)))]
        assert (near.astype(np.float64) < t).any() and (near.astype(np.float64) > t).any(), n
    assert not np.array_equal(sc.logit_list(784, 1)[:98], l)


def test_sigmoid_against_float64(report):
    """ora.sigmoid within 4 ulp of 1/(1 + exp(-x)) evaluated in float64 and rounded to fp32, on 200 001 evenly spaced logits
    in [-87, 87] and on logit_list (measured: 2.22 ulp at x = -16.654; the margin is because the grid is not exhaustive).
    Beyond the clamp the oracle is a constant by contract: exactly 1.0f from 88 up, and from -88 down ONE positive number
    below 2^-126, ora.sigmoid(-88) - those entries of logit_list are held by the exact statements, not by the ulp bar."""
    x = np.concatenate([np.linspace(-87.0, 87.0, 200_001).astype(np.float32), sc.logit_list(784, 0), sc.logit_list(98, 1)])
    got = ora_sigmoid(x)
    x64 = x.astype(np.float64)
    want = (1.0 / (1.0 + np.exp(-x64))).astype(np.float32)
    ulp = np.spacing(want).astype(np.float64)                  # of the rounded float64 value (2^-149 where it is subnormal or 0)
    err = np.abs(got.astype(np.float64) - 1.0 / (1.0 + np.exp(-x64))) / ulp
    inside = x > -88.0
    worst = int(np.argmax(np.where(inside, err, 0)))
    report(f"sigmoid: max error {err[worst]:.2f} ulp at x = {x[worst]:.3f} over {int(inside.sum())} logits")
    assert err[inside].max() <= 4.0
    assert np.isfinite(got).all() and (got > 0).all() and (got <= 1).all()
    floor = ora.sigmoid(-88.0)
    assert 0.0 < float(floor) < F32_MIN_NORMAL                                # a subnormal
    report(f"sigmoid: floor {float(floor):.4e} (bits 0x{int(bits(floor)[0]):08x})")
    assert (x <= -88.0).sum() > 20 and (x >= 88.0).sum() > 20
    assert (bits(got[x <= -88.0]) == bits(floor)).all()
    assert (bits(got[x >= 88.0]) == bits(np.float32(1.0))).all()
    for v in (-88.0, -89.0, -103.97, -110.0, -1e30):
        assert bits(ora.sigmoid(v)) == bits(floor)
    for v in (88.0, 89.0, 103.97, 110.0, 1e30):
        assert bits(ora.sigmoid(v)) == bits(np.float32(1.0))


@pytest.mark.parametrize("hidden", [256, 128])
def test_passthrough_selector_is_the_sigmoid(hidden):
    l = sc.logit_list(98, 0)
    sal = ora.selector_saliency(sc.passthrough_feat(l, 7, 2), sc.passthrough_selector(hidden))
    assert np.array_equal(bits(sal).ravel(), bits(ora_sigmoid(l)))
    assert (sal == 1.0).sum() >= 5 and ((sal > 0) & (sal < F32_MIN_NORMAL)).sum() >= 4      # the fixed points alone


@pytest.mark.parametrize("scale", [60, 200])
def test_steep_selector_against_reference(gold, scale, report):
    """The oracle's saturated map against the reference's float64 map: at most 2 x the error the reference's own fp32 map has
    against it (the factor covers a different summation order).  Measured, oracle then torch fp32: scale 60, 1.54e-5 against
    1.62e-5; scale 200, 3.48e-5 against 3.60e-5."""
    feat = ora.bn_tokens(synth.tokens(48, 28, 2))[0].reshape(2, 28, 28, 384)
    sal = ora.selector_saliency(feat, sc.steep_selector(0, 256, scale))
    f64, f32 = gold[f"steep{scale}_f64"], gold[f"steep{scale}_f32"]
    e_ora = float(np.abs(sal.astype(np.float64) - f64).max())
    e_ref = float(np.abs(f32.astype(np.float64) - f64).max())
    report(f"steep selector x{scale}: oracle {e_ora:.3e}, torch fp32 {e_ref:.3e} against float64; "
           f"{(sal == 1.0).mean():.0%} of the cells exactly 1.0f, {(sal < 0.05).mean():.0%} below 0.05")
    assert e_ora <= 2.0 * e_ref
    if scale == 200:
        assert (sal == 1.0).mean() > 0.2 and (sal < 0.05).mean() > 0.4        # what the map is for: plateaus at 1.0f
        _, _, idx, st = ora.select_keypoints(sal, 500)
        assert not st.any() and all(np.unique(i).size < 500 for i in idx)     # the pad repeats cells


# ------------------------------------------------------------------------------------------------------- refiner
def refine64(x, sd):
    """float64 restatement of the refiner (descriptor_refiner.py: LayerNorm eps 1e-5, F.normalize eps 1e-12).  One fp32 trait
    is kept: a sum of squares beyond the fp32 maximum is +inf, as in the fp32 reference, so such a row normalises to 0."""
    p = {k: np.asarray(v, np.float64) for k, v in sd.items()}

    def ln(h, w, b):
        mu = h.mean(-1, keepdims=True)
        var = ((h - mu) ** 2).mean(-1, keepdims=True)
        return (h - mu) / np.sqrt(var + 1e-5) * w + b
    h = np.maximum(np.asarray(x, np.float64) @ p["input_proj.weight"].T + p["input_proj.bias"], 0.0)
    for i in range(sc.refiner_depth(sd)):
        q = f"residual_blocks.{i}."
        o = np.maximum(ln(h, p[q + "norm1.weight"], p[q + "norm1.bias"]) @ p[q + "fc1.weight"].T + p[q + "fc1.bias"], 0.0)
        o = ln(o, p[q + "norm2.weight"], p[q + "norm2.bias"]) @ p[q + "fc2.weight"].T + p[q + "fc2.bias"]
        h = np.maximum(o + h, 0.0)
    v = h @ p["output_proj.weight"].T + p["output_proj.bias"]
    ss = (v * v).sum(-1, keepdims=True)
    ss = np.where(ss > F32_MAX, np.inf, ss)
    return v / np.maximum(np.sqrt(ss), 1e-12)


def test_refiner_rows_are_what_they_say():
    x = sc.refiner_rows(70)
    assert np.array_equal(bits(x[1]), np.zeros(384, np.uint32)) and np.array_equal(bits(x[7]), np.full(384, 0x80000000, np.uint32))
    assert (np.abs(x[2]) < F32_MIN_NORMAL).all() and (x[2] != 0).sum() > 300
    assert (np.abs(x[8]) > F32_MIN_NORMAL).mean() > 0.9 and np.abs(x[8]).max() < 1e-34
    assert 1e12 < np.abs(x[3]).max() < 1e14 and 1e18 < np.abs(x[4]).max() < 1e20
    assert np.array_equal(bits(x[5]), bits(x[6]))
    big = sc.refiner_rows(257)
    assert np.array_equal(bits(big[:70]), bits(x)) and np.array_equal(bits(big[70:140]), bits(-x))
    assert np.array_equal(bits(big[140:210]), bits(x)) and np.array_equal(bits(sc.refiner_rows(33)), bits(x[:33]))


@pytest.mark.parametrize("depth", [0, 1, 3, 8])
def test_refiner_restatement_against_reference(gold, depth, report):
    """The float64 restatement equals the reference's module run as .double(); the reference's own fp32 run and the oracle
    both sit within the descriptor bar of it."""
    x = sc.refiner_rows(int(gold["rows"]))
    sd = synth.refiner_state(3, n_blocks=depth)
    want = refine64(x, sd)
    assert np.abs(want - gold[f"refine_d{depth}_f64"]).max() < 1e-11
    e_ref = float(np.abs(gold[f"refine_d{depth}_f32"] - want).max())
    e_ora = float(np.abs(ora.refine(x, sd, depth) - want).max())
    report(f"refiner depth {depth}: oracle {e_ora:.2e}, torch fp32 {e_ref:.2e} against float64")
    assert e_ora < 5e-6 and e_ref < 5e-6


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 8])
def test_refiner_oracle_on_every_arm(depth, report):
    """Bar 5e-6: the project's descriptor bar (test_descriptors_match_reference_golden).  Measured on the plain states: 1.8e-7
    at depth 0, 8.2e-7 at depth 8, no stress row above 4.4e-7."""
    x = sc.refiner_rows(70)
    ordinary = np.array([i for i in range(70) if i not in sc.HUGE_ROWS])
    stress = np.array([1, 2, 3, 4, 5, 6, 7, 8])
    for name, sd in sc.refiner_variants(depth).items():
        got = ora.refine(x, sd, depth)
        want = refine64(x, sd)
        assert np.isfinite(got).all(), name
        err = np.abs(got - want).max(axis=1)
        if name == "plain":
            report(f"refiner depth {depth}: max error {err.max():.2e} (stress rows {err[stress].max():.2e})")
        assert err.max() < 5e-6, (name, int(err.argmax()), float(err.max()))
        if name == "dead":                     # relu(input_proj) is all zero: one descriptor, whatever the row
            assert (bits(got[ordinary]) == bits(got[ordinary[0]])).all()
            assert not np.array_equal(bits(got[3]), bits(got[0]))
        elif name == "zero_out":
            assert not bits(got).any()
        elif name == "bias_1e-30":             # the sum of squares underflows to 0: the 1e-12 floor divides
            assert (bits(got) == bits(np.float32(1e-30) / np.float32(1e-12))).all() and abs(float(got[0, 0]) / 1e-18 - 1) < 1e-6
        elif name == "bias_1e-20":             # subnormal squares, sqrt(128) * 1e-20 is still below the floor: 1e-20 / 1e-12
            assert (bits(got) == bits(np.float32(1e-20) / np.float32(1e-12))).all() and abs(float(got[0, 0]) / 1e-8 - 1) < 1e-6
            assert abs(float(want[0, 0]) / 1e-8 - 1) < 1e-6
        elif name == "bias_3e19":              # the squares overflow: the norm is +inf and v / inf == 0
            assert not bits(got).any()


# ----------------------------------------------------------------------------------------------------- batch norm
def bn64(tok, n_prefix, group, gamma, beta, rmean, rvar, train, eps):
    x = tok[:, n_prefix:].astype(np.float64)
    n, cells, c = x.shape
    xg = x.reshape(n // group, group * cells, c)
    if train:
        mean, var = xg.mean(1, keepdims=True), xg.var(1, keepdims=True)
    else:
        mean, var = rmean.astype(np.float64), rvar.astype(np.float64)
    y = (xg - mean) / np.sqrt(var + np.float64(np.float32(eps))) * gamma.astype(np.float64) + beta.astype(np.float64)
    return y.reshape(n, cells, c)


@pytest.mark.parametrize("n_prefix", [0, 1, 5])
@pytest.mark.parametrize("train", [True, False])
def test_bn_oracle_on_altered_channels(train, n_prefix, report):
    """Channels 4 .. 383 within 5e-6 of float64 (measured 8.5e-7); every output finite; in train mode with the default affine
    the constant channel is exactly 0.  Channel 1 (1e4 + 1e-3 noise) is ill-conditioned in fp32 - its error is reported, not
    bounded here - and, like the other altered channels, is held by bits on the device."""
    tok = sc.bn_tokens_case(29 * 29, 2, n_prefix, seed=n_prefix)
    gamma, beta, rmean, rvar = sc.bn_affine(7)
    for group in (2, 1):
        y, _, _ = ora.bn_tokens(tok, n_prefix, group, gamma, beta, rmean, rvar, train, 1e-5)
        want = bn64(tok, n_prefix, group, gamma, beta, rmean, rvar, train, 1e-5)
        assert np.isfinite(y).all()
        err = np.abs(y - want).max(axis=(0, 1))
        if group == 2:
            report(f"bn {'train' if train else 'eval'} n_prefix {n_prefix}: channels 4.. {err[4:].max():.2e}, channel 1 {err[1]:.2e}")
        assert err[4:].max() < 5e-6, (group, int(err[4:].argmax()) + 4)
        if train:
            y0 = ora.bn_tokens(tok, n_prefix, group, train=True)[0]
            assert not bits(y0[..., 0]).any()
            if group == 1:
                assert not bits(y0[0, :, 3]).any() and np.abs(y0[1, :, 3]).max() > 1
