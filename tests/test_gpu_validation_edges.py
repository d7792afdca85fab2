"""GPU tests of the validation kernels (csrc/validate.hip) past what tests/test_gpu_validation.py runs: more than one column
segment of the Sobel / pool pass, both clamps of the logits, unequal sides, stride 0 and more than eight pairs in the row
log-sum-exp, the optional inputs and outputs, the smallest grids and descriptor counts, and hand-made arg-max arrays.  Inputs:
tests/val_edge_cases.py (their properties: tests/test_validation_edge_inputs.py); reference: tests/val_ref.py in float64.

The tolerance is the one rule of val_ref.tolerance with the scales test_gpu_validation.py names: max(|lse|, 1 / T) for a row's lse
and ce, 8 max |gray| for Sobel means and the maximum, the uncentred sums for A, E and Ss.  One tightening: in the FULLY CLAMPED
cases every logit is exactly +-50 in fp32 and in float64 alike, so the similarities' roundoff does not enter and the scale is
|lse| alone (for a sum over rows: the sum of their |lse|).  Exact assertions carry no tolerance."""
import numpy as np
import pytest

import synth
import val_edge_cases as vec
import val_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD      # a NaN's bits: no kernel result


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _same(T, a, b):
    """Same shape and the same bits (floats compared as integers: a NaN or a signed zero cannot hide a difference)."""
    if a.shape != b.shape:
        return False
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return T.equal(a.view(T.int32), b.view(T.int32)) if a.dtype.is_floating_point else T.equal(a, b)


def _dev(T, *arrays):
    return tuple(T.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _guarded(T, *shape):
    """A tensor of one more row in front and one behind than `shape`, filled with the sentinel; -> (whole, middle)."""
    whole = T.full((shape[0] + 2,) + tuple(shape[1:]), SENTINEL, dtype=T.int32, device="cuda").view(T.float32)
    return whole, whole[1:-1]


def _guards_untouched(T, whole):
    w = whole.view(T.int32)
    return bool((w[0] == SENTINEL).all()) and bool((w[-1] == SENTINEL).all())


# --------------------------------------------------------------------------------------------------- 1. Sobel / pool segments
_FRAME_REF = {}


def _frame_ref(kind, size, f):
    if (kind, size, f) not in _FRAME_REF:
        _FRAME_REF[kind, size, f] = val_ref.frame_stats(vec.saliency(size, 2)[f], vec.image(kind, size, f))
    return _FRAME_REF[kind, size, f]


def _gray_scale(img):
    c = img.astype(np.float64)
    return 8.0 * np.abs(0.299 * c[0] + 0.587 * c[1] + 0.114 * c[2]).max()      # Sobel weights times the largest pixel


def _check_frame(lib, what, ref, sal, img, P, M, S):
    """pooled, edge_max and every slot of a frame's statistics row against float64 under the rule."""
    slot = lib.VAL_FRAME_SLOTS
    gray = _gray_scale(img)
    err = np.abs(P - ref["pooled"])
    print(f"{what}: max |P - ref| {err.max():.3e} (tolerance {val_ref.tolerance(0.0, scale=gray):.3e}), m {M:.6e} ref {ref['edge_max']:.6e}")
    assert (err <= val_ref.tolerance(ref["pooled"], scale=gray)).all(), (what, float(err.max()), np.unravel_index(err.argmax(), err.shape))
    assert abs(M - ref["edge_max"]) <= val_ref.tolerance(ref["edge_max"], scale=gray), (what, M, ref["edge_max"])
    assert S[slot["edge_max"]] == M
    for key in ("sal_mean", "sal_var", "sal_max", "sal_dx", "sal_dy", "sal_high", "edge_mean"):
        assert abs(S[slot[key]] - ref[key]) <= val_ref.tolerance(ref[key]), (what, key, S[slot[key]], ref[key])
    s64, p64 = sal.astype(np.float64), ref["pooled"]
    uncentred = dict(edge_a=np.sqrt((p64 ** 2).sum() * (s64 ** 2).sum()), edge_e=(p64 ** 2).sum(), sal_ss=(s64 ** 2).sum())
    for key, scale in uncentred.items():      # centred sums: what a cancellation leaves of the uncentred ones
        assert abs(S[slot[key]] - ref[key]) <= val_ref.tolerance(ref[key], scale=scale), (what, key, S[slot[key]], ref[key])


@pytest.mark.parametrize("kind", vec.KINDS)
@pytest.mark.parametrize("size,n", vec.SIZES_FRAMES)
def test_sobel_pool_across_column_segments(T, size, n, kind):
    """One to three column segments a frame, the last 512, 32 or 16 pixels wide: block means, the frame maximum and every slot
    of the frame statistics (G = 32 .. 65, no descriptors) against float64; a launch per frame and a second run give the same
    bits.  `seams`: structure only around the segment starts; `peak_last`: the maximum in the last segment of frame 0 and in
    the first of frame 1."""
    from sslam_amd import lib
    img, sal = vec.images(kind, size, n), vec.saliency(size, n)
    d_img, d_sal = _dev(T, img, sal)
    pooled, emax = lib.edge_pool(d_img)
    stats, dmean, dm2 = lib.val_frame_stats(d_sal, pooled, emax)
    assert dmean is None and dm2 is None
    P, M, S = (t.cpu().numpy() for t in (pooled, emax, stats))
    for f in range(n):
        _check_frame(lib, f"S {size} {kind} frame {f} of {n}", _frame_ref(kind, size, f), sal[f], img[f], P[f], M[f], S[f])
    for f in range(n):
        p1, m1 = lib.edge_pool(d_img[f:f + 1])
        s1 = lib.val_frame_stats(d_sal[f:f + 1], p1, m1)[0]
        for name, x, y in (("pooled", p1, pooled), ("edge_max", m1, emax), ("stats", s1, stats)):
            assert _same(T, x[0], y[f]), f"{name} of frame {f}: a launch of its own gave other bits"
    p2, m2 = lib.edge_pool(d_img)
    s2 = lib.val_frame_stats(d_sal, p2, m2)[0]
    for name, x, y in (("pooled", p2, pooled), ("edge_max", m2, emax), ("stats", s2, stats)):
        assert _same(T, x, y), f"{name}: a second run gave other bits"


@pytest.mark.parametrize("size", vec.SIZES)
def test_block_mean_does_not_depend_on_the_cells_place(T, size):
    """A cell's block mean is a function of its 18 x 18 neighbourhood alone: the image moved by one cell to the right or to the
    left gives the same bits one cell further, on either side of every seam as in the interior of a segment; the last cell
    column (zero padding on its right) against the same pixels as the last column of a narrower image."""
    from sslam_amd import lib
    a, b, c = vec.shifted_images(size)
    pa, pb, pc = (lib.edge_pool(_dev(T, x[None])[0])[0][0] for x in (a, b, c))
    for_b, for_c = vec.shift_cells(size)
    gb, gc = (T.tensor(v, device="cuda") for v in (for_b, for_c))
    for name, got, want in (("right", pb[:, gb + 1], pa[:, gb]), ("left", pc[:, gc - 1], pa[:, gc])):
        diff = (got.view(T.int32) != want.view(T.int32)).nonzero().cpu().numpy()
        assert len(diff) == 0, f"S {size}: moved {name}, {len(diff)} cells differ, the first at (gy, index) {diff[0]}"
    cc = vec.crop_cells(size)
    if cc:
        col_a, col_crop, rows = cc
        crop = np.ascontiguousarray(a[:, :vec.CROP, -vec.CROP:])
        pcrop = lib.edge_pool(_dev(T, crop[None])[0])[0][0]
        assert _same(T, pcrop[:rows, col_crop], pa[:rows, col_a]), f"S {size}: the last cell column differs from the crop's"


# ------------------------------------------------------------------------------------------------------ 2. row log-sum-exp
_PAIR_REF = {}


def _pair_ref(key, d1, d2, temperature):
    """(lse, logits) in float64, once per named pair."""
    if key not in _PAIR_REF:
        _PAIR_REF[key] = (val_ref.row_lse(d1, d2, temperature), val_ref.logits(d1, d2, temperature))
    return _PAIR_REF[key]


def _check_pair(lib, where, ref, x, temperature, lse, ce, _s00, nn12, nn21, pstats, cnt, clamped=False):
    """One pair's device arrays (numpy) against float64: every row's lse and ce, and the pair sums over the DEVICE's own mutual
    rows.  clamped: the fully clamped cases, scale |lse| (module docstring)."""
    n1, n2 = x.shape
    scale = np.abs(ref) if clamped else np.maximum(np.abs(ref), 1.0 / temperature)
    tol = val_ref.tolerance(ref, scale=scale)
    err = np.abs(lse - ref)
    cref = ref - x.max(axis=1)
    cerr = np.abs(ce - cref)
    print(f"{where} ({n1} x {n2}) T {temperature}: max |lse - ref| {err.max():.3e} (tolerance there {tol[err.argmax()]:.3e}), "
          f"max |ce - ref| {cerr.max():.3e}")
    assert (err <= tol).all(), (where, int(err.argmax()), float(err.max()))
    assert (cerr <= val_ref.tolerance(cref, scale=scale)).all(), (where, int(cerr.argmax()), float(cerr.max()))
    assert ((nn12 >= 0) & (nn12 < n2)).all() and ((nn21 >= 0) & (nn21 < n1)).all()
    mask = val_ref.mutual_rows(nn12, nn21)
    assert mask.any(), "the global maximum is mutual"
    assert cnt == mask.sum() and pstats[lib.VAL_PAIR_SLOTS["matches"]] == mask.sum(), (where, cnt, mask.sum())
    i = np.arange(n1)
    want = float(np.sum(ref[mask] - x[i[mask], nn12[mask]]))
    rows = float(np.abs(ref[mask]).sum()) if clamped else mask.sum() / temperature      # a sum of that many rows
    assert abs(pstats[lib.VAL_PAIR_SLOTS["ce_sum"]] - want) <= val_ref.tolerance(want, scale=max(abs(want), rows)), (where, want)
    pad = float(ref[0] - x[0, 0])
    pscale = max(abs(pad), abs(float(ref[0])) if clamped else 1.0 / temperature)
    assert abs(pstats[lib.VAL_PAIR_SLOTS["pad_ce"]] - pad) <= val_ref.tolerance(pad, scale=pscale), (where, pad)


def _sal(T, n, seed=3):
    return _dev(T, np.random.default_rng(seed).uniform(0, 1, (n, 3, 3)).astype(np.float32))[0]


def _strided(T, lib, d1, stride1, n1, d2, stride2, n2, n_pairs, temperature, sal1, sal2, out=None, rows_only=False):
    """The arg-max launch, the row log-sum-exp on its maxima and the pair statistics -> (lse, ce, s00, nn12, nn21, pstats, cnt)."""
    nn12, s12, nn21, _, _ = lib.sim_argmax(d1, stride1, n1, d2, stride2, n2, n_pairs)
    if rows_only:
        r12, s12r, _ = lib.sim_argmax_rows(d1, stride1, n1, d2, stride2, n2, n_pairs)
        assert _same(T, r12, nn12) and _same(T, s12r, s12)
        s12 = s12r
    if out is None:      # sentinel-filled, so that a row no workgroup wrote cannot hold an earlier result by chance
        out = (_guarded(T, n_pairs, n1)[1], _guarded(T, n_pairs, n1)[1], _guarded(T, n_pairs)[1])
    lse, ce, s00 = lib.row_lse(d1, stride1, n1, d2, stride2, n2, n_pairs, s12, temperature, out=out)
    ps, cnt = lib.val_pair_stats(sal1, sal2, nn12, nn21, s12, ce, s00, temperature)
    return lse, ce, s00, nn12, nn21, ps, cnt


NAMES = ("lse", "ce", "s00", "nn12", "nn21", "pair stats", "n_matches")


def _one_pair(T, lib, key, first, second, temperature, clamped=False):
    """first (n1, 128) against second (n2, 128) as a launch of one pair, checked against float64; -> the device tuple."""
    n1, n2 = len(first), len(second)
    d1, d2 = _dev(T, first[None], second[None])
    sal = _sal(T, 2)
    got = _strided(T, lib, d1, n1 * lib.D_OUT, n1, d2, n2 * lib.D_OUT, n2, 1, temperature, sal[:1], sal[1:])
    ref, x = _pair_ref(key, first, second, temperature)
    _check_pair(lib, str(key), ref, x, temperature, *(t[0].cpu().numpy() for t in got), clamped=clamped)
    s00 = float(got[2][0])
    assert abs(s00 - val_ref.sims(first[:1], second[:1])[0, 0]) <= val_ref.tolerance(0.0), "s00 is the similarity of rows 0 and 0"
    again = _strided(T, lib, d1, n1 * lib.D_OUT, n1, d2, n2 * lib.D_OUT, n2, 1, temperature, sal[:1], sal[1:])
    for name, a, b in zip(NAMES, got, again):
        assert _same(T, a, b), f"{name}: a second run gave other bits"
    return got


@pytest.mark.parametrize("name", vec.CLAMPED)
def test_row_lse_fully_clamped(T, name):
    """T = 0.01, 129 rows against 65, every logit exactly +50 or -50: all on the upper arm, all on the lower arm (the row
    maximum itself clamped, every term exp(0)), a seeded interleaving of 30 and 35, one high among 64 low.  The reference is
    the closed form; the scale of the tolerance is |lse|."""
    from sslam_amd import lib
    first, second, n_high = vec.clamped_case(name)
    lse, ce = (t[0].cpu().numpy() for t in _one_pair(T, lib, ("clamped", name), first, second, vec.CLAMP_T, clamped=True)[:2])
    closed = vec.clamped_lse(n_high)
    err = np.abs(lse - closed).max()
    print(f"{name}: closed form {closed:.9f}, device {lse[0]:.9f}, max error {err:.3e}, tolerance {val_ref.tolerance(closed, scale=abs(closed)):.3e}")
    assert err <= val_ref.tolerance(closed, scale=abs(closed))
    assert len(np.unique(lse.view(np.uint32))) == 1 and len(np.unique(ce.view(np.uint32))) == 1, "every row sums the same terms"


def test_row_lse_partly_clamped(T):
    """Raw logits below -50, above 50 and in between in the same rows, both directions of the pair."""
    from sslam_amd import lib
    bank = vec.partly_clamped()
    for a, b in ((0, 1), (1, 0)):
        _one_pair(T, lib, ("partly", a, b), bank[a], bank[b], vec.CLAMP_T)


@pytest.mark.parametrize("temperature", [1e3, 1.0])
def test_row_lse_temperatures(T, temperature):
    """T = 1000: every logit near 0, lse near log 65; T = 1: the similarities themselves."""
    from sslam_amd import lib
    bank = vec.unrelated_bank(65)
    _one_pair(T, lib, ("unrelated", temperature), bank[0], bank[1], temperature)


@pytest.mark.parametrize("n1,n2", vec.SHAPES)
def test_row_lse_unequal_sides(T, n1, n2):
    """n1 != n2, two pairs a launch (the pair offsets p n1 and p n2 differ).  At (129, 37) also: the row maxima of
    sim_argmax_rows give the same bits, and outputs taken from the middle of larger tensors leave a sentinel row in front and
    one behind untouched (the second query block has 127 lanes without a query)."""
    from sslam_amd import lib
    temperature = 0.1
    first, second = vec.rect_pair(n1, n2)
    d1, d2 = _dev(T, first, second)
    sal = _sal(T, 4)
    args = (d1, n1 * lib.D_OUT, n1, d2, n2 * lib.D_OUT, n2, 2, temperature, sal[:2], sal[2:])
    got = _strided(T, lib, *args)
    for p in range(2):
        ref, x = _pair_ref(("rect", n1, n2, p), first[p], second[p], temperature)
        _check_pair(lib, f"rect pair {p}", ref, x, temperature, *(t[p].cpu().numpy() for t in got))
        alone = _strided(T, lib, d1[p:p + 1], n1 * lib.D_OUT, n1, d2[p:p + 1], n2 * lib.D_OUT, n2, 1, temperature, sal[p:p + 1], sal[2 + p:3 + p])
        for name, a, b in zip(NAMES, got, alone):
            assert _same(T, a[p], b[0]), f"{name} of pair {p}: a launch of its own gave other bits"
    if (n1, n2) == (129, 37):
        whole = [_guarded(T, 2, n1), _guarded(T, 2, n1), _guarded(T, 2)]
        rows = _strided(T, lib, *args, out=tuple(m for _, m in whole), rows_only=True)
        for name, a, b in zip(NAMES, got, rows):
            assert _same(T, a, b), f"{name}: other bits from the maxima of sim_argmax_rows, written into the middle of a larger tensor"
        for name, (w, _) in zip(NAMES, whole):
            assert _guards_untouched(T, w), f"{name}: a guard row was written"


_ROUNDS = {}


def _rounds(T):
    if not _ROUNDS:
        bank = vec.rounds_bank()
        _ROUNDS.update(bank=bank, dev=_dev(T, bank)[0], sal=_sal(T, vec.ROUNDS_FRAMES, seed=9), alone={})
    return _ROUNDS


def _alone(T, lib, a, b, temperature):
    """Frames (a, b) of the rounds bank as a launch of that pair alone, checked against float64 once."""
    r = _rounds(T)
    if (a, b) not in r["alone"]:
        k, dev, sal = vec.ROUNDS_K, r["dev"], r["sal"]
        got = _strided(T, lib, dev[a:a + 1], k * lib.D_OUT, k, dev[b:b + 1], k * lib.D_OUT, k, 1, temperature, sal[a:a + 1], sal[b:b + 1])
        ref, x = _pair_ref(("rounds", a, b), r["bank"][a], r["bank"][b], temperature)
        _check_pair(lib, f"rounds ({a}, {b})", ref, x, temperature, *(t[0].cpu().numpy() for t in got))
        r["alone"][a, b] = got
    return r["alone"][a, b]


def _same_as_alone(T, lib, got, pairs, temperature, where):
    for p, (a, b) in enumerate(pairs):
        for name, x, y in zip(NAMES, got, _alone(T, lib, a, b, temperature)):
            assert _same(T, x[p], y[0]), f"{where}: {name} of pair {p} = frames ({a}, {b}) differs from a launch of that pair alone"


@pytest.mark.parametrize("n_pairs", [9, 17])
def test_row_lse_more_than_eight_pairs_strided(T, n_pairs):
    """9 and 17 consecutive pairs of 129 rows: pair = (slot / qblocks) * 8 + xcd goes into a second and a third round of eight,
    two query blocks a pair, and the surplus workgroups of the last round return.  Every pair has the bits of a launch of that
    pair alone (each checked against float64).  At 9 pairs the outputs lie between sentinel rows."""
    from sslam_amd import lib
    r, k, temperature = _rounds(T), vec.ROUNDS_K, 0.1
    dev, sal, stride = r["dev"], r["sal"], vec.ROUNDS_K * lib.D_OUT
    whole = [_guarded(T, n_pairs, k), _guarded(T, n_pairs, k), _guarded(T, n_pairs)] if n_pairs == 9 else None
    got = _strided(T, lib, dev[:n_pairs], stride, k, dev[1:n_pairs + 1], stride, k, n_pairs, temperature, sal[:n_pairs], sal[1:n_pairs + 1],
                   out=tuple(m for _, m in whole) if whole else None)
    _same_as_alone(T, lib, got, [(p, p + 1) for p in range(n_pairs)], temperature, f"{n_pairs} strided pairs")
    if whole:
        for name, (w, _) in zip(NAMES, whole):
            assert _guards_untouched(T, w), f"{name}: a guard row was written"


def test_row_lse_stride_zero(T):
    """stride1 = 0: frame 0 against frames 1 .. 9 in one launch of 9 pairs."""
    from sslam_amd import lib
    r, k, temperature = _rounds(T), vec.ROUNDS_K, 0.1
    dev, sal, stride = r["dev"], r["sal"], vec.ROUNDS_K * lib.D_OUT
    got = _strided(T, lib, dev[:1], 0, k, dev[1:10], stride, k, 9, temperature, sal[:1].repeat(9, 1, 1), sal[1:10])
    _same_as_alone(T, lib, got, [(0, b) for b in range(1, 10)], temperature, "stride 0")


def test_row_lse_more_than_eight_pairs_listed(T):
    """17 listed pairs with two absent pairs (zero rows, count 0), two self pairs and a repeated pair."""
    from sslam_amd import lib
    r, temperature = _rounds(T), 0.1
    first, second = vec.ROUNDS_LISTED
    f, s = (T.tensor(v, dtype=T.int32, device="cuda") for v in (first, second))
    nn12, s12, nn21, _, _ = lib.sim_argmax_pairs(r["dev"], f, s)
    lse, ce, s00 = lib.row_lse_pairs(r["dev"], f, s, s12, temperature)
    ps, cnt = lib.val_pair_stats_pairs(r["sal"], f, s, nn12, nn21, s12, ce, s00, temperature)
    got = (lse, ce, s00, nn12, nn21, ps, cnt)
    present = [p for p, (a, b) in enumerate(zip(first, second)) if 0 <= a < vec.ROUNDS_FRAMES and 0 <= b < vec.ROUNDS_FRAMES]
    assert len(present) == 15
    _same_as_alone(T, lib, [t[present] for t in got], [(first[p], second[p]) for p in present], temperature, "17 listed pairs")
    for p in sorted(set(range(17)) - set(present)):
        for name, t in zip(("lse", "ce", "s00", "pair stats", "n_matches"), (lse, ce, s00, ps, cnt)):
            assert not t[p].reshape(-1).view(T.int32).any(), f"absent pair {p}: {name} is not all +0"
    assert _same(T, lse[0], lse[12]) and _same(T, ps[0], ps[12]), "the repeated pair"


def test_row_lse_null_outputs(T):
    """lse only, ce only, both without s00: what is written has the bits of the full call, what is not asked for is not written
    (the listed form too); neither lse nor ce is an invalid argument."""
    from sslam_amd import lib
    n1, n2, temperature = 129, 37, 0.1
    first, second = vec.rect_pair(n1, n2)
    d1, d2 = _dev(T, first, second)
    args = (d1, n1 * lib.D_OUT, n1, d2, n2 * lib.D_OUT, n2, 2)
    s12 = lib.sim_argmax(*args)[1]
    full = lib.row_lse(*args, s12, temperature)

    def fresh():
        return T.empty((2, n1), device="cuda"), T.empty((2, n1), device="cuda"), T.empty((2,), device="cuda")

    for keep in ((True, False, True), (False, True, True), (True, True, False), (True, False, False), (False, True, False)):
        out = tuple(t if k else None for t, k in zip(fresh(), keep))
        got = lib.row_lse(*args, s12, temperature, out=out)
        for name, k, g, o, want in zip(NAMES, keep, got, out, full):
            assert (g is o) if k else (g is None), name
            assert not k or _same(T, g, want), f"{name} with outputs {keep}: other bits than the full call"
    with pytest.raises(ValueError):
        lib.row_lse(*args, s12, temperature, out=(None, None, fresh()[2]))
    # the listed form on a bank of the same frames (K = 129 both sides)
    r = _rounds(T)
    f, s = (T.tensor(v, dtype=T.int32, device="cuda") for v in ([0, 3, -1], [1, 3, 2]))
    s12 = lib.sim_argmax_pairs(r["dev"], f, s)[1]
    full = lib.row_lse_pairs(r["dev"], f, s, s12, temperature)
    for keep in ((True, False, False), (False, True, True)):
        out = tuple(T.empty_like(t) if k else None for t, k in zip(full, keep))
        got = lib.row_lse_pairs(r["dev"], f, s, s12, temperature, out=out)
        for name, k, g, want in zip(NAMES, keep, got, full):
            assert (g is None) if not k else _same(T, g, want), f"listed, {name} with outputs {keep}"
    with pytest.raises(ValueError):
        lib.row_lse_pairs(r["dev"], f, s, s12, temperature, out=(None, None, None))


# ----------------------------------------------------------------------------------------------------- 3. frame statistics
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("cell", [0.37, 0.7])
def test_frame_stats_of_a_single_cell(T, cell):
    """G = 1 (a 16 x 16 image): no neighbour, nothing to centre - dx = dy = 0, var = ss = A = E = +0, means = the cells."""
    from sslam_amd import lib
    img = vec.image("random", 16, 0)
    sal = np.full((1, 1, 1), cell, np.float32)
    d_img, d_sal = _dev(T, img[None], sal)
    pooled, emax = lib.edge_pool(d_img)
    S = lib.val_frame_stats(d_sal, pooled, emax)[0][0].cpu().numpy()
    slot = lib.VAL_FRAME_SLOTS
    _check_frame(lib, "G 1", val_ref.frame_stats(sal[0], img), sal[0], img, pooled[0].cpu().numpy(), float(emax[0]), S)
    for key in ("sal_var", "sal_dx", "sal_dy", "sal_ss", "edge_a", "edge_e"):
        assert _bits(S[slot[key]]) == 0, key
    assert _bits(S[slot["sal_mean"]]) == _bits(cell) and _bits(S[slot["sal_max"]]) == _bits(cell)
    assert S[slot["sal_high"]] == (1.0 if np.float32(cell) > vec.HIGH else 0.0)
    assert _bits(S[slot["edge_mean"]]) == _bits(pooled.cpu().numpy()[0, 0, 0])


def test_frame_stats_of_four_cells(T):
    from sslam_amd import lib
    img = vec.images("random", 32, 2)
    sal = np.random.default_rng(2).uniform(0.02, 0.98, (2, 2, 2)).astype(np.float32)
    d_img, d_sal = _dev(T, img, sal)
    pooled, emax = lib.edge_pool(d_img)
    S = lib.val_frame_stats(d_sal, pooled, emax)[0].cpu().numpy()
    for f in range(2):
        _check_frame(lib, f"G 2 frame {f}", val_ref.frame_stats(sal[f], img[f]), sal[f], img[f], pooled[f].cpu().numpy(), float(emax[f]), S[f])


def test_frame_stats_threshold_and_optional_edge_inputs(T):
    """G = 5 with 0.6f in four cells and its two neighbouring floats in two more: the count is of cells ABOVE 0.6f.  Without
    pooled / edge_max the four EDGE slots are +0 and every saliency slot has the bits of the call that had them."""
    from sslam_amd import lib
    sal = np.stack([vec.threshold_map(), np.random.default_rng(8).uniform(0, 1, (5, 5)).astype(np.float32)])
    img = vec.images("random", 80, 2)
    d_img, d_sal = _dev(T, img, sal)
    pooled, emax = lib.edge_pool(d_img)
    with_edges = lib.val_frame_stats(d_sal, pooled, emax)[0]
    without = lib.val_frame_stats(d_sal)[0]
    S, S0 = with_edges.cpu().numpy(), without.cpu().numpy()
    slot = lib.VAL_FRAME_SLOTS
    for f in range(2):
        _check_frame(lib, f"G 5 frame {f}", val_ref.frame_stats(sal[f], img[f]), sal[f], img[f], pooled[f].cpu().numpy(), float(emax[f]), S[f])
        assert S[f, slot["sal_high"]] == S0[f, slot["sal_high"]] == (sal[f] > np.float32(0.6)).sum()
    assert (sal[0] > np.float32(0.6)).sum() + 4 == (sal[0] >= np.float32(0.6)).sum()
    for key, i in slot.items():
        if key.startswith("edge_"):
            assert not _bits(S0[:, i]).any(), f"{key} without the edge inputs is not +0"
            assert _bits(S[:, i]).all(), f"{key} with the edge inputs"
        else:
            assert np.array_equal(_bits(S0[:, i]), _bits(S[:, i])), f"{key} depends on the edge inputs"
    assert not _bits(S0[:, len(slot):]).any() and not _bits(S[:, len(slot):]).any(), "the unused slots are +0"


@pytest.mark.parametrize("k", [1, 2, 37])
def test_frame_stats_descriptor_moments(T, k):
    """K = 1: the mean is the row and M2 is +0 (row parity 1 has no row); K = 2: one row per parity; K = 37: the statistics
    row is the same bits with and without descriptors."""
    from sslam_amd import lib
    desc = np.stack([synth.unit_descriptors(900 + 10 * k + f, k, 128, 0) for f in range(2)])
    sal = np.random.default_rng(k).uniform(0, 1, (2, 4, 4)).astype(np.float32)
    d_desc, d_sal = _dev(T, desc, sal)
    stats, dmean, dm2 = lib.val_frame_stats(d_sal, descriptors=d_desc)
    bare, none1, none2 = lib.val_frame_stats(d_sal)
    assert none1 is None and none2 is None and _same(T, stats, bare), "the statistics row depends on the descriptors"
    DM, D2 = dmean.cpu().numpy(), dm2.cpu().numpy()
    for f in range(2):
        ref = val_ref.frame_stats(sal[f], None, desc[f])
        assert (np.abs(DM[f] - ref["desc_mean"]) <= val_ref.tolerance(ref["desc_mean"], scale=1.0)).all()      # unit rows
        assert (np.abs(D2[f] - ref["desc_m2"]) <= val_ref.tolerance(ref["desc_m2"])).all()
    if k == 1:
        assert np.array_equal(_bits(DM), _bits(desc[:, 0])) and not _bits(D2).any()


# ------------------------------------------------------------------------------- 4. pair statistics on hand-made arg-max arrays
@pytest.mark.parametrize("pattern,n1,n2", [(pt, a, b) for pt in vec.PATTERNS for a, b in vec.PAIR_SHAPES if pt != "identity" or a <= b])
def test_pair_stats_on_hand_made_index_arrays(T, pattern, n1, n2):
    """Every row mutual, no row mutual, and a quarter of nn12 outside [0, n2) (-1, n2, 2^31 - 1: not counted, nothing read
    through them), two pairs a launch, n1 on either side of the 256-thread stride."""
    from sslam_amd import lib
    temperature = 0.1
    z = vec.pair_arrays(pattern, n1, n2)
    d = {k: _dev(T, v)[0] for k, v in z.items()}
    ps, cnt = lib.val_pair_stats(d["sal1"], d["sal2"], d["nn12"], d["nn21"], d["s12"], d["ce"], d["s00"], temperature)
    ps2, cnt2 = lib.val_pair_stats(d["sal1"], d["sal2"], d["nn12"], d["nn21"], d["s12"], d["ce"], d["s00"], temperature)
    assert _same(T, ps, ps2) and _same(T, cnt, cnt2), "a second run gave other bits"
    ps, cnt = ps.cpu().numpy(), cnt.cpu().numpy()
    slot = lib.VAL_PAIR_SLOTS
    for p in range(2):
        want = val_ref.pair_sums(z["ce"][p], z["nn12"][p], z["nn21"][p], z["s12"][p, 0], z["s00"][p], temperature)
        n = want["n_matches"]
        assert cnt[p] == n and ps[p, slot["matches"]] == n, (pattern, p, cnt[p], n)
        if pattern == "identity":
            assert n == n1
        if pattern == "none":
            assert n == 0 and _bits(ps[p, slot["ce_sum"]]) == 0, "no mutual row: the sum is +0"
        tol = val_ref.tolerance(want["ce_sum"], scale=max(abs(want["ce_sum"]), n / temperature))      # a sum of that many rows
        print(f"{pattern} ({n1}, {n2}) pair {p}: {n} matches, ce_sum {ps[p, slot['ce_sum']]:.6f} ref {want['ce_sum']:.6f} tolerance {tol:.2e}")
        assert abs(ps[p, slot["ce_sum"]] - want["ce_sum"]) <= tol
        pad = want["pad_ce"]
        assert abs(ps[p, slot["pad_ce"]] - pad) <= val_ref.tolerance(pad, scale=max(abs(pad), 1.0 / temperature))
        rep = float(np.mean((z["sal1"][p].astype(np.float64) - z["sal2"][p]) ** 2))
        assert abs(ps[p, slot["repeat"]] - rep) <= val_ref.tolerance(rep)


# ------------------------------------------------------------------------------------------------ 5. the pipeline above 512
def test_validate_at_input_size_544(T):
    """validation.validate on 5 synthetic frames at input_size 544 (G = 34: a second column segment of 32 pixels), tokens in,
    K = 64, uint8 images through A0, a batch of 4: equal to val_ref.validate on the pipeline's OWN saliency, descriptors and A0
    image within the rule."""
    from sslam_amd import validation
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    n, g, k = 5, 34, 64
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    toks = T.from_numpy(synth.token_sequence(n, g)).cuda()
    imgs = T.from_numpy(synth.image_sequence(n, 96, 128)).cuda()
    got = validation.validate(pipe, imgs, spacing=1, batch=4, tokens=toks)
    out = pipe.extract(toks, None)
    a0 = pipe.preprocess(imgs)
    assert tuple(a0.shape) == (n, 3, 544, 544)
    first = np.arange(n - 1)
    want = val_ref.validate(out["saliency"].cpu().numpy(), a0.cpu().numpy(), out["descriptors"].cpu().numpy(), first, first + 1, batch=4,
                            temperature=0.1)
    assert set(got) == set(want) == set(("total",) + validation.TERMS + validation.METRICS)
    for key in want:
        print(f"validate at 544 {key:20s} got {got[key]:+.9e} ref64 {want[key]:+.9e} |d| {abs(got[key] - want[key]):.2e}")
    for key in want:
        assert abs(got[key] - want[key]) <= val_ref.tolerance(want[key]), (key, got[key], want[key])
