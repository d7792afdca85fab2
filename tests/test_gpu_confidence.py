"""GPU tests of the keypoint confidence head: the four device entries of libsslam_conf.so through sslam_amd.lib, and every host
layer that carries them - SequencePipeline.extract / filter_by_confidence, online.FrameStepper, the drop-in
models.uncertainty_estimator.

Reference: tests/confidence_ref.py, the header restated in numpy (a correctly rounded float32 fma built from float64, the
oracle's gather and sigmoid), and the reference's own filter outputs (tests/golden/confidence.npz).  Every comparison is of BITS,
device against restatement, never device against itself alone.  Every launch goes into poisoned outputs between guard bands, from
inputs between bands of NaN bits (tests/guarded.py); launches are counted."""
import ctypes as C
import os

import numpy as np
import pytest

import conf_table as ct
import confidence_cases as cases
import confidence_ref as ref
import guarded

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ROWS = 150


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "confidence.npz")))


def _rows(name, rows=MAX_ROWS, seed=0):
    """`rows` seeded input rows for a head: standard-normal features, unit descriptors; row 7 all zeros."""
    d = cases.HEADS[name][0]
    rng = np.random.default_rng(40 + seed)
    x = rng.standard_normal((rows, 384)).astype(F)
    desc = rng.standard_normal((rows, d))
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(F)
    if rows > 7:
        x[7], desc[7] = 0, 0
    return x, desc


@pytest.fixture(scope="module")
def heads():
    """head -> weights, packed host buffer, MAX_ROWS input rows and the restatement's confidence of them: computed once, never
    written afterwards."""
    from sslam_amd import lib
    out = {}
    for name in cases.HEADS:
        ws = ref.weight_list(cases.head_state(name))
        x, desc = _rows(name)
        out[name] = dict(ws=ws, packed=lib.confidence_pack(ws), x=x, desc=desc, want=ref.confidence_rows(x, desc, ws))
    return out


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))
    assert bad.size == 0, f"{what}: differs from the restatement in {bad.size} of {got.size} elements, the first at flat index {bad[0]}: " \
                          f"{got.reshape(-1)[bad[0]]!r} for {want.reshape(-1)[bad[0]]!r}"


def _check_inputs(ins, what):
    for name, (whole, mid, host) in ins.items():
        guarded.assert_guards(whole, mid, f"{what} {name}")
        assert mid.cpu().numpy().tobytes() == host.tobytes(), f"{what}: the input {name} was written"


def _inputs(T, **arrays):
    return {name: guarded.guarded_input(T, a, name=name) + (np.ascontiguousarray(a),) for name, a in arrays.items()}


def run_rows(T, x, desc, packed, what):
    """One guarded launch of sslc_confidence_rows -> conf as numpy.  Under a guarded.Placement every operand takes its place."""
    from sslam_amd import lib
    ins = _inputs(T, x=x, desc=desc, packed=packed)
    whole, conf = guarded.guarded(T, x.shape[:-1], T.float32, name="conf")
    n0, m0 = lib.conf_launch_count(), lib.launch_count()
    back = lib.confidence_rows(ins["x"][1], ins["desc"][1], ins["packed"][1], out=conf)
    assert lib.conf_launch_count() - n0 == 1 and lib.launch_count() == m0 and back is conf, "one launch, of the seventh library"
    guarded.assert_guards(whole, conf, f"{what} conf")
    guarded.assert_written(conf, f"{what} conf")
    _check_inputs(ins, what)
    return conf.cpu().numpy()


def run_gather(T, feat, kp, desc, packed, what):
    from sslam_amd import lib
    ins = _inputs(T, feat=feat, kp_xy=kp, desc=desc, packed=packed)
    whole, conf = guarded.guarded(T, kp.shape[:2], T.float32, name="conf")
    n0, m0 = lib.conf_launch_count(), lib.launch_count()
    lib.gather_confidence(ins["feat"][1], ins["kp_xy"][1], ins["desc"][1], ins["packed"][1], out=conf)
    assert lib.conf_launch_count() - n0 == 1 and lib.launch_count() == m0
    guarded.assert_guards(whole, conf, f"{what} conf")
    guarded.assert_written(conf, f"{what} conf")
    _check_inputs(ins, what)
    return conf.cpu().numpy()


def run_filter(T, conf, threshold, what):
    from sslam_amd import lib
    ins = _inputs(T, conf=conf)
    n, k = conf.shape
    outs = [guarded.guarded(T, shape, dt, name=name) for name, (shape, dt) in zip(("slot", "count", "conf_out"),
                                                                                  lib.confidence_filter_shapes(n, k).values())]
    n0 = lib.conf_launch_count()
    lib.confidence_filter(ins["conf"][1], threshold, out=tuple(mid for _, mid in outs))
    assert lib.conf_launch_count() - n0 == 1
    for name, (whole, mid) in zip(("slot", "count", "conf_out"), outs):
        guarded.assert_guards(whole, mid, f"{what} {name}")
        guarded.assert_written(mid, f"{what} {name}")
    _check_inputs(ins, what)
    return tuple(mid.cpu().numpy() for _, mid in outs)


def run_take(T, src, slot, what):
    from sslam_amd import lib
    ins = _inputs(T, src=src, slot=slot)
    whole, dst = guarded.guarded(T, src.shape, ins["src"][1].dtype, name="dst")
    n0 = lib.conf_launch_count()
    lib.take_rows(ins["src"][1], ins["slot"][1], out=dst)
    assert lib.conf_launch_count() - n0 == 1
    guarded.assert_guards(whole, dst, f"{what} dst")
    guarded.assert_written(dst, f"{what} dst")
    _check_inputs(ins, what)
    return dst.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the rows form
# one row; one short of, exactly, and one past a tile of 32; two tiles and one row; several tiles with a ragged last one
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 65, 150])
@pytest.mark.parametrize("name", list(cases.HEADS))
def test_rows_equal_the_restatement(T, heads, name, rows):
    h = heads[name]
    got = run_rows(T, h["x"][:rows], h["desc"][:rows], h["packed"], f"{name}, {rows} rows")
    _same_bits(got, h["want"][:rows], f"{name} (D = {cases.HEADS[name][0]}), {rows} rows")
    assert (got >= 0).all() and (got <= 1).all()
    if rows > 7:
        zero = ref.sigmoid(ref.logits(np.zeros((1, 384), F), np.zeros((1, h["desc"].shape[1]), F), h["ws"]))[0]
        assert got[7].view(np.uint32) == zero.view(np.uint32), "the all-zero row gives the sigmoid of the biases' chain"


@pytest.mark.parametrize("bias", [100.0, 1e4, -100.0, -1e4])
def test_saturating_head(T, heads, bias):
    """The x4 head with its last bias at +-100 and +-1e4: the logits leave the sigmoid's range and the confidence is exactly 1.0f
    and exactly 0.0f.  The canonical sigmoid alone stops at the subnormal 6.054601e-39 (its exponential clamps its argument to
    [-87, 88]); the head's output stage writes a subnormal result as +0.0f (include/sslam_conf.h, SSLC_CONF_MIN), which the
    restatement states too."""
    h = heads["x4"]
    ws = list(h["ws"])
    ws[5] = np.array([bias], F)
    from sslam_amd import lib
    x, desc = h["x"][:33], h["desc"][:33]
    got = run_rows(T, x, desc, lib.confidence_pack(ws), f"last bias {bias}")
    print(f"last bias {bias}: confidence {got.min()!r} .. {got.max()!r}")
    _same_bits(got, ref.confidence_rows(x, desc, ws), f"last bias {bias}")
    assert (got >= 0).all() and (got <= 1).all()
    assert (got.view(np.uint32) == np.array(1.0 if bias > 0 else 0.0, F).view(np.uint32)).all(), \
        f"saturated confidences {got.min()!r} .. {got.max()!r} are not exactly {1.0 if bias > 0 else 0.0}"


def test_the_output_floor_falls_where_the_sigmoid_turns_subnormal(T, heads):
    """The x4 head with its last bias at -80: the 150 rows' logits lie between about -95 and -77, on both sides of the logit (about
    -87.3) below which the canonical sigmoid is subnormal.  Bit for bit the restatement: the sigmoid's own bits above, +0.0f below,
    no subnormal anywhere."""
    h = heads["x4"]
    ws = list(h["ws"])
    ws[5] = np.array([-80.0], F)
    from sslam_amd import lib
    got = run_rows(T, h["x"], h["desc"], lib.confidence_pack(ws), "last bias -80")
    _same_bits(got, ref.confidence_rows(h["x"], h["desc"], ws), "last bias -80")
    s = ref.sigmoid(ref.logits(h["x"], h["desc"], ws))
    print(f"last bias -80: {int((got == 0).sum())} of {got.size} rows at zero; the least confidence above it {got[got > 0].min()!r}")
    assert (got == 0).sum() >= 5 and (got > 0).sum() >= 5, "rows on both sides of the floor"
    assert ((got == 0) | (got >= ref.CONF_MIN)).all() and (got.view(np.uint32)[got == 0] == 0).all()
    assert np.array_equal(got == 0, s < ref.CONF_MIN) and np.array_equal(got[got > 0].view(np.uint32), s[s >= ref.CONF_MIN].view(np.uint32))


@pytest.mark.parametrize("name", ["x4", "wide"])
def test_a_row_s_confidence_does_not_depend_on_its_position(T, heads, name):
    """The same row at row 0, at the last row of a tile and in a ragged last tile (row 64 of 65): the same bits, the restatement's."""
    h = heads[name]
    x, desc = h["x"][:65].copy(), h["desc"][:65].copy()
    for r in (0, 31, 64):
        x[r], desc[r] = h["x"][100], h["desc"][100]
    got = run_rows(T, x, desc, h["packed"], "position")
    assert got[0].view(np.uint32) == got[31].view(np.uint32) == got[64].view(np.uint32) == h["want"][100].view(np.uint32)
    alone = run_rows(T, x[64:], desc[64:], h["packed"], "alone")
    assert alone[0].view(np.uint32) == got[64].view(np.uint32)


# -------------------------------------------------------------------------------------------------------------- the gather form
def _gather_case(name, n, g, k, seed):
    """Features, descriptors and keypoints on the grid's borders and corners, at fractional positions and outside the grid."""
    rng = np.random.default_rng(seed)
    d = cases.HEADS[name][0]
    feat = rng.standard_normal((n, g, g, 384)).astype(F)
    desc = rng.standard_normal((n, k, d))
    desc = (desc / np.linalg.norm(desc, axis=-1, keepdims=True)).astype(F)
    kp = rng.uniform(0, g - 1, (n, k, 2)).astype(F)
    special = [(0, 0), (g - 1, g - 1), (0, g - 1), (g - 1, 0.5), (0.25, 0), (-0.5, 0.5), (g - 0.5, 1), (-3, 0), (1, g + 2), (1e9, -1e9),
               (1, 1), (g - 1.000001, 0.75)]
    flat = kp.reshape(-1, 2)
    for i, xy in enumerate(special[:max(0, len(flat) - 1)]):
        flat[1 + i] = xy
    kp[..., :k // 3, :] = np.round(kp[..., :k // 3, :])          # whole cells, as the selector writes them
    return feat, kp, desc


@pytest.mark.parametrize("n,g,k", [(1, 2, 1), (3, 5, 50), (2, 28, 33)])
@pytest.mark.parametrize("name", ["x4", "wide"])
def test_gather_form_equals_gather_then_rows_and_the_restatement(T, heads, name, n, g, k):
    from sslam_amd import lib
    h = heads[name]
    feat, kp, desc = _gather_case(name, n, g, k, 10 * g + k)
    got = run_gather(T, feat, kp, desc, h["packed"], f"{name} {n} x {g} x {k}")
    _same_bits(got, ref.gather_confidence(feat, kp, desc, h["ws"]), f"{name} gather form {n} x {g} x {k}")
    x = lib.gather(T.from_numpy(feat).cuda(), T.from_numpy(kp).cuda())
    two = lib.confidence_rows(x, T.from_numpy(desc).cuda(), T.from_numpy(h["packed"]).cuda())
    _same_bits(got, two.cpu().numpy(), "sslam_gather followed by the rows form")


# -------------------------------------------------------------------------------------------------------- the filter and the take
def _filter_conf(k, seed):
    """3 frames of k distinct confidences in (0.1, 0.9); frame 1 has its maximum twice (where there are two slots)."""
    rng = np.random.default_rng(seed)
    conf = rng.permutation(3 * k).reshape(3, k).astype(F) / F(3 * k) * F(0.8) + F(0.1)
    if k >= 2:
        a, b = sorted(rng.choice(k, 2, replace=False))
        conf[1, a] = conf[1, b] = F(0.95)
    return conf


@pytest.mark.parametrize("k", [1, 64, 65, 257, 4096])
def test_filter_equals_the_restatement(T, k):
    conf = _filter_conf(k, k)
    top = conf.max()
    thresholds = dict(none=2.0, one=float(top), all=0.0, half=float(np.median(conf)), tie=float(conf[0, k // 2]), nan=float("nan"))
    for tag, thr in thresholds.items():
        slot, count, out = run_filter(T, conf, thr, f"K = {k}, {tag}")
        rs, rc, ro = ref.confidence_filter(conf, thr)
        assert np.array_equal(slot, rs) and np.array_equal(count, rc), (k, tag)
        _same_bits(out, ro, f"K = {k}, {tag}: conf_out")
        if tag in ("none", "nan"):
            assert (count == 1).all() and np.array_equal(slot[:, 0], conf.argmax(axis=1)), "each frame keeps its first largest confidence"
            assert k < 2 or (conf[1] == conf[1].max()).sum() == 2, "frame 1 has a tie for the maximum"
        if tag == "one":
            assert sorted(count.tolist())[:2] == [1, 1] and (conf >= F(thr)).sum() in (1, 2)
        if tag == "all":
            assert (count == k).all() and np.array_equal(slot, np.tile(np.arange(k, dtype=np.int32), (3, 1)))
        if tag == "tie":
            assert k // 2 in slot[0, :count[0]], "a confidence equal to the threshold is kept"
        if tag == "half" and k > 1:
            assert abs(int(count.sum()) - 3 * k // 2) <= 2


@pytest.mark.parametrize("width", [1, 2, 128, 256])
def test_take_rows_equals_the_restatement(T, width):
    k = 65
    conf = _filter_conf(k, 3)
    slot = ref.confidence_filter(conf, float(np.median(conf)))[0]
    rng = np.random.default_rng(width)
    src = rng.standard_normal((3, k, width)).astype(F)
    got = run_take(T, src, slot, f"width {width}")
    assert got.tobytes() == ref.take_rows(src, slot).tobytes()
    ints = rng.integers(-2 ** 31, 2 ** 31 - 1, (3, k, width)).astype(np.int32)          # bit patterns, NaN payloads among them
    assert run_take(T, ints, slot, f"int32 width {width}").tobytes() == ref.take_rows(ints, slot).tobytes()
    if width == 2:
        wild = slot.copy()
        wild[0, 0], wild[1, 1], wild[2, 2] = -1, k, 2 ** 31 - 1
        assert run_take(T, src, wild, "slots outside the frame").tobytes() == ref.take_rows(src, wild).tobytes()
        flat = run_take(T, src[..., 0].copy(), slot, "rows of one word, (n, K)")
        assert flat.tobytes() == ref.take_rows(src[..., 0], slot).tobytes()


def test_dropin_filter_equals_the_reference_s_padded_outputs(T, gold):
    from models.uncertainty_estimator import UncertaintyEstimator
    from sslam_amd import lib
    m = UncertaintyEstimator().cuda().eval()
    conf = T.from_numpy(gold[f"{cases.FILTER_HEAD}_conf"]).cuda()
    _, desc, kp = (T.from_numpy(a).cuda() for a in cases.head_inputs(cases.FILTER_HEAD))
    for tag in ("half", "median", "tie", "none"):
        n0 = lib.conf_launch_count()
        with T.no_grad():
            out = m.filter_keypoints_by_confidence(kp, desc, conf, threshold=float(gold[f"filter_{tag}_threshold"]))
        assert lib.conf_launch_count() - n0 == 3, "the filter and two takes"
        for got, key in zip(out, ("keypoints", "descriptors", "confidence")):
            w = gold[f"filter_{tag}_{key}"]
            assert tuple(got.shape) == w.shape and got.cpu().numpy().tobytes() == w.tobytes(), (tag, key)


# ------------------------------------------------------------------------------------------------------------- the disciplines
def _launch(T, entry, heads, what):
    """One guarded launch of `entry` on fixed operands -> (got, want) lists of arrays."""
    h = heads["x4"]
    if entry == "sslc_confidence_rows":
        return [run_rows(T, h["x"][:33], h["desc"][:33], h["packed"], what)], [h["want"][:33]]
    if entry == "sslc_gather_confidence":
        feat, kp, desc = _gather_case("x4", 2, 5, 33, 1)
        return [run_gather(T, feat, kp, desc, h["packed"], what)], [ref.gather_confidence(feat, kp, desc, h["ws"])]
    conf = _filter_conf(65, 8)
    thr = float(np.median(conf))
    if entry == "sslc_confidence_filter":
        return list(run_filter(T, conf, thr, what)), list(ref.confidence_filter(conf, thr))
    slot = ref.confidence_filter(conf, thr)[0]
    src = np.random.default_rng(2).standard_normal((3, 65, 3)).astype(F)
    return [run_take(T, src, slot, what)], [ref.take_rows(src, slot)]


@pytest.mark.parametrize("mode", ["lo", "hi"])
@pytest.mark.parametrize("entry", list(ct.ALIGN))
def test_every_pointer_at_its_least_alignment(T, heads, entry, mode):
    """Each operand at the alignment include/sslam_conf.h states and no better, just past and just before a 256-byte boundary:
    the restatement's bits all the same."""
    with guarded.placed(guarded.Placement(ct.ALIGN[entry], mode)) as p:
        got, want = _launch(T, entry, heads, f"{entry} placed {mode}")
    assert sorted(r["name"] for r in p.made) == sorted(ct.ALIGN[entry])
    for r in p.made:
        a = r["align"]
        assert r["middle"].data_ptr() % 256 == (a if mode == "lo" else 256 - a), r["name"]
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes(), f"{entry} placed {mode}"


def test_every_refusal_comes_before_the_launch_and_writes_nothing(T, heads):
    from sslam_amd import lib
    L = lib.conf()
    stream = lambda: C.c_void_p(T.cuda.current_stream().cuda_stream)       # noqa: E731
    h = heads["x4"]
    n, g, k, d, w = 2, 4, 5, 128, 3
    feat, kp, desc = _gather_case("x4", n, g, k, 3)
    ins = _inputs(T, x=h["x"][:n * k], desc=desc, packed=h["packed"], feat=feat, kp_xy=kp, conf_in=_filter_conf(k, 1)[:n],
                  slot_in=np.zeros((n, k), np.int32), src=np.zeros((n, k, w), F))
    outs = dict(conf=guarded.guarded(T, (n, k), T.float32), slot=guarded.guarded(T, (n, k), T.int32), count=guarded.guarded(T, (n,), T.int32),
                conf_out=guarded.guarded(T, (n, k), T.float32), dst=guarded.guarded(T, (n, k, w), T.float32))
    at = {name: v[1].data_ptr() for name, v in {**ins, **outs}.items()}
    calls = {   # entry -> (call(pointers, sizes), pointer names in the header's order, sizes, {size name: (values, code)})
        "sslc_confidence_rows": (lambda p, s: L.sslc_confidence_rows(p[0], p[1], s["rows"], s["D"], p[2], p[3], stream()),
                                 ("x", "desc", "packed", "conf"), dict(rows=n * k, D=d),
                                 dict(rows=((0, -1), lib.E_INVALID), D=((0, 64, 129, 384, -128), lib.E_UNSUPPORTED))),
        "sslc_gather_confidence": (lambda p, s: L.sslc_gather_confidence(p[0], s["n"], s["G"], p[1], s["K"], p[2], s["D"], p[3], p[4], stream()),
                                   ("feat", "kp_xy", "desc", "packed", "conf"), dict(n=n, G=g, K=k, D=d),
                                   dict(n=((0, -1), lib.E_INVALID), G=((1, 0, -4), lib.E_INVALID), K=((0, -5), lib.E_INVALID),
                                        D=((0, 64, 512), lib.E_UNSUPPORTED))),
        "sslc_confidence_filter": (lambda p, s: L.sslc_confidence_filter(p[0], s["n"], s["K"], C.c_float(0.5), p[1], p[2], p[3], stream()),
                                   ("conf_in", "slot", "count", "conf_out"), dict(n=n, K=k),
                                   dict(n=((0, -1), lib.E_INVALID), K=((0, -1), lib.E_INVALID))),
        "sslc_take_rows": (lambda p, s: L.sslc_take_rows(p[0], p[1], s["n"], s["K"], s["width"], p[2], stream()),
                           ("src", "slot_in", "dst"), dict(n=n, K=k, width=w),
                           dict(n=((0, -1), lib.E_INVALID), K=((0, -2), lib.E_INVALID), width=((0, -1), lib.E_INVALID))),
    }
    n0 = lib.conf_launch_count()
    for entry, (call, names, sizes, bad_sizes) in calls.items():
        aligns = list(ct.ALIGN[entry].values())
        ok = [C.c_void_p(at[name]) for name in names]
        for i in range(len(names)):
            assert call([None if j == i else v for j, v in enumerate(ok)], sizes) == lib.E_INVALID, f"{entry}: NULL {names[i]}"
            half = [C.c_void_p(at[name] + (aligns[j] // 2 if j == i else 0)) for j, name in enumerate(names)]
            assert call(half, sizes) == lib.E_INVALID, f"{entry}: {names[i]} at half its alignment"
        for key, (values, code) in bad_sizes.items():
            for v in values:
                assert call(ok, {**sizes, key: v}) == code, f"{entry}: {key} = {v}"
    big = [C.c_void_p(at[name]) for name in ("conf_in", "slot", "count", "conf_out")]
    assert calls["sslc_confidence_filter"][0](big, dict(n=1, K=4097)) == lib.E_UNSUPPORTED, "K = 4097"
    assert calls["sslc_confidence_filter"][0](big, dict(n=1, K=2 ** 31 - 1)) == lib.E_UNSUPPORTED
    rows_p = [C.c_void_p(at[name]) for name in ("x", "desc", "packed", "conf")]
    assert calls["sslc_confidence_rows"][0](rows_p, dict(rows=2 ** 31, D=d)) == lib.E_UNSUPPORTED
    gat_p = [C.c_void_p(at[name]) for name in ("feat", "kp_xy", "desc", "packed", "conf")]
    assert calls["sslc_gather_confidence"][0](gat_p, dict(n=2 ** 20, G=g, K=2 ** 11, D=d)) == lib.E_UNSUPPORTED
    take_p = [C.c_void_p(at[name]) for name in ("src", "slot_in", "dst")]
    for shape in (dict(n=2 ** 20, K=2 ** 11, width=1), dict(n=2 ** 10, K=2 ** 11, width=2 ** 10), dict(n=2 ** 31 - 1, K=2 ** 31 - 1, width=2 ** 31 - 1)):
        assert calls["sslc_take_rows"][0](take_p, shape) == lib.E_UNSUPPORTED, shape
    same = [C.c_void_p(at["src"]), C.c_void_p(at["slot_in"]), C.c_void_p(at["src"])]
    assert calls["sslc_take_rows"][0](same, dict(n=n, K=k, width=w)) == lib.E_INVALID, "dst == src"
    alias = [C.c_void_p(at["conf_in"]), C.c_void_p(at["slot"]), C.c_void_p(at["count"]), C.c_void_p(at["conf_in"])]
    assert calls["sslc_confidence_filter"][0](alias, dict(n=n, K=k)) == lib.E_INVALID, "conf_out == conf"
    T.cuda.synchronize()
    assert lib.conf_launch_count() == n0, "a refusal launched"
    for name, (whole, mid) in outs.items():
        assert bool((whole.view(T.int32) == guarded.SENTINEL).all()), f"a refusal wrote {name}"
    # the same pointers with the sizes they were made for: accepted, one launch each
    for entry, (call, names, sizes, _) in calls.items():
        assert call([C.c_void_p(at[name]) for name in names], sizes) == lib.OK, entry
    assert lib.conf_launch_count() == n0 + 4
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.confidence_filter(T.zeros((1, 4097), device="cuda"), 0.5)
    with pytest.raises(ValueError, match="different devices|CUDA"):
        lib.confidence_filter(T.zeros((1, 4)), 0.5)
    assert lib.conf_launch_count() == n0 + 4


# ------------------------------------------------------------------------------------------------------------------ the layers
N_SEQ, K_SEQ, G_SEQ = 3, 100, 28


@pytest.fixture(scope="module")
def seq(T):
    import synth
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    ssd, rsd, csd = synth.selector_state(0), synth.refiner_state(0), cases.head_state("x4")
    kw = dict(input_size=16 * G_SEQ, num_keypoints=K_SEQ)
    make = lambda **more: SequencePipeline(ExtractorConfig(**kw, **more), ssd, rsd, device="cuda", confidence_state=csd)       # noqa: E731
    toks_h = synth.token_sequence(N_SEQ, G_SEQ)
    toks, imgs = T.from_numpy(toks_h).cuda(), T.from_numpy(synth.image_sequence(N_SEQ, 48, 64)).cuda()
    off, on = SequencePipeline(ExtractorConfig(**kw), ssd, rsd, device="cuda"), make(confidence=True)
    return dict(off=off, on=on, make=make, toks=toks, toks_h=toks_h, imgs=imgs, ws=ref.weight_list(csd), ex_off=off.extract(toks, imgs),
                ex_on=on.extract(toks, imgs))


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_extract_confidence_equals_the_restatement_and_leaves_the_rest(T, seq):
    from oracle import ora
    a, b = seq["ex_off"], seq["ex_on"]
    assert list(b) == list(a) + ["confidence"] and b["confidence"].shape == (N_SEQ, K_SEQ) and b["confidence"].dtype == T.float32
    for key in a:
        assert _bytes_equal(a[key], b[key]), f"extract: {key} changed under confidence=True"
    feat = ora.bn_tokens(seq["toks_h"])[0].reshape(N_SEQ, G_SEQ, G_SEQ, 384)
    want = ref.gather_confidence(feat, b["keypoints_patch"].cpu().numpy(), b["descriptors"].cpu().numpy(), seq["ws"])
    _same_bits(b["confidence"].cpu().numpy(), want, "extract: confidence")
    c = want
    print(f"extract: confidence {c.min():.3g} .. {c.max():.3g}, median {np.median(c):.3g}")
    # under subcell_descriptors the head gathers where the descriptors were gathered: at the refined keypoints
    sub = seq["make"](confidence=True, subcell=True, subcell_descriptors=True).extract(seq["toks"], seq["imgs"])
    want = ref.gather_confidence(feat, sub["keypoints_subpatch"].cpu().numpy(), sub["descriptors"].cpu().numpy(), seq["ws"])
    _same_bits(sub["confidence"].cpu().numpy(), want, "extract, subcell descriptors: confidence")
    assert not _bytes_equal(sub["confidence"], b["confidence"])
    with pytest.raises(ValueError, match="confidence"):
        seq["on"].extract(seq["toks"], seq["imgs"], out=seq["off"].alloc_extract(N_SEQ, True))
    with pytest.raises(ValueError, match="holds no confidence"):
        seq["on"].filter_by_confidence(a, 0.5)


def test_filter_by_confidence_feeds_the_matcher(T, seq):
    from oracle import ora
    from sslam_amd import lib
    ex = seq["ex_on"]
    conf = ex["confidence"].cpu().numpy()
    thr = float(np.median(conf))
    n0 = lib.conf_launch_count()
    f = seq["on"].filter_by_confidence(ex, thr)
    per_kp = [k for k in ex if k not in ("saliency", "status", "confidence")]
    assert lib.conf_launch_count() - n0 == 1 + len(per_kp), "one filter launch and one take per per-keypoint array"
    assert list(f) == list(ex) + ["count", "slot"]
    slot, count, out = ref.confidence_filter(conf, thr)
    assert np.array_equal(f["slot"].cpu().numpy(), slot) and np.array_equal(f["count"].cpu().numpy(), count)
    _same_bits(f["confidence"].cpu().numpy(), out, "filtered confidence")
    assert 0 < count.min() and count.max() < K_SEQ
    for key in per_kp:
        assert f[key].shape == ex[key].shape and f[key].cpu().numpy().tobytes() == ref.take_rows(ex[key].cpu().numpy(), slot).tobytes(), key
    assert _bytes_equal(f["saliency"], ex["saliency"]) and _bytes_equal(f["status"], ex["status"])
    m = seq["on"].match(f["descriptors"], f["scores"], f["intensity"], spacing=1)
    cfg = seq["on"].cfg
    d, s, i = (f[key].cpu().numpy() for key in ("descriptors", "scores", "intensity"))
    for p in range(N_SEQ - 1):
        mt, q = ora.match_with_quality(d[p], d[p + 1], s[p], s[p + 1], cfg.saliency_weight, cfg.min_saliency, cfg.min_descriptor_sim,
                                       i[p], i[p + 1], cfg.min_intensity)
        c = int(m["match_count"][p])
        assert c == len(mt) and np.array_equal(m["matches"][p, :c].cpu().numpy(), mt), f"pair {p}"
        assert np.array_equal(m["quality"][p, :c].cpu().numpy().view(np.uint32), q.view(np.uint32)), f"pair {p}"


@pytest.mark.parametrize("use_graph", [False, True])
def test_one_stepper_step_equals_extract(T, seq, use_graph):
    from sslam_amd import lib
    from sslam_amd.online import FrameStepper
    st = FrameStepper(seq["on"], 48, 64, use_graph=use_graph, tokens_in=True)
    for i in range(2):
        n0 = lib.conf_launch_count()
        out = st.step(seq["imgs"][i], seq["toks"][i])
        if use_graph and i:
            assert lib.conf_launch_count() == n0, "a replayed step makes no library call"
        for key in ("confidence", "descriptors", "keypoints_pixel", "idx"):
            assert _bytes_equal(out[key], seq["ex_on"][key][i]), f"frame {i}: {key} (graph {use_graph})"
    plain = FrameStepper(seq["off"], 48, 64, use_graph=False, tokens_in=True)
    assert "confidence" not in plain.step(seq["imgs"][0], seq["toks"][0]), "a pipeline without the head returns what it returned"


@pytest.mark.parametrize("name", ["x4", "wide"])
def test_dropin_forward_runs_the_kernel_under_no_grad(T, heads, name):
    from models.uncertainty_estimator import UncertaintyEstimator
    from sslam_amd import lib
    h = heads[name]
    m = UncertaintyEstimator(384, cases.HEADS[name][0], 128).cuda().eval()
    m.load_state_dict({k: T.from_numpy(v) for k, v in cases.head_state(name).items()})
    x, desc = T.from_numpy(h["x"][:66].reshape(2, 33, -1)).cuda(), T.from_numpy(h["desc"][:66].reshape(2, 33, -1)).cuda()
    n0 = lib.conf_launch_count()
    with T.no_grad():
        conf = m(x, desc)
    assert lib.conf_launch_count() == n0 + 1, "the drop-in's forward ran sslc_confidence_rows"
    assert conf.shape == (2, 33, 1)
    _same_bits(conf.cpu().numpy()[..., 0], h["want"][:66].reshape(2, 33), "drop-in forward")
    eager = m(x, desc)                                           # gradients on: torch ops on the same Parameters
    assert lib.conf_launch_count() == n0 + 1 and eager.requires_grad
    assert float((eager.detach() - conf).abs().max()) < 1e-5
    with T.no_grad():                                            # a changed parameter is packed again
        m.mlp[4].bias.add_(1.0)
        moved = m(x, desc)
    ws = list(h["ws"])
    ws[5] = (ws[5] + F(1.0)).astype(F)
    _same_bits(moved.cpu().numpy()[..., 0], ref.confidence_rows(h["x"][:66], h["desc"][:66], ws).reshape(2, 33), "after an in-place update")
