"""CPU tests of the keypoint confidence head: the numpy restatement (tests/confidence_ref.py) against what the reference's own
UncertaintyEstimator computed (tests/golden/confidence.npz, written by tests/golden/make_golden_confidence.py), the drop-in
models.uncertainty_estimator - its surface and its eager path - against the same fixture, and the interface of
libsslam_conf.so: include/sslam_conf.h, sslam_amd.lib.CONF_EXPORTS and tests/conf_table.py hold the same entries (the built
library's symbols are tests/test_libraries_cpu.py).  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import conf_table as ct
import confidence_cases as cases
import confidence_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sslam_conf.h")
TAGS = ("half", "median", "tie", "none")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "confidence.npz")))


@pytest.fixture(scope="module")
def restated():
    """head -> the restatement's confidences (B, N), computed once."""
    out = {}
    for name in cases.HEADS:
        x, desc, _ = cases.head_inputs(name)
        out[name] = ref.confidence_rows(x, desc, ref.weight_list(cases.head_state(name)))
    return out


# ------------------------------------------------------------------------------------------------- restatement against reference
@pytest.mark.parametrize("name", list(cases.HEADS))
def test_restatement_is_as_close_to_float64_as_the_reference(gold, restated, name):
    """Two fp32 summation orders of 384 + D terms differ by order-dependent rounding, so the restatement (one fma chain) is held to
    the float64 evaluation of the same head, at 4 x the reference's own distance e_ref from it - a bound computed here from the
    stored arrays.  Measured on the fixture's draw (e_ref, restatement): default 4.96e-8, 6.93e-8; x4 4.94e-7, 5.11e-7; wide
    5.18e-8, 7.06e-8 - ratios 1.40, 1.04, 1.36."""
    f64 = gold[f"{name}_conf_f64"][..., 0]
    e_ref = float(np.abs(gold[f"{name}_conf"][..., 0].astype(np.float64) - f64).max())
    e_re = float(np.abs(restated[name].astype(np.float64) - f64).max())
    print(f"{name}: reference to float64 {e_ref:.3g}, restatement to float64 {e_re:.3g}, ratio {e_re / e_ref:.2f}")
    assert np.abs(ref.confidence_f64(*cases.head_inputs(name)[:2], ref.weight_list(cases.head_state(name))) - f64).max() < 1e-12, \
        "the stored float64 evaluation is of these weights and inputs"
    assert e_ref > 0 and e_re <= 4 * e_ref
    c = restated[name]
    assert c.dtype == np.float32 and c.shape == (cases.B, cases.N) and (c >= 0).all() and (c <= 1).all()


def test_the_heads_cover_a_flat_and_a_wide_range(gold):
    c = gold["default_conf"]
    assert 0.40 < c.min() and c.max() < 0.53, "the default init gives confidences in a flat band below and around one half"
    c = gold["x4_conf"]
    assert c.min() < 1e-5 and c.max() > 0.9, "every parameter x 4: the confidences spread over most of (0, 1)"
    assert gold["wide_conf"].shape == (cases.B, cases.N, 1)


@pytest.mark.parametrize("tag", TAGS)
def test_filter_outputs_equal_the_reference(gold, tag):
    """The restated filter and takes, on the reference's own confidences: keypoints, descriptors and confidence equal
    filter_keypoints_by_confidence's bit for bit, padded length included."""
    conf = gold[f"{cases.FILTER_HEAD}_conf"]
    _, desc, kp = cases.head_inputs(cases.FILTER_HEAD)
    thr = gold[f"filter_{tag}_threshold"]
    assert thr == cases.thresholds(conf[..., 0])[tag]
    (fk, fd), fc = ref.filter_padded([kp, desc], conf[..., 0], thr)
    for got, key in ((fk, "keypoints"), (fd, "descriptors"), (fc, "confidence")):
        want = gold[f"filter_{tag}_{key}"]
        assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes(), (tag, key)
    slot, count, _ = ref.confidence_filter(conf[..., 0], thr)
    if tag == "none":
        assert fk.shape[1] == 1 and (count == 1).all() and np.array_equal(slot[:, 0], conf[..., 0].argmax(axis=1))
    if tag == "tie":
        f, k = cases.TIE_SLOT
        assert conf[f, k, 0] == thr and k in slot[f, :count[f]], "a confidence equal to the threshold is kept"
    if tag == "median":
        assert count.sum() == conf.size // 2
    assert (slot[:, :1] >= 0).all() and all((np.diff(slot[f, :count[f]]) > 0).all() for f in range(cases.B))


@pytest.mark.parametrize("name", list(cases.HEADS))
def test_losses_equal_the_reference(gold, name):
    err = cases.error_array()
    conf = gold[f"{name}_conf"]
    for fn, key in ((ref.calibration_loss, "calibration_loss"), (ref.expected_error_loss, "expected_error_loss")):
        got, want = fn(conf, err), float(gold[f"{name}_{key}"])
        assert abs(got - want) <= 1e-6 * abs(want), (key, got, want)


def test_restated_output_writes_no_subnormal():
    """The canonical sigmoid's floor is a subnormal; the head writes +0.0f for it and the sigmoid's own bits everywhere else."""
    logit = np.array([-1e4, -100.0, -88.0, -87.5, -87.3, -87.0, -20.0, 0.0, 16.0, 17.5, 100.0, 1e4], np.float32)
    s, c = ref.sigmoid(logit), ref.output(logit)
    assert s[0] == s[1] == s[2] and 0 < s[0] < ref.CONF_MIN, "the floor of the canonical sigmoid: 6.05e-39"
    assert (c[:4].view(np.uint32) == 0).all() and (c[-3:] == 1).all()
    normal = s >= ref.CONF_MIN
    assert normal[5:].all() and np.array_equal(c[normal].view(np.uint32), s[normal].view(np.uint32))
    assert (c[~normal].view(np.uint32) == 0).all() and ((c == 0) | (c >= ref.CONF_MIN)).all()


def test_restated_filter_edges():
    nan = np.float32(np.nan)
    conf = np.array([[0.2, 0.7, 0.7, 0.1], [0.3, 0.3, 0.1, 0.3], [nan, 0.2, nan, 0.6], [nan, nan, nan, nan]], np.float32)
    slot, count, out = ref.confidence_filter(conf, 0.7)
    assert slot.tolist() == [[1, 2, 2, 2], [0, 0, 0, 0], [3, 3, 3, 3], [0, 0, 0, 0]] and count.tolist() == [2, 1, 1, 1]
    assert out[0].tolist() == [np.float32(0.7)] * 2 + [0, 0] and out[1].tolist() == [np.float32(0.3), 0, 0, 0] and np.isnan(out[3, 0])
    slot, count, _ = ref.confidence_filter(conf[:3], nan)
    assert count.tolist() == [1, 1, 1] and slot[:, 0].tolist() == [1, 0, 3]
    src = np.arange(4 * 4 * 2, dtype=np.int32).reshape(4, 4, 2)
    got = ref.take_rows(src, np.array([[3, 0, 4, -1]] * 4, np.int32))
    assert got[1].tolist() == [[14, 15], [8, 9], [0, 0], [0, 0]]


# ------------------------------------------------------------------------------------------------------------------ the drop-in
def _module():
    import torch
    from models.uncertainty_estimator import UncertaintyEstimator
    return torch, UncertaintyEstimator


def test_dropin_surface_is_the_reference_s():
    """Constructor, attributes, state_dict keys and the five methods' signatures of models/uncertainty_estimator.py."""
    torch, U = _module()
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    E = inspect.Parameter.empty
    assert sig(U.__init__) == [("self", E), ("dino_dim", 384), ("descriptor_dim", 128), ("hidden_dim", 128)]
    assert sig(U.forward) == [("self", E), ("dino_features", E), ("descriptors", E)]
    assert sig(U.compute_calibration_loss) == [("self", E), ("predicted_confidence", E), ("actual_error", E), ("epsilon", 1e-6)]
    assert sig(U.compute_expected_error_loss) == [("self", E), ("predicted_confidence", E), ("actual_error", E)]
    assert sig(U.filter_keypoints_by_confidence) == [("self", E), ("keypoints", E), ("descriptors", E), ("confidence", E), ("threshold", 0.5)]
    m = U()
    assert (m.dino_dim, m.descriptor_dim) == (384, 128)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "mlp.0.weight": (128, 512), "mlp.0.bias": (128,), "mlp.2.weight": (64, 128), "mlp.2.bias": (64,), "mlp.4.weight": (1, 64),
        "mlp.4.bias": (1,)}
    assert [type(layer).__name__ for layer in m.mlp] == ["Linear", "ReLU", "Linear", "ReLU", "Linear", "Sigmoid"]
    odd = U(32, 16, 8)       # any widths the reference accepts
    with pytest.warns(UserWarning, match="outside the HIP"):
        assert not odd._hip_ok(torch.zeros(1))
    assert odd(torch.zeros(2, 3, 32), torch.zeros(2, 3, 16)).shape == (2, 3, 1)


@pytest.mark.parametrize("name", list(cases.HEADS))
def test_dropin_eager_path_equals_the_fixture(gold, name):
    torch, U = _module()
    d = cases.HEADS[name][0]
    m = U(cases.DINO_DIM, d, cases.HIDDEN_DIM).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cases.head_state(name).items()})
    x, desc, kp = (torch.from_numpy(a) for a in cases.head_inputs(name))
    err = torch.from_numpy(cases.error_array())
    with torch.no_grad():
        conf = m(x, desc)
    want = gold[f"{name}_conf"]
    assert conf.shape == want.shape and conf.dtype == torch.float32
    # the same torch ops on the same weights; another torch build may order a GEMM's sums otherwise: the reference's own distance
    # from float64 bounds that, as above
    e_ref = np.abs(want.astype(np.float64) - gold[f"{name}_conf_f64"]).max()
    assert np.abs(conf.numpy().astype(np.float64) - gold[f"{name}_conf_f64"]).max() <= 4 * e_ref
    ref_conf = torch.from_numpy(want)
    for fn, key in ((m.compute_calibration_loss, "calibration_loss"), (m.compute_expected_error_loss, "expected_error_loss")):
        got = fn(ref_conf, err)
        assert got.shape == () and abs(float(got) - float(gold[f"{name}_{key}"])) <= 1e-6 * abs(float(gold[f"{name}_{key}"]))
    if name == cases.FILTER_HEAD:
        for tag in TAGS:
            out = m.filter_keypoints_by_confidence(kp, desc, ref_conf.clone(), threshold=float(gold[f"filter_{tag}_threshold"]))
            assert isinstance(out, tuple) and len(out) == 3
            for got, key in zip(out, ("keypoints", "descriptors", "confidence")):
                w = gold[f"filter_{tag}_{key}"]
                assert tuple(got.shape) == w.shape and got.numpy().tobytes() == w.tobytes(), (tag, key)


def test_dropin_losses_carry_gradients():
    torch, U = _module()
    m = U()
    x, desc = torch.randn(2, 5, 384), torch.randn(2, 5, 128)
    conf = m(x, desc)
    assert conf.requires_grad and conf.shape == (2, 5, 1)
    (m.compute_calibration_loss(conf, torch.rand(2, 5)) + m.compute_expected_error_loss(conf, torch.rand(2, 5))).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


# ---------------------------------------------------------------------------------------------------------------- the interface
def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_header_symbols_exports_and_table_agree():
    """The table and the constants against the export list; that list against the header and the built library is
    tests/test_libraries_cpu.py."""
    from sslam_amd import lib
    declared = lib.CONF_EXPORTS
    assert set(ct.ALIGN) | set(ct.HOST_ONLY) == set(declared) and not set(ct.ALIGN) & set(ct.HOST_ONLY) and set(ct.LIMITS) == set(ct.ALIGN)
    consts = {k: int(v) for k, v in re.findall(r"#define (SSLC_\w+) (\d+)\s", open(HEADER).read())}
    assert re.findall(r"#define SSLC_CONF_MIN (\S+)f ", open(HEADER).read()) == ["1.17549435e-38"] and \
        ref.CONF_MIN == np.float32(1.17549435e-38) == np.finfo(np.float32).tiny
    assert consts == dict(SSLC_DINO_DIM=ct.DINO_DIM, SSLC_HIDDEN_DIM=ct.HIDDEN_DIM, SSLC_FILTER_MAX_K=ct.FILTER_MAX_K, SSLC_TILE_ROWS=ct.TILE_ROWS)
    assert (lib.CONF_DINO_DIM, lib.CONF_HIDDEN_DIM, lib.CONF_FILTER_MAX_K) == (ct.DINO_DIM, ct.HIDDEN_DIM, ct.FILTER_MAX_K) == \
        (ref.DINO_DIM, ref.HIDDEN_DIM, ref.FILTER_MAX_K)
    assert lib.CONF_STATE_KEYS == ref.STATE_KEYS == cases.STATE_KEYS


def test_the_header_states_both_tables_line_for_line():
    elem = {"int32_t": 4, "float": 4, "void": 4}         # sslc_take_rows moves 4-byte words of any type
    for entry, row in ct.ALIGN.items():
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*?)\)\s*;", _header())
        assert m, entry
        args = [re.match(r"(.*?)(\w+)$", " ".join(a.split())).groups() for a in m.group(1).split(",")]
        pointers = [(t.strip(), n) for t, n in args if "*" in t and n != "stream"]
        assert [n for _, n in pointers] == list(row), entry
        for t, n in pointers:
            assert row[n] in (4, 16) and row[n] >= elem[t.replace("const", "").replace("*", "").strip()], (entry, n)
    raw = open(HEADER).read()
    for title, lines in (("ALIGNMENT, every entry", ct.header_lines()), ("SIZE LIMITS: the expressions", ct.limit_lines())):
        start = raw.index(title)
        stated = re.sub(r"\n \*\s+", " ", raw[start:raw.index("*/", start)]).strip()
        for line in lines:
            assert line + " " in stated + " ", f"include/sslam_conf.h does not state: {line}"
        assert len(re.findall(r"\bsslc_\w+: ", stated)) == len(ct.ALIGN)
    for text in ("acc = fmaf(in[k], W1[n][k], acc)", "acc = fmaf(h1[k], W2[n][k], acc)", "acc = fmaf(h2[k], W3[k], acc)",
                 "relu(v) = v > 0 ? v : +0.0f", "1.0f / (1.0f + expf_c(-logit))", "conf  = s < SSLC_CONF_MIN ? +0.0f : s", "conf[k] >= threshold", "the lowest index on equality",
                 "Every element of the three outputs is written", "every refusal comes before anything is launched and writes nothing",
                 "The same bits as sslam_gather followed by sslc_confidence_rows", "Rows are independent"):
        assert text in re.sub(r"\n \*\s+", " ", raw), text          # the comments' lines joined, the margin dropped
    assert 4 * ct.TILE_ROWS * (ct.DINO_DIM + 256 + 4) <= 160 * 1024 and 2 * 4 * ct.TILE_ROWS * (ct.DINO_DIM + 128 + 4) <= 160 * 1024, \
        "one 256-wide tile, two 128-wide tiles fit a CU's 160 KB of LDS"
    assert 4 * ct.FILTER_MAX_K + 4 * 3 * 256 + 4 <= 64 * 1024, "the filter's static LDS fits 64 KB"


# ------------------------------------------------------------------------------------------------------------- host-side layers
def test_the_packer_writes_fragment_order_and_refuses_other_widths():
    from sslam_amd import lib
    kp8 = lambda k: (k & ~7) | ((k & 1) << 2) | ((k & 7) >> 1)       # noqa: E731
    for name, (d, _, _) in cases.HEADS.items():
        ws = ref.weight_list(cases.head_state(name))
        packed = lib.confidence_pack(ws)
        lay = lib.confidence_layout(d)
        assert packed.dtype == np.float32 and packed.shape == (lay.total,) == (ct.packed_floats(d),) and lay.d == d
        assert all(o % 4 == 0 for o in (lay.w1, lay.b1, lay.w2, lay.b2, lay.w3, lay.b3))
        for off, w in ((lay.w1, ws[0]), (lay.w2, ws[2])):
            n_out, k_in = w.shape
            k, n = np.meshgrid(np.arange(k_in), np.arange(n_out))
            pos = off + ((k // 8) * n_out + n) * 8 + (kp8(k % 8))
            assert np.array_equal(packed[pos], w)
        for off, w in ((lay.b1, ws[1]), (lay.b2, ws[3]), (lay.w3, ws[4].reshape(-1)), (lay.b3, ws[5])):
            assert np.array_equal(packed[off:off + w.size], w)
    for dims in ((384, 64, 128), (384, 128, 64), (256, 128, 128), (384, 192, 128)):
        assert not lib.confidence_supported(*dims)
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.confidence_layout(dims[1], dims[0], dims[2])
    assert lib.confidence_supported(384, 128, 128) and lib.confidence_supported(384, 256, 128)
    with pytest.raises(ValueError):
        lib.confidence_pack(ws[:5])
    with pytest.raises(ValueError):
        lib.confidence_pack([ws[0], ws[1], ws[2], ws[3], ws[4].reshape(-1), ws[5]])


def test_every_check_comes_before_the_library_is_loaded(monkeypatch):
    import torch
    from sslam_amd import lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were judged")
    conf = torch.zeros((2, 5))
    lib.packed_confidence_width(torch.zeros(ct.packed_floats(128)))      # fills the width cache through the library, before it is barred
    monkeypatch.setattr(lib, "conf", boom)
    for bad in ((conf.double(), 0.5), (conf[0], 0.5), (conf, "0.5"), (conf, True), (conf, None), (torch.zeros((2, 0)), 0.5),
                (conf.t(), 0.5), (conf.numpy(), 0.5), (torch.zeros((1, 4097)), 0.5)):
        with pytest.raises((ValueError, lib.SslamHipError)):
            lib.confidence_filter(*bad)
    with pytest.raises(ValueError, match="out"):
        lib.confidence_filter(conf, 0.5, out=(conf, conf))
    slot = torch.zeros((2, 5), dtype=torch.int32)
    src = torch.zeros((2, 5, 3))
    for bad in ((src, slot.long()), (src, slot[:1]), (src.double(), slot), (src[0], slot), (src.numpy(), slot), (src, None)):
        with pytest.raises(ValueError):
            lib.take_rows(*bad)
    with pytest.raises(ValueError, match="must not be src"):
        lib.take_rows(src, slot, out=src)
    packed = torch.zeros(ct.packed_floats(128))
    x, d = torch.zeros((2, 5, 384)), torch.zeros((2, 5, 128))
    for bad in ((x[..., :100], d), (x, d[..., :64]), (x, d[:1]), (x.double(), d), (x, torch.zeros((2, 5, 256)))):
        with pytest.raises(ValueError):
            lib.confidence_rows(*bad, packed)
    with pytest.raises(ValueError, match="fits no supported"):
        lib.confidence_rows(x, d, packed[:-4])
    feat, kp = torch.zeros((2, 4, 4, 384)), torch.zeros((2, 5, 2))
    for bad in ((feat[:, :, :3], kp, d), (feat, kp[:1], d), (feat, kp, d[:, :4]), (torch.zeros((2, 1, 1, 384)), kp, d), (feat, kp.double(), d)):
        with pytest.raises(ValueError):
            lib.gather_confidence(*bad, packed)
    with pytest.raises(ValueError, match="CUDA"):          # everything well-formed, but on the host: refused by the device check
        lib.confidence_filter(conf, 0.5)


def test_pipeline_refuses_confidence_without_a_head_or_in_bf16():
    import synth
    from sslam_amd.pipeline import ExtractorConfig, PackedConfidence, SequencePipeline
    assert ExtractorConfig().confidence is False
    assert "confidence_state" == list(inspect.signature(SequencePipeline.__init__).parameters)[-1]
    assert inspect.signature(SequencePipeline.__init__).parameters["confidence_state"].default is None
    ssd, rsd = synth.selector_state(0), synth.refiner_state(0)
    with pytest.raises(ValueError, match="confidence_state"):
        SequencePipeline(ExtractorConfig(confidence=True), ssd, rsd, device="cpu")
    with pytest.raises(ValueError, match="bf16"):
        SequencePipeline(ExtractorConfig(confidence=True, precision="bf16"), ssd, rsd, device="cpu", confidence_state=cases.head_state("default"))
    with pytest.raises(ValueError, match="width 256"):     # the packed buffers are host arrays moved to `device`: "cpu" serves here
        SequencePipeline(ExtractorConfig(confidence=True), ssd, rsd, device="cpu", confidence_state=cases.head_state("wide"))
    assert PackedConfidence.supported(384, 128, 128) and not PackedConfidence.supported(384, 128, 256)
