"""The validation stage as far as a machine without a GPU sees it: the float64 statement tests/val_ref.py and the host
composition sslam_amd.validation.compose against the reference-held values of tests/golden/val_losses.npz; the new entries
against the header, the built library and sslam_amd.lib; the argument errors, which come before any device work.

One tolerance rule for every scalar (val_ref.tolerance): |x - ref64| <= max(4 |ref32 - ref64|, 2^-20 max(1, |ref64|))."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import val_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sslam_row_lse", "sslam_row_lse_pairs", "sslam_edge_pool", "sslam_val_frame_stats", "sslam_val_pair_stats",
               "sslam_val_pair_stats_pairs")
E_INVALID, E_UNSUPPORTED = -1, -2
GOOD, GOOD2, ODD = 0x10000, 0x20000, 0x10004      # never dereferenced: every call below is refused before the launch


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "val_losses.npz"))


def _assert_rule(got: dict, order, ref32, ref64, what):
    for k, r32, r64 in zip(order, ref32, ref64):
        tol = val_ref.tolerance(r64, r32)
        print(f"{what} {k:20s} got {got[k]:+.9e} ref64 {r64:+.9e} |d| {abs(got[k] - r64):.2e} tol {tol:.2e}")
        assert abs(got[k] - r64) <= tol, (what, k, got[k], r64, tol)


@pytest.mark.parametrize("name", ["g4", "g5"])
def test_val_ref_and_compose_reproduce_the_reference(golden, name):
    from sslam_amd import validation
    c = val_ref.golden_case(golden, name)
    order = c["order"]
    assert tuple(order) == validation.TERMS + ("total",) + validation.METRICS
    assert float(golden[f"{name}_min_gap"]) > 1e-4, "tie-free in both arg-max directions"
    stats = val_ref.stats_dict(c["saliency"], c["images"], c["desc"], c["first"], c["second"], c["temperature"])
    assert np.array_equal(stats["n_matches"], golden[f"{name}_counts"])
    assert len(set(stats["n_matches"].tolist())) > 1, "the padding of the match lists is exercised"
    # B = 4: the float64 statement directly, and compose on the float64 statistics
    f, s = c["first"], c["second"]
    direct = val_ref.batch_terms(c["saliency"][f], c["saliency"][s], c["images"][f], c["desc"][f], c["desc"][s], c["temperature"])
    _assert_rule(direct, order, golden[f"{name}_ref32_b4"], golden[f"{name}_ref64_b4"], f"{name} B=4 val_ref")
    comp = validation.compose(stats, batch=4)
    _assert_rule({k: float(v[0]) for k, v in comp.items()}, order, golden[f"{name}_ref32_b4"], golden[f"{name}_ref64_b4"],
                 f"{name} B=4 compose")
    # B = 1: per-pair values
    comp1 = validation.compose(stats, batch=1)
    for b in range(4):
        _assert_rule({k: float(v[b]) for k, v in comp1.items()}, order, golden[f"{name}_ref32_b1"][b], golden[f"{name}_ref64_b1"][b],
                     f"{name} B=1 pair {b} compose")
    # the mean over batches, a short last batch kept: 3 + 1 pairs
    red = validation.reduce_batches(stats, batch=3)
    three = validation.compose({**stats, **{k: stats[k][:3] for k in ("first", "second", "repeat", "n_matches", "ce_sum", "pad_ce")}}, 3)
    for k in order:
        assert red[k] == pytest.approx((float(three[k][0]) + float(comp1[k][3])) / 2.0, rel=0, abs=1e-15 * max(1.0, abs(red[k])))
    assert set(red) == set(order)


def test_the_clamp_is_active_in_the_cold_case(golden):
    c = val_ref.golden_case(golden, "g4")
    raw = val_ref.f64(c["desc"][0]) @ val_ref.f64(c["desc"][4]).T / c["temperature"]
    assert c["temperature"] == 0.01 and (raw > 50).any() and (val_ref.logits(c["desc"][0], c["desc"][4], 0.01) == 50.0).any()


def test_defaults_are_the_reference_configuration():
    from sslam_amd import validation
    assert validation.WEIGHTS == dict(desc=8.0, repeat=0.3, variance=0.5, peakiness=0.1, activation=0.05, edge=0.3, sparsity=0.3)
    assert validation.TEMPERATURE == 0.10 and validation.BATCH == 4
    assert validation.TARGETS["peakiness_variance"] == 0.22 and validation.TARGETS["activation_mean"] == 0.35
    assert validation.TARGETS["min_variance"] == 0.005 and validation.TARGETS["sparsity_penalty"] == 2.0
    assert validation.WEIGHTS == val_ref.WEIGHTS


def test_constant_saliency_gives_zero_correlation_not_nan(golden):
    from sslam_amd import validation
    c = val_ref.golden_case(golden, "g5")
    sal = c["saliency"].copy()
    sal[:4] = np.float32(0.4)
    stats = val_ref.stats_dict(sal, c["images"], c["desc"], c["first"], c["second"], c["temperature"])
    out = validation.compose(stats, batch=4)
    assert out["edge"][0] == 0.0 and np.isfinite(out["total"][0])


def test_new_entries_are_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sslam_hip.h")).read()
    so = ctypes.CDLL(lib.SO_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, flags=re.M), f"{name} is not declared in include/sslam_hip.h"
        assert name in lib.EXPORTS
        assert hasattr(so, name), f"{name} is not exported by the library"
    L = lib.lib()
    assert L.sslam_version() > 500, "a new entry raises the version"
    for k, v in lib.VAL_FRAME_SLOTS.items():
        assert re.search(rf"#define SSLAM_VAL_{k.upper()} {v}\b", hdr), k
    for k, v in lib.VAL_PAIR_SLOTS.items():
        assert re.search(rf"#define SSLAM_VAL_PAIR_{k.upper()} {v}\b", hdr), k
    assert re.search(rf"#define SSLAM_VAL_FRAME_STATS {lib.VAL_FRAME_STATS}\b", hdr)
    assert re.search(rf"#define SSLAM_VAL_PAIR_STATS {lib.VAL_PAIR_STATS}\b", hdr)


def test_c_entries_refuse_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    f = ctypes.c_float
    before = lib.launch_count()

    def lse(d1=GOOD, s1=512, n1=4, d2=GOOD, s2=512, n2=4, n_pairs=2, s12=GOOD, t=0.1, lse=GOOD, ce=GOOD, s00=GOOD):
        return L.sslam_row_lse(d1, s1, n1, d2, s2, n2, n_pairs, s12, f(t), lse, ce, s00, None)

    def lsep(bank=GOOD, stride=512, n_bank=4, K=4, first=GOOD2, second=GOOD2, n_pairs=2, s12=GOOD, t=0.1, lse=GOOD, ce=GOOD, s00=GOOD):
        return L.sslam_row_lse_pairs(bank, stride, n_bank, K, first, second, n_pairs, s12, f(t), lse, ce, s00, None)

    for kw in (dict(d1=None), dict(d2=None), dict(s12=None), dict(lse=None, ce=None), dict(n1=0), dict(n2=0), dict(n_pairs=0),
               dict(t=0.0), dict(t=-1.0), dict(t=float("inf")), dict(t=float("nan")), dict(d1=ODD), dict(s1=510), dict(s2=2)):
        assert lse(**kw) == E_INVALID, kw
    for kw in (dict(bank=None), dict(first=None), dict(second=None), dict(s12=None), dict(lse=None, ce=None), dict(n_bank=0), dict(K=0),
               dict(n_pairs=-1), dict(t=0.0), dict(bank=ODD), dict(stride=6), dict(first=GOOD2 + 2), dict(second=GOOD2 + 1)):
        assert lsep(**kw) == E_INVALID, kw
    assert L.sslam_edge_pool(None, 1, 64, GOOD, GOOD, None) == E_INVALID
    assert L.sslam_edge_pool(GOOD, 1, 64, None, GOOD, None) == E_INVALID
    assert L.sslam_edge_pool(GOOD, 1, 64, GOOD, None, None) == E_INVALID
    assert L.sslam_edge_pool(GOOD, 0, 64, GOOD, GOOD, None) == E_INVALID
    assert L.sslam_edge_pool(ODD, 1, 64, GOOD, GOOD, None) == E_INVALID
    assert L.sslam_edge_pool(GOOD, 1, 70, GOOD, GOOD, None) == E_UNSUPPORTED
    assert L.sslam_val_frame_stats(None, None, None, None, 1, 4, 0, GOOD, None, None, None) == E_INVALID
    assert L.sslam_val_frame_stats(GOOD, GOOD, None, None, 1, 4, 0, GOOD, None, None, None) == E_INVALID
    assert L.sslam_val_frame_stats(GOOD, None, None, GOOD, 1, 4, 4, GOOD, None, GOOD, None) == E_INVALID
    assert L.sslam_val_frame_stats(GOOD, None, None, None, 1, 0, 0, GOOD, None, None, None) == E_INVALID
    assert L.sslam_val_pair_stats(GOOD, None, 4, GOOD, GOOD, GOOD, GOOD, GOOD, 4, 4, 1, f(0.1), GOOD, GOOD, None) == E_INVALID
    assert L.sslam_val_pair_stats(GOOD, GOOD, 4, GOOD, GOOD, GOOD, None, GOOD, 4, 4, 1, f(0.1), GOOD, GOOD, None) == E_INVALID
    assert L.sslam_val_pair_stats(GOOD, GOOD, 4, GOOD, GOOD, GOOD, GOOD, GOOD, 4, 4, 1, f(0.0), GOOD, GOOD, None) == E_INVALID
    assert L.sslam_val_pair_stats_pairs(GOOD, 4, 3, None, GOOD2, GOOD, GOOD, GOOD, GOOD, GOOD, 4, 1, f(0.1), GOOD, GOOD, None) == E_INVALID
    assert L.sslam_val_pair_stats_pairs(GOOD, 4, 3, GOOD2 + 2, GOOD2, GOOD, GOOD, GOOD, GOOD, GOOD, 4, 1, f(0.1), GOOD, GOOD, None) == E_INVALID
    assert L.sslam_val_pair_stats_pairs(GOOD, 4, 0, GOOD2, GOOD2, GOOD, GOOD, GOOD, GOOD, GOOD, 4, 1, f(0.1), GOOD, GOOD, None) == E_INVALID
    assert lib.launch_count() == before, "a refused call launches nothing"


def test_compose_refuses_bad_batches(golden):
    from sslam_amd import validation
    c = val_ref.golden_case(golden, "g5")
    stats = val_ref.stats_dict(c["saliency"], c["images"], c["desc"], c["first"], c["second"], c["temperature"])
    with pytest.raises(ValueError, match="ragged"):
        validation.compose(stats, batch=3)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="batch"):
            validation.compose(stats, batch=bad)
        with pytest.raises(ValueError, match="batch"):
            validation.reduce_batches(stats, batch=bad)
    absent = dict(stats, second=np.array([4, -1, 6, 7], np.int32))
    with pytest.raises(ValueError, match="absent"):
        validation.compose(absent, batch=4)
    with pytest.raises(ValueError, match="stats lack"):
        validation.compose({k: v for k, v in stats.items() if k != "ce_sum"}, batch=4)


def test_validation_stats_checks_its_arguments_before_any_device_work():
    from sslam_amd import lib
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    pipe = SequencePipeline.__new__(SequencePipeline)          # no packing, no device: the checks come first
    pipe.cfg = ExtractorConfig(input_size=64, num_keypoints=4)
    out = dict(saliency=torch.zeros((3, 4, 4)), descriptors=torch.zeros((3, 4, lib.D_OUT)))
    img = torch.zeros((3, 48, 64, 3), dtype=torch.uint8)
    before = lib.launch_count()
    i64 = torch.tensor([0, 1], dtype=torch.int64)
    with pytest.raises(ValueError, match="int32"):
        pipe.validation_stats(out, img, first=i64, second=i64)
    with pytest.raises(ValueError, match="32-bit integers"):
        pipe.validation_stats(out, img, first=[0.5, 1.0], second=[1, 2])
    with pytest.raises(ValueError, match="unequal"):
        pipe.validation_stats(out, img, first=[0, 1], second=[1])
    with pytest.raises(ValueError, match="both pair lists"):
        pipe.validation_stats(out, img, first=[0, 1])
    with pytest.raises(ValueError, match="not both"):
        pipe.validation_stats(out, img, spacing=1, first=[0], second=[1])
    for sp in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="spacing"):
            pipe.validation_stats(out, img, spacing=sp)
    with pytest.raises(ValueError, match="no pair"):
        pipe.validation_stats(out, img, spacing=3)
    for t in (0.0, -0.1, float("nan"), float("inf"), "0.1", None):
        with pytest.raises(ValueError, match="temperature"):
            pipe.validation_stats(out, img, temperature=t)
    with pytest.raises(ValueError, match="images"):
        pipe.validation_stats(out, img[:2])
    with pytest.raises(ValueError, match="images"):
        pipe.validation_stats(out, torch.zeros((3, 3, 32, 32)))
    with pytest.raises(ValueError, match="saliency"):
        pipe.validation_stats(dict(out, saliency=torch.zeros((3, 5, 5))), img)
    assert lib.launch_count() == before


def test_bindings_check_shapes_before_any_device_work():
    from sslam_amd import lib
    bank = torch.zeros((3, 4, lib.D_OUT))
    i32 = torch.tensor([0, 1], dtype=torch.int32)
    before = lib.launch_count()
    with pytest.raises(ValueError, match="int32"):
        lib.row_lse_pairs(bank, i32.long(), i32, torch.zeros((2, 4)))
    with pytest.raises(ValueError, match="s12"):
        lib.row_lse_pairs(bank, i32, i32, torch.zeros((2, 5)))
    with pytest.raises(ValueError, match="s12"):
        lib.row_lse(bank, 512, 4, bank, 512, 4, 2, torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="temperature"):
        lib.row_lse_pairs(bank, i32, i32, torch.zeros((2, 4)), temperature=0)
    with pytest.raises(ValueError, match="images"):
        lib.edge_pool(torch.zeros((1, 3, 24, 24)))
    with pytest.raises(ValueError, match="images"):
        lib.edge_pool(torch.zeros((1, 3, 32, 32), dtype=torch.float64))
    with pytest.raises(ValueError, match="pooled"):
        lib.edge_pool(torch.zeros((1, 3, 32, 32)), out=(torch.zeros((1, 3, 2)), torch.zeros((1,))))
    with pytest.raises(ValueError, match="together"):
        lib.val_frame_stats(torch.zeros((2, 4, 4)), pooled=torch.zeros((2, 4, 4)))
    with pytest.raises(ValueError, match="descriptors"):
        lib.val_frame_stats(torch.zeros((2, 4, 4)), descriptors=torch.zeros((3, 4, lib.D_OUT)))
    nn = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="ce"):
        lib.val_pair_stats(torch.zeros((2, 4, 4)), torch.zeros((2, 4, 4)), nn, nn, nn.float(), None, torch.zeros((2,)))
    with pytest.raises(ValueError, match="s00"):
        lib.val_pair_stats_pairs(torch.zeros((3, 4, 4)), i32, i32, nn, nn, nn.float(), nn.float(), torch.zeros((3,)))
    assert lib.launch_count() == before
