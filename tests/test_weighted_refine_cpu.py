"""CPU tests of confidence-weighted pose refinement: the interface of libsslam_weight.so (include/sslam_weight.h,
sslam_amd.lib.WEIGHT_EXPORTS and tests/weight_table.py hold the same entries; the built library's symbols are
tests/test_libraries_cpu.py), the seeded cases of tests/weighted_refine_cases.py against their margins, the restatement of
tests/weighted_refine_ref.py against an independent implementation and a finite-difference gradient, the two invariants of the
header on the restatement, the value type and the refusals of the Python layers, the numpy drop-ins, everything the C entries
refuse before any device work, and the planted study that says what a calibrated weight buys.  No GPU."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import pose_ransac_ref as rr
import pose_refine_cases as pc
import pose_refine_ref as fr
import weight_table as wt
import weighted_refine_cases as cases
import weighted_refine_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sslam_weight.h")
E_INVALID, E_UNSUPPORTED = -1, -2
P = [0x10000 * (i + 1) for i in range(24)]       # never dereferenced: every call below is refused before the launch


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300))


# ------------------------------------------------------------------------------------------------------------- the interface
def test_entries_are_declared_exported_and_listed():
    """The table, the constants and the key lists against the export list; that list against the header and the built library is
    tests/test_libraries_cpu.py."""
    from sslam_amd import lib
    declared = lib.WEIGHT_EXPORTS
    assert set(wt.ALIGN) | set(wt.HOST_ONLY) == set(declared) and not set(wt.ALIGN) & set(wt.HOST_ONLY) and set(wt.LIMITS) == set(wt.ALIGN)
    L = lib.weight()
    consts = {k: int(v) for k, v in re.findall(r"#define (SSLU_\w+) (\d+)\s", open(HEADER).read())}
    assert consts == dict(SSLU_WEIGHT_PRODUCT=wt.WEIGHT_PRODUCT, SSLU_WEIGHT_EXPECTED_ERROR=wt.WEIGHT_EXPECTED_ERROR)
    assert (lib.WEIGHT_PRODUCT, lib.WEIGHT_EXPECTED_ERROR) == (wt.WEIGHT_PRODUCT, wt.WEIGHT_EXPECTED_ERROR) == (wr.PRODUCT, wr.EXPECTED_ERROR)
    assert lib.POSE_REFINE_WEIGHTED_KEYS == wr.KEYS == lib.POSE_REFINE_KEYS + ("weight_sum",)
    assert len(L.sslu_pose_refine_weighted_pairs.argtypes) == len(lib.lib().sslam_pose_refine_pairs.argtypes) + 2 == 38
    assert len(L.sslu_match_weights.argtypes) == 13
    import torch
    sh = lib.pose_refine_weighted_shapes(3, 7)
    assert sh["weight_sum"] == ((3,), torch.float64) and {k: v for k, v in sh.items() if k != "weight_sum"} == lib.pose_refine_shapes(3, 7)


def test_the_header_states_both_tables_line_for_line():
    elem = {"int32_t": 4, "float": 4, "double": 8, "int64_t": 8}
    for entry, row in wt.ALIGN.items():
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*?)\)\s*;", _header())
        assert m, entry
        args = [re.match(r"(.*?)(\w+)$", " ".join(a.split())).groups() for a in m.group(1).split(",")]
        pointers = [(t.strip(), n) for t, n in args if "*" in t and n != "stream"]
        assert [n for _, n in pointers] == list(row), entry
        for t, n in pointers:
            e = elem[t.replace("const", "").replace("*", "").strip()]
            assert row[n] == (8 if n == "kp_bank" else e), (entry, n)          # kp_bank is read as float2
    raw = open(HEADER).read()
    for title, lines in (("ALIGNMENT, every entry", wt.header_lines()), ("SIZE LIMITS: the expressions", wt.limit_lines())):
        start = raw.index(title)
        stated = re.sub(r"\n \*\s+", " ", raw[start:raw.index("*/", start)]).strip()
        for line in lines:
            assert line + " " in stated + " ", f"include/sslam_weight.h does not state: {line}"
        assert len(re.findall(r"\bsslu_\w+: ", stated)) == len(wt.ALIGN)
    joined = re.sub(r"\n \*\s+", " ", raw)
    for text in ("EVERY element of weight is written", "w = c1 * c2", "e = 1.0 / ((double)c + 1e-6) - 1.0", "w = s2 / ((s2 + e1*e1) + e2*e2), rounded once to fp32",
                 "No transcendental function", "g > 0 && g - g == 0", "gw = (double)g * w", "cost += (double)g * rho",
                 "H_ij += gw * (Ju[i]*Ju[j] + Jv[i]*Jv[j])", "g_i += gw * (Ju[i]*rx + Jv[i]*ry)", "Huber acts on the raw residual",
                 "weight_sum = the sum of (double)g over the selected rows", "its inlier count over ALL usable rows >= inlier_count_in",
                 "With every weight exactly 1.0f", "Scaling every weight by a power of two", "every refusal comes before anything is launched and writes nothing",
                 "Fewer than 3 selected rows: status 3", "45968 bytes static"):
        assert text in joined, text
    # the sums, the solve and the update are stated once, in sslam_hip.h, and compiled from one header into both kernels
    from sslam_amd import lib
    shared = os.path.join(lib.CSRC, "pose_refine_common.h")
    body = open(shared).read()
    for name in ("refine_h", "refine_terms", "refine_solve", "refine_update", "pose_refine_body"):
        assert re.search(r"\b" + name + r"\s*\(", body), name
    for src in (os.path.join(lib.CSRC, "pose_refine.hip"), os.path.join(lib.LIBRARIES["weight"].csrc, "weighted_refine.hip")):
        text = open(src).read()
        assert "pose_refine_common.h" in text and "refine_solve" not in text and "refine_update" not in text and "LDL" not in text.split("#include")[1], src
    assert shared in lib.LIBRARIES["weight"].prerequisites      # and the first library's objects depend on every header of its directory
    # the LDS arithmetic: 4 KB of weights beside the chunk, under the 64 KB a workgroup can name statically
    assert wt.static_lds_bytes(False) == 41872 and wt.static_lds_bytes(True) == 45968 == wt.static_lds_bytes(False) + 4 * wt.CHUNK
    assert wt.static_lds_bytes(True) <= 64 * 1024
    assert wt.MAX_K == lib.EVAL_MAX_K and wt.MAX_K // wt.THREADS <= 32, "a thread's selected rows fit one 32-bit register"


# ------------------------------------------------------------------------------------------------------------- the case lists
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_cases_keep_their_margins(name, kind):
    m = cases.margins(name, kind)
    print(f"{name} / {kind}: " + ", ".join(f"{key} {v:.3e}" for key, v in m.items()))
    assert cases.margins_ok(m), (name, kind, m)
    w = cases.weights(name, kind)
    c = pc.case(name)
    assert w.dtype == np.float32 and w.shape == c["matches"].shape[:2] and not w.flags.writeable


@pytest.mark.parametrize("name,override", cases.VARIATIONS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in o.items())}" for n, o in cases.VARIATIONS])
def test_variations_keep_their_margins(name, override):
    """Every decision but the cost comparison of a converged iteration (pose_refine_cases' docstring says why that one cannot)."""
    m = cases.check_margins(pc.case(name), cases.weights(name, "random"), with_cost=False, **override)
    print(f"{name} {override}: " + ", ".join(f"{key} {v:.3e}" for key, v in m.items()))
    assert cases.margins_ok(m), (name, override, m)


def test_case_list_covers_what_it_must():
    status, past_chunk, starved, unselected = set(), 0, 0, 0
    for name in cases.NAMES:
        c = pc.case(name)
        for kind in cases.KINDS:
            e = cases.expected(name, kind)
            status |= set(e["status"].tolist())
            live = e["status"] != 3
            assert (e["selected_count"][live] <= e["inlier_count_in"][live]).all() and (e["inlier_count_in"][live] <= e["usable_count"][live]).all()
            unselected += int((e["selected_count"][live] < e["inlier_count_in"][live]).sum())
            past_chunk += int((e["usable_count"] > wt.CHUNK).sum())
        w = cases.weights(name, "bad")
        if w.size >= 64:
            assert np.isnan(w).any() and np.isposinf(w).any() and np.isneginf(w).any() and (w == -1).any()
            assert (np.signbit(w) & (w == 0)).any() and ((w > 0) & (w < np.finfo(np.float32).tiny)).any(), "-0.0 and a subnormal"
        if name == "k3" or name.startswith("k64_p70"):
            h, o = cases.expected(name, "holes"), cases.expected(name, "ones")
            rows = range(len(h["status"])) if name == "k3" else [cases.STARVED_PAIR]
            for p in rows:
                assert h["status"][p] == 3 and h["weight_sum"][p] == 0
                starved += int(o["status"][p] != 3)
    assert status == {0, 1, 2, 3} and past_chunk >= 8 and unselected >= 50
    assert starved >= 3, "pairs the unweighted entry refines and the holes leave under 3 selected rows"
    for kind in ("conf_product", "conf_expected"):
        bank = cases.confidence_bank(pc.case("k64_p70"), 1)
        assert (bank == 0).any() and (bank == 1).any() and (bank == cases.CONF_MIN).any()
        assert (bank == np.nextafter(cases.CONF_MIN, np.float32(0))).any() and (bank == np.nextafter(cases.CONF_MIN, np.float32(1))).any()


# ------------------------------------------------------------------------------------------- the restatement and its invariants
def test_all_ones_is_the_unweighted_restatement_byte_for_byte():
    for name in cases.NAMES:
        w, u = cases.expected(name, "ones"), pc.expected(name)
        for key in fr.KEYS:
            assert w[key].dtype == u[key].dtype and w[key].tobytes() == u[key].tobytes(), (name, key)
        assert np.array_equal(w["weight_sum"], w["selected_count"].astype(np.float64))
    for name, o in cases.VARIATIONS:
        c = pc.case(name)
        w = wr.stacked(cases.run(c, cases.weights(name, "ones"), **o))
        u = pc.expected(name, tuple(o.items()))
        assert all(w[key].tobytes() == u[key].tobytes() for key in fr.KEYS), (name, o)


def test_power_of_two_scaling_is_exact():
    for name in cases.NAMES:
        base = cases.expected(name, "random")
        assert np.array_equal(cases.weights(name, "quarter"), cases.weights(name, "random") * np.float32(0.25))
        assert np.array_equal(cases.weights(name, "eight"), cases.weights(name, "random") * np.float32(8))
        for kind, f in (("quarter", 0.25), ("eight", 8.0)):
            e = cases.expected(name, kind)
            for key in wr.KEYS:
                if key in wr.SCALED:
                    assert (e[key] == base[key] * f).all(), (name, kind, key)
                else:
                    assert e[key].tobytes() == base[key].tobytes(), (name, kind, key)


def _rows_of(r):
    return r["rows"]["Xa"][r["selected"]], r["rows"]["kb"][r["selected"]], r["row_weight"][r["selected"]].astype(np.float64)


def test_restatement_equals_the_independent_implementation():
    """T, cost and info to 1e-9 relative in the maximum norm of each quantity, the status and the accepted steps equal: the bars
    tests/test_pose_refine_cpu.py holds the unweighted pair to, with its exemption for singular pairs."""
    worst, n = dict(T=0.0, cost=0.0, info=0.0), 0
    for name in cases.NAMES:
        c = pc.case(name)
        for kind in ("random", "bad", "conf_expected"):
            w = cases.weights(name, kind)
            for p, r in enumerate(cases.run(c, w, detail=True)):
                if r["status"] == 3:
                    continue
                Xa, kb, g = _rows_of(r)
                T, cost_in, cost, H, accepted = wr.plain_weighted_refine(Xa, kb, g, c["cam"], c["scale_x"], c["scale_y"], c["huber"], c["n_iter"], c["T_in"][p])
                if c["singular"][p] or cases.singular(c, w, p):
                    # no pose is determined: the last pivots are rounding noise around 0 (under some weights one comes out positive and
                    # a step is taken, which the unweighted lists never meet); the independent H says why nothing is compared here
                    assert np.linalg.matrix_rank(H) < 6, (name, kind, p)
                    continue
                assert accepted == r["iterations"], (name, kind, p, accepted, r["iterations"])
                if r["status"] == 2:
                    T, cost = c["T_in"][p], cost_in
                    H = wr.plain_weighted_normal_equations(c["T_in"][p], Xa, kb, g, c["cam"], c["scale_x"], c["scale_y"], c["huber"])[1]
                e = dict(T=_rel(r["T"], T), cost=_rel([r["cost_in"], r["cost"]], [cost_in, cost]), info=_rel(fr.full_info(r["info"]), H))
                worst = {key: max(worst[key], e[key]) for key in worst}
                n += 1
                assert max(e.values()) <= 1e-9, (name, kind, p, e)
                assert abs(r["weight_sum"] - g.sum()) <= 1e-12 * g.sum()
    print(f"{n} pairs: largest relative difference " + ", ".join(f"{key} {v:.2e}" for key, v in worst.items()))
    assert n >= 300


def test_gradient_equals_the_finite_difference_of_half_the_weighted_cost():
    n = 0
    for name in ("k64_p70_prior", "k64_p70_identity", "k64_loose", "k300_n257"):
        c = pc.case(name)
        for p, r in enumerate(cases.run(c, cases.weights(name, "random"), detail=True, n_iter=0)):
            if r["status"] == 3:
                continue
            Xa, kb, g = _rows_of(r)
            fd = wr.finite_difference_gradient(c["T_in"][p], Xa, kb, g, c["cam"], c["scale_x"], c["scale_y"], c["huber"])
            assert _rel(r["g"], fd) <= 1e-6, (name, p, r["g"], fd)
            n += 1
    assert n >= 100


# ------------------------------------------------------------------------------------------------------------ match weights
def test_match_weights_restatement_at_its_edges():
    f = np.float32
    tiny = cases.CONF_MIN
    c = np.array([0.0, 1.0, tiny, np.nextafter(tiny, f(0)), np.nextafter(tiny, f(1)), 0.5, np.nan], f)
    prod = wr.weight_of(c, c, wr.PRODUCT)
    assert prod.dtype == f and prod[0] == 0 and prod[1] == 1 and prod[2] == 0 and prod[5] == f(0.25) and np.isnan(prod[6])
    assert wr.weight_of(f(1), f(1), wr.PRODUCT) == 1 and wr.weight_of(tiny, tiny, wr.PRODUCT) == 0
    ee = wr.weight_of(c, np.full_like(c, 1.0), wr.EXPECTED_ERROR, 0.5)
    e1 = 1.0 / (1.0 + 1e-6) - 1.0                      # a confidence of exactly 1 reads as an error of -1e-6: squared, nothing
    assert ee[1] == f(0.25 / ((0.25 + e1 * e1) + e1 * e1)) and ee[1] == 1
    assert 0 < ee[0] < 1e-12 and 0 < ee[2] < 1e-12 and np.isnan(ee[6]) and not wr.weight_ok(ee[6])
    e = 1.0 / (0.5 + 1e-6) - 1.0
    assert ee[5] == f(0.25 / ((0.25 + e * e) + e1 * e1))
    assert wr.weight_ok(np.array([1e-41, 1.0, 3e38], f)).all()
    assert not wr.weight_ok(np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan], f)).any()
    for shape in ("k1", "k300_n257", "k4096"):
        s = cases.weight_case(shape)
        for mode in (wr.PRODUCT, wr.EXPECTED_ERROR):
            w = wr.match_weights(s["conf"], s["first"], s["second"], s["matches"], s["count"], mode, 0.7)
            assert w.shape == s["matches"].shape[:2] and w.dtype == f
            for p in range(len(w)):
                live = 0 <= s["first"][p] < s["n_bank"] and 0 <= s["second"][p] < s["n_bank"]
                cnt = int(np.clip(s["count"][p], 0, s["n1"])) if live else 0
                assert (w[p, cnt:].view(np.uint32) == 0).all(), "+0.0 past the count and on an absent pair"
                bad = (s["matches"][p, :cnt] < 0).any(axis=1) | (s["matches"][p, :cnt] >= s["K"]).any(axis=1)
                assert (w[p, :cnt][bad].view(np.uint32) == 0).all()


def test_dropin_match_weights_equals_the_restatement():
    import evaluation as ev
    rng = np.random.default_rng(5)
    c1, c2 = cases.confidence_bank(pc.case("k64_p70"), 3)[:2]
    mt = rng.integers(-1, 65, (200, 2)).astype(np.int64)
    for mode, name in ((wr.PRODUCT, "product"), (wr.EXPECTED_ERROR, "expected_error")):
        got = ev.match_weights(c1, c2, mt, name, 0.3)
        want = wr.match_weights(np.stack([c1, c2]), [0], [1], mt[None], [len(mt)], mode, 0.3)[0]
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), name
    assert ev.match_weights(c1, c2, np.zeros((0, 2), np.int64)).shape == (0,)
    for bad in (dict(mode="sum"), dict(mode="expected_error", sigma0=0.0), dict(mode="expected_error", sigma0=float("nan"))):
        with pytest.raises(ValueError):
            ev.match_weights(c1, c2, mt, **bad)
    with pytest.raises(ValueError):
        ev.match_weights(c1[None], c2, mt)
    with pytest.raises(ValueError):
        ev.match_weights(c1, c2, mt.astype(np.float32))
    assert list(inspect.signature(ev.refine_relative_pose).parameters)[-1] == "weights"
    assert inspect.signature(ev.refine_relative_pose).parameters["weights"].default is None
    with pytest.raises(ValueError, match="weights"):
        ev.refine_relative_pose(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), None, None, mt[:3], np.eye(4), weights=np.ones(2, np.float32))
    with pytest.raises(ValueError, match="weights"):
        ev.refine_relative_pose(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), None, None, mt[:3], np.eye(4), weights=np.ones(3))


def test_dropin_refine_relative_pose_with_weights_equals_the_restatement_without_a_gpu(monkeypatch):
    import evaluation as dropin
    from sslam_amd import lib

    def boom():
        raise AssertionError("the weighted drop-in went to the device")
    monkeypatch.setattr(lib, "weight", boom)
    monkeypatch.setattr(lib, "lib", boom)
    import pose_ransac_cases as rc
    import pose_ransac_ref as rr
    c = rc.case("k300_n257")
    cam, p = c["cam"], 2
    a, b = c["first"][p], c["second"][p]
    imgs = np.zeros((2, cam.height, cam.width), np.uint16)      # depth images that hold every keypoint's depth under it (tests/test_gpu_pose_refine.py)
    px = np.floor(c["bank"][[a, b]].astype(np.float64) + 0.5).astype(np.int64)
    inside = (px[..., 0] >= 0) & (px[..., 0] < cam.width) & (px[..., 1] >= 0) & (px[..., 1] < cam.height)
    kd = np.where(inside & (c["depth_bank"][[a, b]] > 0), c["depth_bank"][[a, b]], 0)
    for f in range(2):
        order = np.arange(px.shape[1])[::-1]
        imgs[f, px[f, order, 1].clip(0, cam.height - 1), px[f, order, 0].clip(0, cam.width - 1)] = np.where(inside[f, order], kd[f, order], 0)
    seen = np.stack([np.where(inside[f], imgs[f, px[f, :, 1].clip(0, cam.height - 1), px[f, :, 0].clip(0, cam.width - 1)].astype(np.int32), -1)
                     for f in range(2)])
    cnt = int(np.clip(c["count"][p], 0, c["n1"]))
    mt = c["matches"][p][:cnt]
    start = rr.ransac(c["bank"][a], c["bank"][b], seen[0], seen[1], mt, cnt, cam, 3.0, 128, 9)["T"]
    conf = cases.confidence_bank(dict(bank=c["bank"][[a, b]]), 11)
    for mode, name in ((wr.PRODUCT, "product"), (wr.EXPECTED_ERROR, "expected_error")):
        w = dropin.match_weights(conf[0], conf[1], mt, name, 0.5)
        assert w.tobytes() == wr.match_weights(conf, [0], [1], mt[None], [cnt], mode, 0.5)[0].tobytes()
        want = wr.refine(c["bank"][a], c["bank"][b], seen[0], seen[1], mt, cnt, w, cam, 3.0, 1.0, 5, start)
        T4 = np.eye(4)
        T4[:3] = start.reshape(3, 4)
        Tm, mask, info = dropin.refine_relative_pose(c["bank"][a], c["bank"][b], imgs[0], imgs[1], mt, T4, cam, 3.0, None, 5, weights=w)
        assert Tm[:3].tobytes() == want["T"].reshape(3, 4).tobytes() and np.array_equal(mask, want["inlier_of_slot"] == 1)
        assert info.tobytes() == fr.full_info(want["info"]).tobytes() and want["status"] == 0
        assert want["selected_count"] < want["inlier_count_in"] if mode == wr.PRODUCT else want["selected_count"] == want["inlier_count_in"], \
            "a confidence of exactly 0 gives a product of 0, which is not selected, and a tiny positive expected-error weight, which is"


def test_package_numpy_statement_equals_the_restatement_pair_by_pair():
    """sslam_amd/weight_numpy.py, which the drop-ins run, against tests/weighted_refine_ref.py on every present pair of two 70-pair
    lists (unit scale) under weights with NaN, infinities, zeros, negatives and subnormals: every output, bit for bit."""
    from sslam_amd import weight_numpy as wn
    seen = set()
    for name in ("k64_p70", "k64_p70_identity", "k3"):
        c = pc.case(name)
        assert c["scale_x"] == 1.0 and c["scale_y"] == 1.0
        w = cases.weights(name, "bad")
        want = cases.expected(name, "bad")
        for p, (a, b) in enumerate(zip(c["first"], c["second"])):
            if not (0 <= a < len(c["bank"]) and 0 <= b < len(c["bank"])):
                continue
            cnt = int(np.clip(c["count"][p], 0, c["n1"]))
            if cnt == 0:
                continue
            got = wn.refine_pair(c["bank"][a], c["bank"][b], c["depth_bank"][a], c["depth_bank"][b], c["matches"][p][:cnt], w[p][:cnt], c["cam"],
                                 c["threshold"], c["huber"], c["n_iter"], c["T_in"][p])
            for key in wr.KEYS:
                full = np.asarray(want[key][p])
                full = full[:cnt] if key == "inlier_of_slot" else full
                assert np.asarray(got[key], dtype=full.dtype).tobytes() == full.tobytes(), (name, p, key)
            seen.add(int(got["status"]))
    assert seen >= {0, 2, 3}, seen
    img = np.arange(12, dtype=np.uint16).reshape(3, 4)
    kp = np.array([[0.4, 0.6], [3.49, 1.5], [3.5, 0], [-0.5, 0], [-0.51, 0], [np.nan, 1], [1e30, 1]], np.float32)
    assert wn.keypoint_depth(img, kp).tolist() == [4, 11, -1, 0, -1, -1, -1]


# ---------------------------------------------------------------------------------------------------------- the Python layers
def test_pose_weights_is_validated_like_a_match_rule():
    from sslam_amd import lib
    from sslam_amd.pipeline import PoseWeights
    assert PoseWeights.product() == PoseWeights(lib.WEIGHT_PRODUCT, 1.0) and PoseWeights.expected_error() == PoseWeights(lib.WEIGHT_EXPECTED_ERROR, 1.0)
    assert PoseWeights.expected_error(0.3).sigma0 == 0.3 and PoseWeights.expected_error(sigma0=2).mode == lib.WEIGHT_EXPECTED_ERROR
    for bad in ((2, 1.0), (-1, 1.0), (True, 1.0), ("product", 1.0), (0, 0.5), (1, 0.0), (1, -1.0), (1, float("nan")), (1, float("inf")), (1, "1"), (1, True)):
        with pytest.raises(ValueError):
            PoseWeights(*bad)
    with pytest.raises(Exception):
        PoseWeights.product().sigma0 = 2.0           # frozen
    assert lib.check_weights(0, "ignored") == (0, 1.0) and lib.check_weights(1, 0.25) == (1, 0.25)
    for bad in ((2, 1.0), (True, 1.0), ("0", 1.0), (1, 0.0), (1, float("inf")), (1, None), (None, 1.0)):
        with pytest.raises(ValueError):
            lib.check_weights(*bad)


def test_layers_refuse_before_any_device_work(monkeypatch):
    import torch
    from sslam_amd import lib, odometry, online
    from sslam_amd.pipeline import ExtractorConfig, PoseWeights, SequencePipeline

    def boom():
        raise AssertionError("the library was loaded before the arguments were judged")
    monkeypatch.setattr(lib, "weight", boom)
    plain = types.SimpleNamespace(cfg=ExtractorConfig())
    with_conf = types.SimpleNamespace(cfg=ExtractorConfig(confidence=True))
    img, depth = np.zeros((3, 8, 8, 3), np.uint8), np.zeros((3, 480, 640), np.uint16)
    w = PoseWeights.product()
    with pytest.raises(ValueError, match="confidence=True"):
        odometry.odometry(plain, img, depth, refine=True, weights=w)
    with pytest.raises(ValueError, match="refine=True"):
        odometry.odometry(with_conf, img, depth, weights=w)
    with pytest.raises(ValueError, match="PoseWeights"):
        odometry.odometry(with_conf, img, depth, refine=True, weights="product")
    with pytest.raises(ValueError, match="confidence=True"):
        odometry.odometry_graph(plain, img, depth, weights=w)
    with pytest.raises(ValueError, match="PoseWeights"):
        odometry.odometry_graph(with_conf, img, depth, weights=1.0)
    for pipe, kw, msg in ((plain, dict(refine=True, weights=w), "confidence=True"), (with_conf, dict(weights=w), "refine=True"),
                          (with_conf, dict(refine=True, weights=0), "PoseWeights")):
        with pytest.raises(ValueError, match=msg):
            online.PoseFrameStepper(pipe, 8, 8, 480, 640, **kw)
    for fn in (odometry.odometry, odometry.odometry_graph, online.PoseFrameStepper.__init__, SequencePipeline.refine_poses):
        assert inspect.signature(fn).parameters["weights"].default is None, fn
    assert inspect.signature(SequencePipeline.alloc_pose_refine).parameters["weighted"].default is False
    assert list(inspect.signature(SequencePipeline.match_weights).parameters) == ["self", "confidence", "first", "second", "matches", "weights", "out"]
    # the lib wrappers: every check before the library is loaded
    conf = torch.zeros((2, 5))
    first, second = torch.zeros(3, dtype=torch.int32), torch.ones(3, dtype=torch.int32)
    mt, cnt = torch.zeros((3, 4, 2), dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    for bad in ((conf.double(), first, second, mt, cnt), (conf[0], first, second, mt, cnt), (conf, first.long(), second, mt, cnt),
                (conf, first[:2], second, mt, cnt), (conf, first, second, mt.int(), cnt), (conf, first, second, mt[:2], cnt),
                (conf, first, second, mt, cnt.long()), (conf, first, second, mt, None), (conf, first, second, mt[..., 0], cnt)):
        with pytest.raises(ValueError):
            lib.match_weights(*bad)
    for kw in (dict(mode=2), dict(mode=1, sigma0=0.0), dict(mode=1, sigma0=float("nan")), dict(out=torch.zeros((3, 5))), dict(out=torch.zeros((3, 4)).double())):
        with pytest.raises(ValueError):
            lib.match_weights(conf, first, second, mt, cnt, **kw)
    with pytest.raises(ValueError, match="CUDA"):           # everything well-formed, but on the host: refused by the device check
        lib.match_weights(conf, first, second, mt, cnt)
    kp, kd = torch.zeros((2, 5, 2)), torch.zeros((2, 5), dtype=torch.int32)
    from sslam_amd.evaluation import Camera
    t_in = torch.zeros((3, 12), dtype=torch.float64)
    good = torch.ones((3, 4))
    for weights in (None, good.double(), good[:2], good[:, :3], good.t().contiguous().t(), good.numpy()):
        with pytest.raises(ValueError, match="weights"):
            lib.pose_refine_weighted(kp, kd, first, second, mt, cnt, Camera(), t_in, weights)
    with pytest.raises(ValueError, match="CUDA"):
        lib.pose_refine_weighted(kp, kd, first, second, mt, cnt, Camera(), t_in, good)
    with pytest.raises(ValueError, match="out must hold 13"):
        lib.pose_refine_weighted(kp, kd, first, second, mt, cnt, Camera(), t_in, good, out=(t_in,) * 12)


# -------------------------------------------------------------------------------------------------- refused before the device
def _weights_call(L, conf=P[0], n_bank=3, K=8, first=P[1], second=P[2], n_pairs=2, m=P[3], cnt=P[4], n1=8, mode=0, sigma0=1.0, weight=P[5]):
    return L.sslu_match_weights(conf, n_bank, K, first, second, n_pairs, m, cnt, n1, mode, ctypes.c_double(sigma0), weight, None)


def _refine_call(L, kp=P[0], kd=P[1], n_bank=3, K=8, first=P[2], second=P[3], n_pairs=2, m=P[4], cnt=P[5], n1=8, fx=525.0, fy=525.0, cx=319.5,
                 cy=239.5, ds=5000.0, sx=1.0, sy=1.0, vw=640.0, vh=480.0, thr=3.0, t_in=P[6], huber=1.0, n_iter=5, weight=P[19], T=P[7],
                 status=P[8], its=P[9], sel=P[10], use=P[11], inl_in=P[12], inl=P[13], mask=P[14], cost_in=P[15], cost=P[16], rms=P[17],
                 info=P[18], wsum=P[20]):
    return L.sslu_pose_refine_weighted_pairs(kp, kd, n_bank, K, first, second, n_pairs, m, cnt, n1,
                                             *(ctypes.c_double(v) for v in (fx, fy, cx, cy, ds, sx, sy, vw, vh, thr)), t_in, ctypes.c_double(huber),
                                             n_iter, weight, T, status, its, sel, use, inl_in, inl, mask, cost_in, cost, rms, info, wsum, None)


def test_c_entries_refuse_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.weight()
    before = lib.weight_launch_count()
    nan, inf = float("nan"), float("inf")
    bad = [{name: None} for name in ("conf", "first", "second", "m", "cnt", "weight")]
    bad += [dict(conf=P[0] + 2), dict(first=P[1] + 2), dict(second=P[2] + 1), dict(m=P[3] + 4), dict(cnt=P[4] + 2), dict(weight=P[5] + 2)]
    bad += [dict(n_bank=0), dict(K=0), dict(n1=0), dict(n_pairs=0), dict(n_pairs=-1), dict(mode=2), dict(mode=-1), dict(mode=7, sigma0=1.0)]
    bad += [dict(mode=1, sigma0=v) for v in (0.0, -1.0, nan, inf, -inf)]
    for kw in bad:
        assert _weights_call(L, **kw) == E_INVALID, kw
    for v in (0.0, -1.0, nan, inf):                   # ignored in the first mode: these pass the checks and would launch, so only
        assert lib.check_weights(0, v) == (0, 1.0)    # the wrapper's side is shown here; the GPU test runs the entry
    assert _weights_call(L, n_pairs=1 << 20, n1=1 << 12) == E_UNSUPPORTED and _weights_call(L, n_pairs=0x7fffffff, n1=2) == E_UNSUPPORTED
    pointers = ("kp", "kd", "first", "second", "m", "cnt", "t_in", "weight", "T", "status", "its", "sel", "use", "inl_in", "inl", "mask", "cost_in",
                "cost", "rms", "info", "wsum")
    bad = [{name: None} for name in pointers]
    bad += [dict(kp=P[0] + 4), dict(kd=P[1] + 2), dict(first=P[2] + 2), dict(second=P[3] + 1), dict(m=P[4] + 4), dict(cnt=P[5] + 2),
            dict(t_in=P[6] + 4), dict(weight=P[19] + 2), dict(weight=P[19] + 1), dict(T=P[7] + 4), dict(status=P[8] + 2), dict(its=P[9] + 1),
            dict(sel=P[10] + 2), dict(use=P[11] + 3), dict(inl_in=P[12] + 2), dict(inl=P[13] + 2), dict(mask=P[14] + 2), dict(cost_in=P[15] + 4),
            dict(cost=P[16] + 4), dict(rms=P[17] + 4), dict(info=P[18] + 4), dict(wsum=P[20] + 4)]
    bad += [dict(n_bank=0), dict(K=0), dict(n1=0), dict(n1=-1), dict(n1=9), dict(n_pairs=0), dict(n_iter=-1), dict(n_iter=17),
            dict(thr=-3.0), dict(thr=nan), dict(thr=inf), dict(cx=nan), dict(cy=inf)]
    for name in ("fx", "fy", "ds", "sx", "sy", "vw", "vh", "huber"):
        bad += [{name: 0.0}, {name: -1.0}, {name: nan}, {name: inf}]
    for kw in bad:
        assert _refine_call(L, **kw) == E_INVALID, kw
    for kw in (dict(K=4097, n1=4097), dict(K=4097), dict(K=1 << 20, n1=500)):
        assert _refine_call(L, **kw) == E_UNSUPPORTED, kw
    assert _refine_call(L, K=5000, n1=5001) == E_INVALID, "n1 > K is an invalid argument at any K"
    assert lib.weight_launch_count() == before, "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------------- the planted study
STUDY = dict(seeds=20, matches=200, sigma_lo=0.3, sigma_hi=3.0, share_lo=0.6, huber=3.0, n_iter=8, threshold=40.0, sigma0=0.3)


def _planted_pair(seed):
    """200 matches, depth 1 - 4 m, the default camera; a 3 degree / 5 cm motion; noise on frame b's keypoints of sigma 0.3 px on 60 %
    of the rows and 3 px on the rest; the prior 0.5 degrees and 1.7 cm off; the planted confidences c = 1 / (1 + sigma) on frame b
    and 1 / 1.3 on frame a."""
    rng = np.random.default_rng(41000 + seed)
    cam, n = rr.Cam(), STUDY["matches"]
    a = np.stack([rng.uniform(30, cam.width - 30, n), rng.uniform(30, cam.height - 30, n)], axis=1).astype(np.float32)
    da = rng.integers(5000, 20000, n).astype(np.int32)
    axis = rng.normal(size=3)
    t = rng.normal(size=3)
    T = rr.rigid(rr.rotation(axis, np.deg2rad(3.0)), 0.05 * t / np.linalg.norm(t))
    m = T.reshape(3, 4)
    Xb = rr.back_project(a, da, cam, 1.0, 1.0) @ m[:, :3].T + m[:, 3]
    sigma = np.where(rng.uniform(size=n) < STUDY["share_lo"], STUDY["sigma_lo"], STUDY["sigma_hi"])
    proj = np.stack([cam.fx * Xb[:, 0] / Xb[:, 2] + cam.cx, cam.fy * Xb[:, 1] / Xb[:, 2] + cam.cy], axis=1)
    b = (proj + rng.normal(size=(n, 2)) * sigma[:, None]).astype(np.float32)
    db = np.maximum(np.rint(Xb[:, 2] * cam.depth_scale), 1).astype(np.int32)
    dR = rr.rotation(rng.normal(size=3), np.deg2rad(0.5))
    prior = np.hstack([dR @ m[:, :3], (dR @ m[:, 3] + np.array([0.01, -0.01, 0.01]))[:, None]]).reshape(12)
    matches = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int64)
    conf = np.stack([np.full(n, np.float32(1.0 / 1.3), np.float32), (1.0 / (1.0 + sigma)).astype(np.float32)])
    return dict(a=a, b=b, da=da, db=db, T=T, prior=prior, matches=matches, conf=conf, cam=cam)


def test_planted_study_calibrated_weights_beat_uniform_ones():
    """The issue's study, fixed: 20 seeds; the restatement under expected_error(0.3) and under product() against all-ones weights,
    from the same prior, Huber 3 px, 8 steps, every row geometrically in (threshold 40 px: the prior moves a point by at most about
    15 px, the noise by 9).  Each weighted form must have the lower median rotation error and the lower median translation error,
    and be better in at least 18 of 20 seeds on each figure.  Measured with this restatement (rotation / translation, medians over
    the seeds): uniform 0.0454 degrees / 1.45 mm; expected_error 0.0126 degrees / 0.38 mm, better in 19 and 20 of 20; product
    0.0221 degrees / 0.75 mm, better in 19 and 20 of 20."""
    err = {"uniform": [], "expected_error": [], "product": []}
    for seed in range(STUDY["seeds"]):
        p = _planted_pair(seed)
        n = STUDY["matches"]
        forms = {"uniform": np.ones((1, n), np.float32),
                 "expected_error": wr.match_weights(p["conf"], [0], [1], p["matches"][None], [n], wr.EXPECTED_ERROR, STUDY["sigma0"]),
                 "product": wr.match_weights(p["conf"], [0], [1], p["matches"][None], [n], wr.PRODUCT)}
        for form, w in forms.items():
            r = wr.refine(p["a"], p["b"], p["da"], p["db"], p["matches"], n, w[0], p["cam"], STUDY["threshold"], STUDY["huber"], STUDY["n_iter"],
                          p["prior"])
            assert r["status"] == 0 and r["inlier_count_in"] == n == r["selected_count"], (seed, form, r["status"])
            err[form].append(rr.pose_error(r["T"], p["T"]))
    err = {k: np.array(v) for k, v in err.items()}
    med = {k: np.median(v, axis=0) for k, v in err.items()}
    for form in err:
        better = (err[form] < err["uniform"]).sum(axis=0)
        print(f"{form}: median {med[form][0]:.4f} degrees / {med[form][1] * 1e3:.2f} mm; better than uniform in {better[0]} (rotation) and "
              f"{better[1]} (translation) of {STUDY['seeds']} seeds")
    for form in ("expected_error", "product"):
        better = (err[form] < err["uniform"]).sum(axis=0)
        assert med[form][0] < med["uniform"][0] and med[form][1] < med["uniform"][1], (form, med)
        assert better[0] >= 18 and better[1] >= 18, (form, better)
