"""CPU tests of the pose refinement: the seeded cases of tests/pose_refine_cases.py against their margins, the restatement of
tests/pose_refine_ref.py against an independent implementation (np.linalg.solve, np.sum, matrix products), against a
finite-difference gradient and against the planted motions, its accuracy on noisy pairs beside RANSAC's Horn refit, and everything
that is refused before any device work.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pose_ransac_cases as rc
import pose_ransac_ref as rr
import pose_refine_cases as cases
import pose_refine_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
P = [0x10000 * (i + 1) for i in range(20)]       # never dereferenced: every call below is refused before the launch


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300))


# ------------------------------------------------------------------------------------------------------------- the case lists
@pytest.mark.parametrize("name", cases.NAMES)
def test_cases_keep_their_margins(name):
    c = cases.case(name)
    m = cases.check_margins(c)
    print(f"{name}: " + ", ".join(f"{key} {v:.3e}" for key, v in m.items()))
    assert cases.margins_ok(m), (name, m)
    assert rc.margins_ok(rc.check_margins(c, cases.SEED)), "the RANSAC restatement that gives T_in keeps its own margins"


@pytest.mark.parametrize("name,override", cases.VARIATIONS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in o.items())}" for n, o in cases.VARIATIONS])
def test_variations_keep_their_margins(name, override):
    """Every decision but the cost comparison of a converged iteration (pose_refine_cases' docstring says why that one cannot)."""
    m = cases.check_margins(cases.case(name), with_cost=False, **override)
    print(f"{name} {override}: " + ", ".join(f"{key} {v:.3e}" for key, v in m.items()))
    assert cases.margins_ok(m), (name, override, m)


def test_case_list_covers_what_it_must():
    usable, pairs, status, kinds = set(), set(), set(), set()
    for name in cases.NAMES:
        c, e = cases.case(name), cases.expected(name)
        usable |= {int(rr.usable_rows(c["bank"][a], c["bank"][b], c["depth_bank"][a], c["depth_bank"][b], c["matches"][p], c["count"][p], c["cam"],
                                      c["scale_x"], c["scale_y"])["slot"].size) for p, (a, b) in enumerate(zip(c["first"], c["second"])) if rc.present(c, p)}
        pairs.add(len(c["first"]))
        status |= set(e["status"].tolist())
        kinds.add(c["kind"])
    assert {3, 5, 64, 255, 256, 257, 1024, 1025, 4096} <= usable, sorted(usable)
    assert {1, 3, 70} <= pairs and status == {0, 1, 2, 3} and kinds == {"ransac", "prior", "identity", "nan"}
    assert {(cases.case(n)["bank"].shape[1], cases.case(n)["n1"]) for n in cases.NAMES} >= {(300, 257), (4096, 4096), (1025, 1025)}
    assert {cases.case(n)["n_iter"] for n in cases.NAMES} | {o["n_iter"] for _, o in cases.VARIATIONS if "n_iter" in o} >= {0, 1, 5, 16}
    assert {(cases.case(n)["scale_x"], cases.case(n)["scale_y"]) for n in cases.NAMES} == {(1.0, 1.0), rc.SCALE_448}
    c, e = cases.case("k64_p70"), cases.expected("k64_p70")
    absent = [p for p in range(70) if not rc.present(c, p)]
    assert absent == [1, 30, 68]
    for p in absent + [3, 4, 7]:                          # absent, count 0, count negative, 2 usable rows: not attempted
        assert e["status"][p] == 3 and not e["info"][p].any() and e["cost"][p] == 0.0 and e["usable_count"][p] == 0
        assert e["T"][p].tobytes() == c["T_in"][p].tobytes()
    assert not e["inlier_of_slot"][1].any() and (e["inlier_of_slot"][7] == 0).sum() == 2 and (e["inlier_of_slot"][7] == -1).sum() == c["n1"] - 2
    k3 = cases.expected("k3")
    assert k3["status"][0] == 0 and k3["selected_count"][0] == 3 and k3["usable_count"][0] == 3, "three usable rows are refined"
    assert e["status"][2] == 3, "all outliers: RANSAC's pose has fewer than 3 inliers"
    assert e["status"][9] == 0 and len(np.unique(c["bank"][c["first"][9]], axis=0)) < 40, "coincident points that still determine a pose"
    d = cases.case("k5_dup")
    assert d["singular"][0] and cases.expected("k5_dup")["status"][0] == 1, "coincident points: the singular system ends at its pivot"
    nan = cases.expected("k64_p70_nan")
    for p in range(1, 70, 2):
        assert nan["status"][p] == 3 and nan["T"][p].tobytes() == cases.case("k64_p70_nan")["T_in"][p].tobytes()
    assert not np.isfinite(cases.case("k64_p70_nan")["T_in"]).all(axis=1)[1::2].any()
    few = cases.expected("k64_p70_identity")
    assert ((few["selected_count"] >= 3) & (few["selected_count"] < 0.5 * few["usable_count"])).any(), "a pose with few inliers is refined"
    # huber below every residual and above every residual, in every pass
    for name, override, below in (("k64_loose", dict(huber=1e-3, n_iter=2), True), ("k64_p70_identity", dict(huber=1e-3, n_iter=1), True),
                                  ("k64_loose", dict(huber=1e5, n_iter=5), False), ("k257", dict(huber=1e3, n_iter=5), False)):
        assert (name, override) in cases.VARIATIONS
        for r in cases.run(cases.case(name), detail=True, **override):
            for d_ in (r["log"]["pass_d"] if r["log"] else []):
                assert ((d_ > override["huber"]) if below else (d_ < override["huber"])).all()


# ---------------------------------------------------------------------------------------- the restatement against the independent one
def _rows_of(c, p, r):
    return r["rows"]["Xa"][r["selected"]], r["rows"]["kb"][r["selected"]]


def test_restatement_equals_the_independent_implementation():
    """T, cost and info to 1e-9 relative; the status and the accepted steps of the base runs equal.  Relative means in the
    maximum norm of each quantity - the 12 entries of T, the 36 of H, and the pair (cost_in, cost): a cost that a step takes to
    the rounding level of the residuals (three points fitted exactly: 4e-15 from 1.4e-5) is a cancelled sum of squares of
    differences of ~300 px coordinates and has no relative accuracy of its own in either implementation."""
    worst, n = dict(T=0.0, cost=0.0, info=0.0), 0
    for name in cases.NAMES:
        c = cases.case(name)
        for p, r in enumerate(cases.run(c, detail=True)):
            if r["status"] == 3:
                continue
            Xa, kb = _rows_of(c, p, r)
            T, cost_in, cost, H, accepted = fr.plain_refine(Xa, kb, c["cam"], c["scale_x"], c["scale_y"], c["huber"], c["n_iter"], c["T_in"][p])
            if c["singular"][p]:
                assert np.linalg.matrix_rank(H) < 6 and r["status"] == 1, (name, p)
                continue
            assert accepted == r["iterations"], (name, p, accepted, r["iterations"])
            if r["status"] == 2:                              # not kept: the restatement reports T_in's figures
                T, cost, H = c["T_in"][p], cost_in, fr.plain_normal_equations(c["T_in"][p], Xa, kb, c["cam"], c["scale_x"], c["scale_y"], c["huber"])[1]
            e = dict(T=_rel(r["T"], T), cost=_rel([r["cost_in"], r["cost"]], [cost_in, cost]), info=_rel(fr.full_info(r["info"]), H))
            worst = {key: max(worst[key], e[key]) for key in worst}
            n += 1
            assert max(e.values()) <= 1e-9, (name, p, e)
    print(f"{n} pairs: largest relative difference " + ", ".join(f"{key} {v:.2e}" for key, v in worst.items()))
    assert n >= 150


def test_gradient_equals_the_finite_difference_of_half_the_cost():
    n = 0
    for name in ("k64_p70_prior", "k64_p70_identity", "k64_loose", "k300_n257"):
        c = cases.case(name)
        for p, r in enumerate(cases.run(c, detail=True, n_iter=0)):
            if r["status"] == 3:
                continue
            Xa, kb = _rows_of(c, p, r)
            g = fr.finite_difference_gradient(c["T_in"][p], Xa, kb, c["cam"], c["scale_x"], c["scale_y"], c["huber"])
            assert _rel(r["g"], g) <= 1e-6, (name, p, r["g"], g)
            n += 1
    assert n >= 100


def test_cost_never_rises_and_an_unrefined_pose_is_the_input_bit_for_bit():
    runs = [(name, ()) for name in cases.NAMES] + [(name, tuple(o.items())) for name, o in cases.VARIATIONS]
    for name, var in runs:
        c, e = cases.case(name), cases.expected(name, var)
        t_in = dict(var).get("T_in", c["T_in"])
        assert (e["cost"] <= e["cost_in"]).all(), (name, var)
        for p in np.where(e["status"] != 0)[0]:
            assert e["T"][p].tobytes() == t_in[p].tobytes(), (name, var, p)
            assert e["cost"][p] == e["cost_in"][p]
        ok = e["status"] == 0
        assert (e["cost"][ok] < e["cost_in"][ok]).all() and (e["iterations"][ok] >= 1).all() and (e["inlier_count"][ok] >= e["inlier_count_in"][ok]).all()
        assert (e["iterations"][e["status"] == 1] == 0).all() and (e["iterations"][e["status"] == 2] >= 1).all()
        assert (e["iterations"] <= dict(var).get("n_iter", c["n_iter"])).all()
        assert np.array_equal(e["selected_count"], e["inlier_count_in"])
        assert np.array_equal((e["inlier_of_slot"] == 1).sum(axis=1), e["inlier_count"])


def test_restatement_keeps_the_planted_motion_and_converges_from_the_prior():
    worst, n = [0.0, 0.0], 0
    for name in cases.NAMES:
        c, e = cases.case(name), cases.expected(name)
        if c["kind"] != "ransac":
            continue
        for p in np.where(c["recover"])[0]:
            deg, m = rr.pose_error(e["T"][p], c["planted"][p])
            worst, n = [max(worst[0], deg), max(worst[1], m)], n + 1
            assert deg <= cases.RECOVER_DEG and m <= cases.RECOVER_M, (name, p, deg, m)
    print(f"{n} noise-free pairs refined from RANSAC's pose: largest rotation error {worst[0]:.3e} degrees, largest translation error {worst[1]:.3e} m")
    assert n >= 20
    # the prior (2 degrees, 5 cm off) under the wide threshold: 16 steps take nine recoverable pairs in ten at least 5 times closer
    # in both figures.  The minimum they reach is the Huber minimum over the rows within 60 px of the prior, chance outliers
    # among them, so not every pair ends AT the planted motion (printed, not asserted); a pair whose result loses inliers is not kept
    for name in ("k64_p70_prior", "k1025"):
        c, e = cases.case(name), cases.expected(name, (("n_iter", 16),))
        closer = exact = total = 0
        for p in np.where(c["recover"])[0]:
            d0, m0 = rr.pose_error(c["T_in"][p], c["planted"][p])
            d1, m1 = rr.pose_error(e["T"][p], c["planted"][p])
            total += 1
            closer += e["status"][p] == 0 and d1 <= d0 / 5 and m1 <= m0 / 5
            exact += d1 <= cases.RECOVER_DEG and m1 <= cases.RECOVER_M
        print(f"{name}: of {total} pairs {closer} end 5 times closer, {exact} at the planted motion")
        assert total >= 2 and closer >= 0.9 * total


# ------------------------------------------------------------------------------------------------------ accuracy on noisy pairs
def _noisy_pair(seed):
    """pose_ransac_cases' planted pair (K = 500, 380 listed, 30 % outliers) with Gaussian keypoint noise of 0.5 px on both frames and
    depth noise of 0.0012 z^2 m on both."""
    rng = np.random.default_rng(seed)
    p = rc._pair(rng, 500, 380, (1.0, 1.0))
    cam = rc.CAM
    out = {}
    for kp, d, key in ((p["a"], p["da"], "a"), (p["b"], p["db"], "b")):
        z = d / cam.depth_scale
        out["d" + key] = np.where(d > 0, np.maximum(np.rint((z + rng.normal(size=len(z)) * 0.0012 * z * z) * cam.depth_scale), 1), d).astype(np.int32)
        out[key] = (kp.astype(np.float64) + rng.normal(size=kp.shape) * 0.5).astype(np.float32)
    return dict(p, **out)


def test_refinement_halves_the_translation_error_of_noisy_pairs():
    """The issue's first prototype row: sigma 0.5 px, depth noise 0.0012 z^2, 30 % outliers, K = 500, 380 listed, threshold 3,
    huber 1, 256 hypotheses, 5 steps, 40 seeded pairs.  Measured with this restatement: median after the Horn refit 0.0360 degrees
    / 2.012 mm, after the refinement 0.0159 degrees / 0.472 mm; translation better in 40 of 40 pairs, rotation in 36.  The bounds
    are the issue's: at most half the median translation error, better in 32 of 40 at least."""
    before, after = [], []
    for seed in range(40):
        p = _noisy_pair(9000 + seed)
        r = rr.ransac(p["a"], p["b"], p["da"], p["db"], p["matches"], p["count"], rc.CAM, 3.0, 256, seed)
        f = fr.refine(p["a"], p["b"], p["da"], p["db"], p["matches"], p["count"], rc.CAM, 3.0, 1.0, 5, r["T"])
        before.append(rr.pose_error(r["T"], p["T"]))
        after.append(rr.pose_error(f["T"], p["T"]))
    before, after = np.array(before), np.array(after)
    med_b, med_a = np.median(before, axis=0), np.median(after, axis=0)
    better = (after < before).sum(axis=0)
    print(f"median error after the Horn refit {med_b[0]:.4f} degrees, {med_b[1] * 1e3:.3f} mm; after refinement {med_a[0]:.4f} degrees, "
          f"{med_a[1] * 1e3:.3f} mm; translation better in {better[1]} of 40 pairs, rotation in {better[0]}")
    assert med_a[1] <= 0.5 * med_b[1]
    assert better[1] >= 32


# -------------------------------------------------------------------------------------------------- refused before the device
def _refine(L, kp=P[0], kd=P[1], n_bank=3, K=8, first=P[2], second=P[3], n_pairs=2, m=P[4], cnt=P[5], n1=8, fx=525.0, fy=525.0, cx=319.5,
            cy=239.5, ds=5000.0, sx=1.0, sy=1.0, vw=640.0, vh=480.0, thr=3.0, t_in=P[6], huber=1.0, n_iter=5, T=P[7], status=P[8], its=P[9],
            sel=P[10], use=P[11], inl_in=P[12], inl=P[13], mask=P[14], cost_in=P[15], cost=P[16], rms=P[17], info=P[18]):
    return L.sslam_pose_refine_pairs(kp, kd, n_bank, K, first, second, n_pairs, m, cnt, n1,
                                     *(ctypes.c_double(v) for v in (fx, fy, cx, cy, ds, sx, sy, vw, vh, thr)), t_in, ctypes.c_double(huber), n_iter,
                                     T, status, its, sel, use, inl_in, inl, mask, cost_in, cost, rms, info, None)


def test_c_entry_refuses_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    before = lib.launch_count()
    nan, inf = float("nan"), float("inf")
    pointers = ("kp", "kd", "first", "second", "m", "cnt", "t_in", "T", "status", "its", "sel", "use", "inl_in", "inl", "mask", "cost_in", "cost",
                "rms", "info")
    bad = [{name: None} for name in pointers]
    bad += [dict(kp=P[0] + 4), dict(kd=P[1] + 2), dict(first=P[2] + 2), dict(second=P[3] + 1), dict(m=P[4] + 4), dict(cnt=P[5] + 2),
            dict(t_in=P[6] + 4), dict(T=P[7] + 4), dict(status=P[8] + 2), dict(its=P[9] + 1), dict(sel=P[10] + 2), dict(use=P[11] + 3),
            dict(inl_in=P[12] + 2), dict(inl=P[13] + 2), dict(mask=P[14] + 2), dict(cost_in=P[15] + 4), dict(cost=P[16] + 4), dict(rms=P[17] + 4),
            dict(info=P[18] + 4)]
    bad += [dict(n_bank=0), dict(K=0), dict(n1=0), dict(n1=-1), dict(n1=9), dict(n_pairs=0), dict(n_iter=-1), dict(n_iter=17),
            dict(thr=-3.0), dict(thr=nan), dict(thr=inf), dict(cx=nan), dict(cy=inf)]
    for name in ("fx", "fy", "ds", "sx", "sy", "vw", "vh", "huber"):
        bad += [{name: 0.0}, {name: -1.0}, {name: nan}, {name: inf}]
    for kw in bad:
        assert _refine(L, **kw) == E_INVALID, kw
    for kw in (dict(K=4097, n1=4097), dict(K=4097), dict(K=1 << 20, n1=500)):
        assert _refine(L, **kw) == E_UNSUPPORTED, kw
    assert _refine(L, K=5000, n1=5001) == E_INVALID, "n1 > K is an invalid argument at any K"
    assert lib.launch_count() == before, "a refused call launches nothing"


def test_entry_is_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sslam_hip.h")).read()
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    entry = "sslam_pose_refine_pairs"
    assert re.search(r"^int\s+" + entry + r"\s*\(", hdr, flags=re.M)
    assert entry in lib.EXPORTS and re.search(r"\bT\s+" + entry + r"$", dyn, flags=re.M)
    L = lib.lib()
    assert L.sslam_version() > 640, "a new entry raises the version"
    assert len(L.sslam_pose_refine_pairs.argtypes) == 36
    decl = hdr[hdr.index("int " + entry):]
    assert decl[:decl.index(";")].count(",") == 35, "36 arguments in the header's declaration"
    assert re.search(r"#define\s+SSLAM_REFINE_MAX_ITER\s+16", hdr) and lib.REFINE_MAX_ITER == 16 == fr.MAX_ITER
    for text in ("rho = (2 * huber) * d - huber * huber", "Ju = (a, 0, c, c*Y', a*Z' - c*X', -(a*Y'))", "Jv = (0, b, e, e*Y' - b*Z', -(e*X'), b*X')",
                 "D_j = D_j - (L_jk * L_jk) * D_k", "delta_i = delta_i - L_ki * delta_k", "x = 0.5 * wx", "its cost < the current cost",
                 "KEEP RULE", "lanes by xor 32 .. 1"):
        assert text in hdr, text
    assert os.path.exists(os.path.join(lib.CSRC, "pose_refine.hip"))
    assert lib.POSE_REFINE_KEYS == fr.KEYS
    import torch
    sh = lib.pose_refine_shapes(3, 7)
    assert sh["T"] == ((3, 12), torch.float64) and sh["inlier_of_slot"] == ((3, 7), torch.int32) and sh["info"] == ((3, 21), torch.float64)
    assert all(sh[key] == ((3,), torch.float64) for key in ("cost_in", "cost", "rms"))
    assert all(sh[key] == ((3,), torch.int32) for key in ("status", "iterations", "selected_count", "usable_count", "inlier_count_in", "inlier_count"))


def test_api_refuses_malformed_arguments_before_the_library_is_touched(monkeypatch):
    import torch

    import evaluation as dropin
    from sslam_amd import evaluation as ev
    from sslam_amd import harness, lib, online
    from sslam_amd import odometry as od
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline

    def touched():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(lib, "lib", touched)
    for v in (0.0, -1.0, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError, match="huber"):
            lib.check_huber(v)
    for v in (-1, 17, 2.0, True, None):
        with pytest.raises(ValueError, match="iterations"):
            lib.check_iterations(v)
    assert lib.check_huber(2) == 2.0 and lib.check_iterations(0) == 0 and lib.check_iterations(np.int64(16)) == 16
    cam = ev.Camera()
    kp, kd = torch.zeros((3, 8, 2)), torch.zeros((3, 8), dtype=torch.int32)
    f, s = torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    m, c = torch.zeros((2, 8, 2), dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    t_in = torch.zeros((2, 12), dtype=torch.float64)
    for kw, match in ((dict(huber=0.0), "huber"), (dict(huber=float("nan")), "huber"), (dict(iterations=17), "iterations"),
                      (dict(iterations=-1), "iterations"), (dict(iterations=1.0), "iterations"), (dict(threshold=-1.0), "threshold"),
                      (dict(scale_x=0.0), "scale_x"), (dict(camera=ev.Camera(fx=0.0)), "camera fx"), (dict(T_in=t_in.float()), "T_in"),
                      (dict(T_in=t_in[:1]), "T_in"), (dict(T_in=None), "T_in")):
        args = dict(camera=cam, T_in=t_in)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            lib.pose_refine_pairs(kp, kd, f, s, m, c, **args)
    for args, match in (((kp.double(), kd, f, s, m, c), "kp_bank"), ((kp, None, f, s, m, c), "kp_depth_bank"), ((kp, kd, f, s[:1], m, c), "unequal"),
                        ((kp, kd, f, s, m.int(), c), "matches"), ((kp, kd, f, s, m, None), "count")):
        with pytest.raises(ValueError, match=match):
            lib.pose_refine_pairs(*args, cam, t_in)
    with pytest.raises(ValueError, match="out must hold"):
        lib.pose_refine_pairs(kp, kd, f, s, m, c, cam, t_in, out=(m,))
    with pytest.raises(ValueError, match="out `T`"):
        lib.pose_refine_pairs(kp, kd, f, s, m, c, cam, t_in, out=(torch.zeros((2, 12)),) + (c,) * 11)
    with pytest.raises(ValueError):                                 # well-formed host tensors: refused for where they live
        lib.pose_refine_pairs(kp, kd, f, s, m, c, cam, t_in)
    pipe = SequencePipeline.__new__(SequencePipeline)               # the argument checks need no weights and no device
    pipe.cfg = ExtractorConfig(input_size=64, num_keypoints=8)
    mm = dict(matches=m, match_count=c)
    for args, kw, match in (((kp[0], kd, f, s, mm, cam, t_in), {}, "keypoints_pixel"), ((kp, kd[:, :7], f, s, mm, cam, t_in), {}, "kp_depth"),
                            ((kp, kd, None, s, mm, cam, t_in), {}, "pair lists"), ((kp, kd, f, s, m, cam, t_in), {}, "dictionary"),
                            ((kp, kd, f, s, mm, cam, t_in[:1]), {}, "pose must be"), ((kp, kd, f, s, mm, cam, dict(rms=c)), {}, "pose must be"),
                            ((kp, kd, f, s, mm, cam, t_in), dict(huber=-1.0), "huber"), ((kp, kd, f, s, mm, cam, t_in), dict(threshold=0.0), "huber"),
                            ((kp, kd, f, s, mm, cam, t_in), dict(iterations=99), "iterations")):
        with pytest.raises(ValueError, match=match):
            pipe.refine_poses(*args, **kw)
    toks, depth = np.zeros((3, 9, 384), np.float32), np.zeros((3, 480, 640), np.uint16)
    for kw, match in ((dict(refine=1), "refine"), (dict(refine=True, huber=0.0), "huber"), (dict(refine=True, iterations=17), "iterations"),
                      (dict(refine=True, threshold=0.0), "huber")):
        with pytest.raises(ValueError, match=match):
            od.odometry(None, tokens=toks, depth=depth, **kw)
        with pytest.raises(ValueError, match=match):
            od.odometry_result(None, {"frames": {"keypoints_pixel": kp}, 1: mm}, depth=depth, **kw)
    with pytest.raises(ValueError, match="flag"):
        harness.run_directory("/nonexistent", evaluate={"odometry": True, "refine": 1})
    with pytest.raises(ValueError, match='needs "odometry"'):
        harness.run_directory("/nonexistent", evaluate={"refine": True})
    with pytest.raises(ValueError, match='needs "odometry"'):
        harness.run_directory("/nonexistent", evaluate={"depth": True, "refine": True})
    with pytest.raises(ValueError, match="refine"):
        online.PoseFrameStepper(None, 48, 64, 480, 640, refine="yes")
    with pytest.raises(ValueError, match="huber"):
        online.PoseFrameStepper(None, 48, 64, 480, 640, refine=True, huber=0.0)
    with pytest.raises(ValueError, match="iterations"):
        online.PoseFrameStepper(None, 48, 64, 480, 640, refine=True, iterations=17)
    k1, d1, pm = np.zeros((5, 2), np.float32), np.zeros((480, 640), np.uint16), np.zeros((4, 2), np.int64)
    for args, kw, match in (((k1, k1, d1.astype(np.int32), d1, pm, np.eye(4)), {}, "depth1"), ((k1, k1, d1, d1, pm, np.eye(3)), {}, "T \\(4, 4\\)"),
                            ((k1, k1, d1, d1, pm, np.eye(4)), dict(huber=0.0), "huber"), ((k1, k1, d1, d1, pm, np.eye(4)), dict(iterations=-1), "iterations"),
                            ((k1, k1, d1, d1, pm, np.eye(4)), dict(threshold=-2.0), "threshold"), ((k1[:, :1], k1, d1, d1, pm, np.eye(4)), {}, "keypoints"),
                            ((k1, k1, d1, d1, pm[:, :1], np.eye(4)), {}, "matches")):
        with pytest.raises(ValueError, match=match):
            dropin.refine_relative_pose(*args, **kw)
    start = np.eye(4)
    start[0, 3] = 0.25
    T, mask, info = dropin.refine_relative_pose(k1, k1, d1, d1, np.zeros((0, 2), np.int64), start)
    assert np.array_equal(T, start) and mask.shape == (0,) and mask.dtype == bool and info.shape == (6, 6) and not info.any()
    ii = od.info_matrix(np.arange(42.0).reshape(2, 21))
    assert ii.shape == (2, 6, 6) and np.array_equal(ii, ii.transpose(0, 2, 1)) and np.array_equal(ii[0][np.triu_indices(6)], np.arange(21.0))
