"""CPU tests of the relative pose from matches and depth: the seeded cases of tests/pose_ransac_cases.py against their margins, the
sampler, the restatement of tests/pose_ransac_ref.py against the planted motions, the host arithmetic of sslam_amd.odometry against
hand-computed examples, and everything that is refused before any device work.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pose_ransac_cases as cases
import pose_ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
P = [0x10000 * (i + 1) for i in range(16)]       # never dereferenced: every call below is refused before the launch


# ------------------------------------------------------------------------------------------------------------- the case lists
@pytest.mark.parametrize("name", cases.NAMES)
def test_cases_keep_their_margins(name):
    c = cases.case(name)
    for seed in cases.seeds_of(name):
        m = cases.check_margins(c, seed)
        print(f"{name} seed {seed:#x}: least |d - threshold| {m['edge']:.3e} px, least |Z'| {m['z']:.3e} m")
        assert cases.margins_ok(m), (name, seed, m)


def test_case_list_covers_what_it_must():
    shapes = {(c["bank"].shape[1], c["n1"]) for c in map(cases.case, cases.NAMES)}
    assert {(k, k) for k in (3, 5, 64, 257, 1024, 1025, 4096)} | {(300, 257)} <= shapes
    assert {cases.case(n)["n_hyp"] for n in cases.NAMES} >= {1, 63, 64, 65, 256, 1024}
    assert {len(cases.case(n)["first"]) for n in cases.NAMES} >= {1, 3, 70}
    assert {(cases.case(n)["scale_x"], cases.case(n)["scale_y"]) for n in cases.NAMES} == {(1.0, 1.0), cases.SCALE_448}
    c, e = cases.case("k64_p70"), cases.expected("k64_p70", cases.SEEDS[0])
    assert len(cases.seeds_of("k64_p70")) == 2
    absent = [p for p in range(70) if not cases.present(c, p)]
    assert absent == [1, 30, 68] and all(cases.present(c, p - 1) and cases.present(c, p + 1) for p in absent)
    for p in absent:                                     # no pose, whatever the list holds
        assert e["best_hypothesis"][p] == -1 and e["usable_count"][p] == 0 and not e["inlier_of_slot"][p].any()
        assert np.array_equal(e["T"][p], cases.IDENT) and e["rms"][p] == 0.0
    assert c["count"][3] == 0 and c["count"][4] < 0 and c["count"][5] > c["n1"] and 0 < c["count"][13] < c["n1"]
    assert e["usable_count"][3] == 0 and e["usable_count"][4] == 0 and e["usable_count"][5] == c["n1"]
    assert (e["inlier_of_slot"][13][c["count"][13]:] == 0).all(), "0 past the count"
    assert (c["matches"][6] < 0).any() and (c["matches"][6] >= 64).any() and (e["inlier_of_slot"][6] == -1).sum() >= 4
    assert e["usable_count"][7] == 2 and e["best_hypothesis"][7] == -1 and (e["inlier_of_slot"][7] == 0).sum() == 2
    assert e["usable_count"][8] == 3 and e["best_hypothesis"][8] == 0 and e["inlier_count"][8] == 3
    assert e["inlier_count"][2] < 3 and e["refit_kept"][2] == 0, "all outliers: no refit"
    loose = cases.expected("k64_loose", cases.SEEDS[0])
    assert ((loose["inlier_count"] >= 3) & (loose["refit_kept"] == 0)).any(), "a refit that lost inliers and was dropped"
    assert ((loose["inlier_count"] >= 3) & (loose["refit_kept"] == 1)).any()
    # coincident points: some hypothesis samples three of them, and rows behind the camera are scored
    d = cases.case("k5_dup")
    r = rr.ransac(d["bank"][0], d["bank"][1], d["depth_bank"][0], d["depth_bank"][1], d["matches"][0], d["count"][0], d["cam"], d["threshold"],
                  d["n_hyp"], cases.SEEDS[0], d["scale_x"], d["scale_y"], detail=True)
    Xa = r["rows"]["Xa"][r["samples"]]
    assert (np.ptp(Xa, axis=1) == 0).all(axis=1).any(), "a degenerate sample"
    behind = False
    for p in (14, 18, 22):                               # pairs with 60 % outliers: hypotheses from outliers turn the scene around
        a, b = c["first"][p], c["second"][p]
        r = rr.ransac(c["bank"][a], c["bank"][b], c["depth_bank"][a], c["depth_bank"][b], c["matches"][p], c["count"][p], c["cam"], c["threshold"],
                      c["n_hyp"], cases.SEEDS[0], detail=True)
        behind |= bool((rr.score(r["hypotheses"], r["rows"]["Xa"], r["rows"]["kb"], c["cam"], 1.0, 1.0, c["threshold"])["Z2"] <= 0).any())
    assert behind, "rows with Z' <= 0"


# ------------------------------------------------------------------------------------------------------------------ the sampler
def test_sampler_rows_are_distinct_and_in_range():
    for seed in cases.SEEDS + (1, 2 ** 64 - 1):
        for n in list(range(3, 70)) + [255, 256, 257, 1000, 4095, 4096]:
            s = rr.sample(seed, rr.MAX_HYP, n)
            assert s.min() >= 0 and s.max() < n, (seed, n)
            assert ((s[:, 0] != s[:, 1]) & (s[:, 0] != s[:, 2]) & (s[:, 1] != s[:, 2])).all(), (seed, n)
    assert set(map(tuple, rr.sample(0, rr.MAX_HYP, 3))) == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    # a pure function of (seed, h, draw): a prefix of the hypotheses is a prefix of the samples; splitmix64's published first output
    assert np.array_equal(rr.sample(7, 64, 500), rr.sample(7, 1024, 500)[:64])
    assert int(rr.mix(np.uint64(0x9e3779b97f4a7c15))) == 0xe220a8397b1dcdaf


# ------------------------------------------------------------------------------------------- the restatement against the truth
def test_restatement_recovers_the_planted_motion():
    worst = [0.0, 0.0]
    n = 0
    for name in cases.NAMES:
        c = cases.case(name)
        for seed in cases.seeds_of(name):
            e = cases.expected(name, seed)
            for p in np.where(c["recover"])[0]:
                deg, m = rr.pose_error(e["T"][p], c["planted"][p])
                worst = [max(worst[0], deg), max(worst[1], m)]
                n += 1
                assert deg <= cases.RECOVER_DEG and m <= cases.RECOVER_M, (name, seed, p, deg, m)
                assert e["refit_kept"][p] == 1 and e["inlier_count"][p] >= 0.5 * e["usable_count"][p]
    print(f"{n} pairs: largest rotation error {worst[0]:.3e} degrees, largest translation error {worst[1]:.3e} m")
    assert n >= 20


def test_horn_on_exact_points_and_on_degenerate_ones():
    rng = np.random.default_rng(3)
    Xa = rng.uniform(-2, 2, (50, 3, 3)) + np.array([0, 0, 4.0])
    T = rr.rigid(rr.rotation([0.1, -0.7, 0.3], 0.4), [0.3, -0.2, 0.1]).reshape(3, 4)
    got = rr.solve_samples(Xa, Xa @ T[:, :3].T + T[:, 3])
    assert np.abs(got - T.reshape(12)).max() < 1e-12
    same = np.broadcast_to(Xa[:1, :1], (1, 3, 3))        # three coincident points: no rotation is taken, R = I
    deg = rr.solve_samples(same, same + 1.0)[0].reshape(3, 4)
    assert np.array_equal(deg[:, :3], np.eye(3)) and np.allclose(deg[:, 3], 1.0)
    assert np.isfinite(rr.solve_samples(np.zeros((1, 3, 3)), np.zeros((1, 3, 3)))).all()


def test_tree_sum_is_a_sum_in_one_fixed_order():
    rng = np.random.default_rng(4)
    for n in (1, 3, 255, 256, 257, 1000, 4096):
        t = rng.uniform(-1, 1, (n, 3))
        assert np.abs(rr.tree_sum(t) - t.sum(axis=0)).max() < 1e-12
    assert rr.tree_sum(np.array([1.0, 2 ** -53, 0.0, 2 ** -53])) == 1.0 + 2 ** -52      # xor 2 joins lanes 1 and 3 before xor 1 adds them to lane 0
    assert ((1.0 + 2 ** -53) + 0.0) + 2 ** -53 == 1.0, "the same terms left to right"


# --------------------------------------------------------------------------------------------------------------------- odometry
def test_pose_errors_and_summaries_on_hand_computed_examples():
    from sslam_amd import evaluation as ev
    from sslam_amd import odometry as od
    rng = np.random.default_rng(5)
    poses = [np.eye(4)]
    for _ in range(6):
        step = np.eye(4)
        step[:3] = rr.rigid(rr.rotation(rng.normal(size=3), rng.uniform(0.02, 0.1)), rng.uniform(-0.1, 0.1, 3)).reshape(3, 4)
        poses.append(poses[-1] @ step)
    poses = np.stack(poses)
    pairs = [(i, i + 1) for i in range(6)]
    T_gt = np.stack([ev.relative_transform(poses[a], poses[b]) for a, b in pairs])
    err = od.relative_pose_errors(T_gt, poses, pairs)
    assert err["translation"].max() < 1e-12 and err["rotation"].max() < 1e-5          # arccos near 1: 1e-5 degrees is 1.5e-14 in the cosine
    ident = od.relative_pose_errors(np.stack([np.eye(4)] * 2), np.stack([np.eye(4)] * 3), [(0, 1), (1, 2)])
    assert not ident["translation"].any() and not ident["rotation"].any()
    s0 = od.rpe_summary(ident)
    assert s0 == {"translation": dict(rmse=0.0, mean=0.0, median=0.0, std=0.0), "rotation": dict(rmse=0.0, mean=0.0, median=0.0, std=0.0)}
    # a known offset: the estimate is the truth followed by 10 degrees about z and 0.1 m along x
    off = np.eye(4)
    off[:3, :3], off[0, 3] = rr.rotation([0, 0, 1.0], np.deg2rad(10.0)), 0.1
    err = od.relative_pose_errors(np.stack([t @ off for t in T_gt]), poses, pairs)
    assert np.abs(err["rotation"] - 10.0).max() < 1e-9 and np.abs(err["translation"] - 0.1).max() < 1e-12
    for shape in ((-1, 12), (-1, 3, 4)):                                              # (P, 12) and (P, 3, 4) are taken as well
        e2 = od.relative_pose_errors(T_gt[:, :3].reshape(shape), poses, pairs)
        assert e2["translation"].max() < 1e-12
    s = od.rpe_summary({"translation": np.array([3.0, 4.0]), "rotation": np.array([1.0, 1.0, 4.0])})
    assert list(s) == ["translation", "rotation"] and list(s["translation"]) == ["rmse", "mean", "median", "std"]
    assert s["translation"] == dict(rmse=float(np.sqrt(12.5)), mean=3.5, median=3.5, std=0.5)
    assert s["rotation"] == dict(rmse=float(np.sqrt(6.0)), mean=2.0, median=1.0, std=float(np.sqrt(2.0)))
    # chain of the true transforms gives the poses back, from the identity and from any start
    assert np.abs(od.chain(T_gt) - poses).max() < 1e-12
    start = np.eye(4)
    start[:3] = rr.rigid(rr.rotation([1, 2, 3.0], 1.0), [1.0, 2.0, 3.0]).reshape(3, 4)
    assert np.abs(od.chain(T_gt[:, :3], start) - start @ poses).max() < 1e-12
    assert od.chain(np.zeros((0, 4, 4))).shape == (1, 4, 4)
    # ATE: a rigidly moved copy of the trajectory has none; a single displaced position is seen after the alignment
    a = od.ate_summary(start @ poses, poses)
    assert list(a) == ["rmse", "mean", "median", "std", "min", "max"] and max(a.values()) < 1e-12
    line = np.stack([np.eye(4)] * 5)
    line[:, 0, 3] = np.arange(5.0)
    bent = line.copy()
    bent[2, 1, 3] = 0.5                                   # positions (i, 0, 0) with the middle one 0.5 to the side
    a = od.ate_summary(bent, line)
    # the best rigid fit of a symmetric bump is the shift by its mean, 0.1: errors 0.1 x 4 and 0.4
    assert abs(a["max"] - 0.4) < 1e-12 and abs(a["min"] - 0.1) < 1e-12 and abs(a["mean"] - 0.16) < 1e-12 and abs(a["median"] - 0.1) < 1e-12
    assert abs(a["rmse"] - np.sqrt((4 * 0.01 + 0.16) / 5)) < 1e-12
    mirrored = line.copy()
    mirrored[:, :3, 3] = rng.normal(size=(5, 3))
    R, _ = od.align_rigid(mirrored[:, :3, 3] * np.array([1, 1, -1.0]), mirrored[:, :3, 3])
    assert abs(np.linalg.det(R) - 1.0) < 1e-12, "no reflection"
    with pytest.raises(ValueError):
        od.ate_summary(line[:4], line)
    with pytest.raises(ValueError):
        od.relative_pose_errors(T_gt, poses, pairs[:5])
    with pytest.raises(ValueError):
        od.relative_pose_errors(T_gt, poses[:6], pairs)
    assert od.consecutive_pairs(5, 2) == [(0, 2), (1, 3), (2, 4)] and od.consecutive_pairs(5, 1, 2) == [(0, 1), (1, 2)]
    assert od.consecutive_pairs(3, 5) == []


# -------------------------------------------------------------------------------------------------- refused before the device
def _ransac(L, kp=P[0], kd=P[1], n_bank=3, K=8, first=P[2], second=P[3], n_pairs=2, m=P[4], cnt=P[5], n1=8, fx=525.0, fy=525.0, cx=319.5,
            cy=239.5, ds=5000.0, sx=1.0, sy=1.0, vw=640.0, vh=480.0, thr=3.0, n_hyp=16, seed=0, T=P[6], inl=P[7], use=P[8], best=P[9],
            kept=P[10], mask=P[11], rms=P[12]):
    return L.sslam_pose_ransac_pairs(kp, kd, n_bank, K, first, second, n_pairs, m, cnt, n1,
                                     *(ctypes.c_double(v) for v in (fx, fy, cx, cy, ds, sx, sy, vw, vh, thr)), n_hyp, ctypes.c_uint64(seed),
                                     T, inl, use, best, kept, mask, rms, None)


def test_c_entry_refuses_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    before = lib.launch_count()
    nan, inf = float("nan"), float("inf")
    pointers = ("kp", "kd", "first", "second", "m", "cnt", "T", "inl", "use", "best", "kept", "mask", "rms")
    bad = [{name: None} for name in pointers]
    bad += [dict(kp=P[0] + 4), dict(kd=P[1] + 2), dict(first=P[2] + 2), dict(second=P[3] + 1), dict(m=P[4] + 4), dict(cnt=P[5] + 2),
            dict(T=P[6] + 4), dict(inl=P[7] + 2), dict(use=P[8] + 1), dict(best=P[9] + 2), dict(kept=P[10] + 3), dict(mask=P[11] + 2),
            dict(rms=P[12] + 4)]
    bad += [dict(n_bank=0), dict(K=0), dict(n1=0), dict(n1=-1), dict(n1=9), dict(n_pairs=0), dict(n_hyp=0), dict(n_hyp=-1), dict(n_hyp=1025),
            dict(thr=-3.0), dict(thr=nan), dict(thr=inf), dict(cx=nan), dict(cy=inf)]
    for name in ("fx", "fy", "ds", "sx", "sy", "vw", "vh"):
        bad += [{name: 0.0}, {name: -1.0}, {name: nan}, {name: inf}]
    for kw in bad:
        assert _ransac(L, **kw) == E_INVALID, kw
    for kw in (dict(K=4097, n1=4097), dict(K=4097), dict(K=1 << 20, n1=500)):
        assert _ransac(L, **kw) == E_UNSUPPORTED, kw
    assert _ransac(L, K=5000, n1=5001) == E_INVALID, "n1 > K is an invalid argument at any K"
    assert lib.launch_count() == before, "a refused call launches nothing"


def test_entry_is_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = open(os.path.join(ROOT, "include", "sslam_hip.h")).read()
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    entry = "sslam_pose_ransac_pairs"
    assert re.search(r"^int\s+" + entry + r"\s*\(", hdr, flags=re.M)
    assert entry in lib.EXPORTS and re.search(r"\bT\s+" + entry + r"$", dyn, flags=re.M)
    L = lib.lib()
    assert L.sslam_version() > 630, "a new entry raises the version"
    assert len(L.sslam_pose_ransac_pairs.argtypes) == 30
    decl = hdr[hdr.index("int " + entry):]
    assert decl[:decl.index(";")].count(",") == 29, "30 arguments in the header's declaration"
    assert re.search(r"#define\s+SSLAM_POSE_MAX_HYP\s+1024", hdr) and lib.POSE_MAX_HYP == 1024 == rr.MAX_HYP
    for text in ("0xbf58476d1ce4e5b9", "0x94d049bb133111eb", "0x9e3779b97f4a7c15 * (3*h + k + 1)", "exactly 8 sweeps", "a_pq == 0.0",
                 "theta = (a_qq - a_pp) / (2 * a_pq)", "lanes by xor 32 .. 1", "((w0 + w1) + w2) + w3", "the lowest h on equality",
                 "t_i = c_b[i] - ((r_i0 * c_a[0] + r_i1 * c_a[1]) + r_i2 * c_a[2])", "NO POSE"):
        assert text in hdr, text
    assert os.path.exists(os.path.join(lib.CSRC, "pose_estimate.hip"))
    assert lib.POSE_RANSAC_KEYS == rr.KEYS
    import torch
    sh = lib.pose_ransac_shapes(3, 7)
    assert sh["T"] == ((3, 12), torch.float64) and sh["inlier_of_slot"] == ((3, 7), torch.int32) and sh["rms"] == ((3,), torch.float64)
    assert all(sh[key] == ((3,), torch.int32) for key in ("inlier_count", "usable_count", "best_hypothesis", "refit_kept"))


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
    cam = ev.Camera()
    kp, kd = torch.zeros((3, 8, 2)), torch.zeros((3, 8), dtype=torch.int32)
    f, s = torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    m, c = torch.zeros((2, 8, 2), dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    for kw, match in ((dict(hypotheses=0), "hypotheses"), (dict(hypotheses=1025), "hypotheses"), (dict(hypotheses=2.0), "hypotheses"),
                      (dict(hypotheses=True), "hypotheses"), (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"), (dict(seed=0.5), "seed"),
                      (dict(threshold=-1.0), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(scale_x=0.0), "scale_x"),
                      (dict(scale_y=float("inf")), "scale_y"), (dict(camera=ev.Camera(fx=0.0)), "camera fx"), (dict(camera=(1, 2)), "camera must have")):
        args = dict(camera=cam)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            lib.pose_ransac_pairs(kp, kd, f, s, m, c, **args)
    for args, match in (((kp.double(), kd, f, s, m, c), "kp_bank"), ((kp, kd.long(), f, s, m, c), "kp_depth_bank"), ((kp, None, f, s, m, c), "kp_depth_bank"),
                        ((kp, kd, f.long(), s, m, c), "int32"), ((kp, kd, f, s[:1], m, c), "unequal"), ((kp, kd, f, s, m.int(), c), "matches"),
                        ((kp, kd, f, s, m[:1], c), "matches"), ((kp, kd, f, s, torch.zeros((2, 9, 2), dtype=torch.int64), c), "matches"),
                        ((kp, kd, f, s, m, None), "count"), ((kp, kd, f, s, m, c.long()), "count")):
        with pytest.raises(ValueError, match=match):
            lib.pose_ransac_pairs(*args, cam)
    with pytest.raises(ValueError, match="out must hold"):
        lib.pose_ransac_pairs(kp, kd, f, s, m, c, cam, out=(m,))
    with pytest.raises(ValueError, match="out `T`"):
        lib.pose_ransac_pairs(kp, kd, f, s, m, c, cam, out=(torch.zeros((2, 12)),) + (c,) * 6)
    with pytest.raises(ValueError):                                 # well-formed host tensors: refused for where they live
        lib.pose_ransac_pairs(kp, kd, f, s, m, c, cam)
    pipe = SequencePipeline.__new__(SequencePipeline)               # the argument checks need no weights and no device
    pipe.cfg = ExtractorConfig(input_size=64, num_keypoints=8)
    mm = dict(matches=m, match_count=c)
    for args, kw, match in (((kp[0], kd, f, s, mm, cam), {}, "keypoints_pixel"), ((kp, kd[:, :7], f, s, mm, cam), {}, "kp_depth"),
                            ((kp, kd, None, s, mm, cam), {}, "pair lists"), ((kp, kd, f, s, m, cam), {}, "dictionary"),
                            ((kp, kd, f, s, dict(matches=m[:1], match_count=c), cam), {}, "matches holds"),
                            ((kp, kd, f, s, mm, cam), dict(threshold=float("inf")), "threshold"), ((kp, kd, f, s, mm, cam), dict(hypotheses=0), "hypotheses"),
                            ((kp, kd, f, s, mm, cam), dict(seed=-5), "seed"), ((kp, kd, [0, 1.5], s, mm, cam), {}, "32-bit")):
        with pytest.raises(ValueError, match=match):
            pipe.estimate_poses(*args, **kw)
    toks, poses, depth = np.zeros((3, 9, 384), np.float32), np.stack([np.eye(4)] * 3), np.zeros((3, 480, 640), np.uint16)
    for kw, match in ((dict(depth=None), "needs depth"), (dict(depth=depth.astype(np.int32)), "uint16"), (dict(depth=depth[:2]), "frames"),
                      (dict(depth=depth[:, :100]), "camera describes"), (dict(depth=depth, poses=poses[:2]), "poses"),
                      (dict(depth=depth, threshold=-1.0), "threshold"), (dict(depth=depth, hypotheses=4096), "hypotheses"),
                      (dict(depth=depth, seed=-1), "seed"), (dict(depth=depth, spacing=0), "spacing"), (dict(depth=depth, spacing=3), "no pair"),
                      (dict(depth=depth, num_pairs=0), "num_pairs"), (dict(depth=depth, camera=ev.Camera(fy=float("nan"))), "camera fy")):
        with pytest.raises(ValueError, match=match):
            od.odometry(None, tokens=toks, **kw)
    with pytest.raises(ValueError, match="images_u8 or tokens"):
        od.odometry(None, depth=depth)
    result = {"frames": {"keypoints_pixel": kp}, 1: mm}
    with pytest.raises(ValueError, match="result expected"):
        od.odometry_result(None, {}, depth=depth)
    with pytest.raises(ValueError, match="no pair at spacing 2"):
        od.odometry_result(None, result, depth=depth, spacing=2)
    with pytest.raises(ValueError, match="one argument"):
        od.odometry_result(None, result, depth=depth, kp_depth=kd)
    with pytest.raises(ValueError, match="kp_depth must"):
        od.odometry_result(None, result, kp_depth=kd[:, :7])
    with pytest.raises(ValueError, match="flag"):
        harness.run_directory("/nonexistent", evaluate={"odometry": 1})
    with pytest.raises(ValueError, match="camera describes"):
        online.PoseFrameStepper(None, 48, 64, 24, 32)
    with pytest.raises(ValueError, match="hypotheses"):
        online.PoseFrameStepper(None, 48, 64, 480, 640, hypotheses=0)
    k1, d1, pm = np.zeros((5, 2), np.float32), np.zeros((480, 640), np.uint16), np.zeros((4, 2), np.int64)
    for args, kw, match in (((k1, k1, d1.astype(np.int32), d1, pm), {}, "depth1"), ((k1, k1, d1, d1[:100], pm), {}, "camera describes"),
                            ((k1, k1, d1, d1, pm), dict(hypotheses=0), "hypotheses"), ((k1, k1, d1, d1, pm), dict(threshold=-2.0), "threshold"),
                            ((k1[:, :1], k1, d1, d1, pm), {}, "keypoints"), ((k1, k1, d1, d1, pm.astype(np.float32)), {}, "matches"),
                            ((k1, k1, d1, d1, pm[:, :1]), {}, "matches")):
        with pytest.raises(ValueError, match=match):
            dropin.estimate_relative_pose(*args, **kw)
    T, mask = dropin.estimate_relative_pose(k1, k1, d1, d1, np.zeros((0, 2), np.int64))
    assert np.array_equal(T, np.eye(4)) and mask.shape == (0,) and mask.dtype == bool
