"""GPU tests of the depth ground truth of the scoring stage: sslam_keypoint_depth, sslam_pose_depth_nn_pairs and
sslam_match_score_known_pairs through sslam_amd.lib, SequencePipeline.keypoint_depth / pose_depth_scores,
sslam_amd.evaluation.evaluate / evaluate_result with depth=, and the two drop-in functions of evaluation.py.

Reference: the float64 restatement of tests/pose_depth_ref.py on the seeded cases of tests/pose_depth_cases.py, which
tests/test_pose_depth_cpu.py holds to their margins and to closed forms.  Integers equal; dist_sum / valid_count and dist_median
within 1e-10 px (pose_depth_ref's docstring); against the homography entry at t = 0 within 1e-9 px (two evaluation orders of one
quantity: ten roundings of 2^-53 on a coordinate below 4096 px are 5e-12 px on either side).
Every launch goes into poisoned outputs between guard bands (tests/guarded.py); inputs are compared with their host copies after
the call; launches are counted."""
import numpy as np
import pytest

import guarded
import pose_depth_cases as cases
import pose_depth_ref as dr
import pose_eval_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dev(T, a, name=None):
    """The device copy of an input; `name`, its argument in include/sslam_hip.h, places it under a guarded.Placement."""
    return guarded.device_input(T, a, name)


def _outputs(T, keys, n_pairs, n1):
    """Poisoned outputs between guard bands: {key: (whole, middle, tensor handed to the entry)}; float64 lies in an int64 layout."""
    from sslam_amd import lib
    shapes, out = lib.pose_depth_score_shapes(n_pairs, n1), {}
    for key in keys:
        shape, dt = shapes[key]
        whole, mid = guarded.guarded(T, shape, T.int64 if dt == T.float64 else dt, name=key)
        out[key] = (whole, mid, mid.view(T.float64) if dt == T.float64 else mid)
    return out


def _collect(out, what):
    for key, (whole, mid, _) in out.items():
        guarded.assert_guards(whole, mid, f"{what} {key}")
        guarded.assert_written(mid, f"{what} {key}")
    return {key: t.cpu().numpy() for key, (_, _, t) in out.items()}


def _untouched(T, what, *pairs):
    for name, (dev, host) in zip(what, pairs):
        assert np.array_equal(dev.cpu().numpy(), host, equal_nan=host.dtype.kind == "f"), f"input {name} was written"


def gather(T, c):
    from sslam_amd import lib
    dd, dk = _dev(T, c["depth"], "depth"), _dev(T, c["kp"], "kp_pixel")
    whole, mid = guarded.guarded(T, c["kp"].shape[:2], T.int32, name="kp_depth")
    n0 = lib.launch_count()
    lib.keypoint_depth(dd, dk, c["scale_x"], c["scale_y"], out=mid)
    assert lib.launch_count() - n0 == 1, "one launch"
    guarded.assert_guards(whole, mid, "keypoint_depth")
    guarded.assert_written(mid, "keypoint_depth")
    _untouched(T, ("depth", "kp_pixel"), (dd, c["depth"]), (dk, c["kp"]))
    return mid.cpu().numpy()


def depth_nn(T, c, threshold=None):
    """sslam_pose_depth_nn_pairs on a case of pose_depth_cases, one launch into poisoned, guarded outputs -> dict of numpy arrays."""
    from sslam_amd import lib
    db, dd, df, ds, dt = (_dev(T, c[key], name) for key, name in (("bank", "kp_bank"), ("depth_bank", "kp_depth_bank"), ("first", "pair_first"),
                                                                  ("second", "pair_second"), ("T", "T")))
    out = _outputs(T, lib.POSE_DEPTH_SCORE_KEYS, len(c["first"]), c["n1"])
    n0 = lib.launch_count()
    lib.pose_depth_nn_pairs(db, dd, df, ds, dt, c["cam"], c["scale_x"], c["scale_y"], c["threshold"] if threshold is None else threshold,
                            n1=c["n1"], n2=c["n2"], out=tuple(out[key][2] for key in lib.POSE_DEPTH_SCORE_KEYS))
    assert lib.launch_count() - n0 == 1, "one launch"
    _untouched(T, ("kp_bank", "kp_depth_bank", "first", "second", "T"), (db, c["bank"]), (dd, c["depth_bank"]), (df, c["first"]),
               (ds, c["second"]), (dt, c["T"]))
    return _collect(out, "pose_depth_nn_pairs")


def check_against_restatement(got, want, where):
    """got: the device's arrays for P pairs; want: pose_depth_ref's list of dicts.  Integers equal, distances within 1e-10 px."""
    for p, w in enumerate(want):
        assert got["valid_count"][p] == w["valid_count"], (where, p, int(got["valid_count"][p]), w["valid_count"])
        assert got["gt_count"][p] == w["gt_count"], (where, p, int(got["gt_count"][p]), w["gt_count"])
        assert np.array_equal(got["gt_of_row"][p], w["gt_of_row"]), (where, p)
        assert np.array_equal(got["gt_matches"][p], w["gt_matches"]), (where, p)          # zero rows past the count included
        v = max(w["valid_count"], 1)
        for key, scale in (("dist_sum", v), ("dist_median", 1)):
            a, b = got[key][p] / scale, w[key] / scale
            print(f"{where} pair {p} {key} / {scale}: device {a!r} restatement {b!r}")
            assert abs(a - b) <= dr.ABS, (where, p, key, a, b)


# ------------------------------------------------------------------------------------------------------------ 1. the gather
@pytest.mark.parametrize("index", range(7))
def test_depth_gather_equals_the_restatement(T, index):
    c = cases.gather_cases()[index]
    got = gather(T, c)
    want = dr.keypoint_depth(c["depth"], c["kp"], c["scale_x"], c["scale_y"])
    assert got.dtype == np.int32 and np.array_equal(got, want), c["name"]
    assert (got == -1).any() and (got == 0).any() and (got > 0).any(), c["name"]


# ------------------------------------------------------------------------------------------------------ 2. warp and search
@pytest.mark.parametrize("index", range(len(cases.WARP_SIZES)))
def test_warp_and_search_equal_the_restatement(T, index):
    c = cases.warp_case(index)
    got = depth_nn(T, c)
    assert got["gt_matches"].dtype == np.int64 and got["valid_count"].dtype == np.int32 and got["dist_median"].dtype == np.float64
    want = dr.pose_depth_nn_pairs(c["bank"], c["depth_bank"], c["first"], c["second"], c["T"], c["cam"], c["threshold"], c["scale_x"],
                                  c["scale_y"], c["n1"], c["n2"])
    check_against_restatement(got, want, c["name"])
    if len(c["first"]) == 8:
        for key in got:
            assert got[key][0].tobytes() == got[key][3].tobytes(), f"{c['name']} {key}: a pair listed twice gave other bytes"
        for p in (1, 6):                                                  # the absent pairs: sslam_pose_nn_pairs' rows, valid_count 0
            assert got["valid_count"][p] == 0 and got["gt_count"][p] == 0 and (got["gt_of_row"][p] == -1).all() and not got["gt_matches"][p].any()
            assert got["dist_sum"][p] == 0.0 and got["dist_median"][p] == 0.0
        assert got["valid_count"][5] == 0 and (got["gt_of_row"][5] == -2).all() and got["dist_sum"][5] == 0.0 and got["dist_median"][5] == 0.0


# ------------------------------------------------------------------------------------- 3. t = 0: the homography's ground truth
@pytest.mark.parametrize("index", range(2))
def test_without_translation_it_is_the_homography_entry(T, index):
    from sslam_amd import lib
    c = cases.homography_cases()[index]
    got = depth_nn(T, c)
    hom = lib.pose_nn_pairs(_dev(T, c["bank"]), _dev(T, c["first"]), _dev(T, c["second"]), _dev(T, c["H"]), c["threshold"])
    hom = {key: v.cpu().numpy() for key, v in zip(lib.POSE_SCORE_KEYS, hom)}
    k = c["n1"]
    assert (got["valid_count"] == k).all(), "every projection is inside the view"
    for key in ("gt_matches", "gt_count", "gt_of_row"):
        assert np.array_equal(got[key], hom[key]), (c["name"], key)
    assert 0 < got["gt_count"].min() and got["gt_count"].max() < k
    for p in range(len(c["first"])):
        for key, scale in (("dist_sum", k), ("dist_median", 1)):
            a, b = got[key][p] / scale, hom[key][p] / scale
            print(f"{c['name']} pair {p} {key} / {scale}: depth entry {a!r} homography entry {b!r} difference {abs(a - b):.3e}")
            assert abs(a - b) <= 1e-9, (c["name"], p, key, a, b)


# ----------------------------------------------------------------------------------------------------- 4. translation is seen
def test_translation_is_seen_by_the_depth_entry_and_not_by_the_homography(T):
    from sslam_amd import lib
    c = cases.translation_case()
    got = depth_nn(T, c)                                                  # threshold 0.01 px
    valid = got["gt_of_row"][0] != -2
    assert got["valid_count"][0] == valid.sum() > 0.5 * c["n1"]
    assert got["gt_count"][0] == got["valid_count"][0], "every row with ground truth finds its partner within 0.01 px"
    assert np.array_equal(got["gt_of_row"][0][valid], np.where(valid)[0])
    hom = lib.pose_nn_pairs(_dev(T, c["bank"]), _dev(T, c["first"]), _dev(T, c["second"]), _dev(T, c["H"]), 3.0)
    at3 = depth_nn(T, c, threshold=3.0)
    n_hom, n_depth = int(hom[1].cpu()[0]), int(at3["gt_count"][0])
    print(f"0.1 m sideways at 0.5 - 5 m: rows within 3 px of a keypoint - homography (same R) {n_hom}, depth ground truth {n_depth} "
          f"of {int(got['valid_count'][0])} rows with ground truth; within 0.01 px {int(got['gt_count'][0])}")
    assert n_hom < int(got["gt_count"][0]) <= n_depth


# --------------------------------------------------------------------------------------------------------- 5. the score entry
def score(T, c, gt_of_row, count, known=True):
    from sslam_amd import lib
    host = [(c["matches"], np.int64), (c["value"], np.float32), (count, np.int32), (gt_of_row, np.int32), (c["gt_count"], np.int32)]
    ins = [_dev(T, np.asarray(a, dt), name) for (a, dt), name in zip(host, ("matches", "value", "count", "gt_of_row", "gt_count"))]
    keys = lib.MATCH_KNOWN_SCORE_KEYS if known else lib.MATCH_SCORE_KEYS
    out = _outputs(T, keys, len(count), c["n1"])
    n0 = lib.launch_count()
    (lib.match_score_known_pairs if known else lib.match_score_pairs)(*ins, out=tuple(out[key][2] for key in keys))
    assert lib.launch_count() - n0 == 1, "one launch"
    _untouched(T, ("matches", "value", "count", "gt_of_row", "gt_count"), *((d, np.asarray(a, dt)) for d, (a, dt) in zip(ins, host)))
    return _collect(out, "match_score_known_pairs" if known else "match_score_pairs")


@pytest.mark.parametrize("which", ["count", "count_neg"])
def test_score_entry_counts_unknown_rows_apart(T, which):
    c = cases.score_case()
    count = c[which]
    got = score(T, c, c["gt_of_row"], count)
    for p in range(len(count)):
        n = int(np.clip(count[p], 0, c["n1"]))
        tp, fp, fn, un, vs = dr.match_score_known(c["matches"][p, :n], c["value"][p, :n], c["gt_of_row"][p], c["gt_count"][p])
        assert (got["tp"][p], got["fp"][p], got["fn"][p], got["unknown"][p]) == (tp, fp, fn, un), (which, p)
        assert got["tp"][p] + got["fp"][p] + got["unknown"][p] == n
        assert abs(got["value_sum"][p] - vs) <= 1e-12 * max(1.0, abs(vs)), (which, p)      # float64 sums of fp32 terms
    assert got["unknown"].max() > 0 or which == "count_neg"
    plain, old = score(T, c, c["plain"], count), score(T, c, c["plain"], count, known=False)
    assert not plain["unknown"].any()
    for key in old:
        assert plain[key].tobytes() == old[key].tobytes(), f"{key}: without -2 the entry is sslam_match_score_pairs bit for bit"
    assert got["value_sum"].tobytes() == old["value_sum"].tobytes(), "value_sum covers all listed rows in the existing order"


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
E2E_THRESHOLD = 12.0        # px: the selector's keypoints sit on the 16-px patch grid, so 3 px keeps almost no row


@pytest.fixture(scope="module")
def seq(T):
    from sslam_amd import evaluation as ev
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    inp = pr.sequence_inputs()
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K), inp["selector"], inp["refiner"], device="cuda")
    toks = T.from_numpy(inp["tokens"]).cuda()
    ex = pipe.extract(toks, None)
    return dict(pipe=pipe, toks=toks, poses=inp["poses"], depth=cases.sequence_depth(), cam=ev.Camera(), ex=ex,
                kp=ex["keypoints_pixel"].cpu().numpy(), rule=MatchRule.mnn_ratio(0.9))


def host_composition(T, s, spacing, num_pairs):
    """The restatement on the device's own keypoints and M4 lists, put together by the summaries' host arithmetic."""
    from sslam_amd import evaluation as ev
    pipe, kp, cam = s["pipe"], s["kp"], s["cam"]
    sx, sy = cases.SCALE_448
    pairs = ev.pair_list(len(kp), spacing, num_pairs)
    first, second = [a for a, _ in pairs], [b for _, b in pairs]
    Tr = ev.pair_transforms(s["poses"], pairs).reshape(-1, 12)
    assert dr.gather_margin(kp, sx, sy) >= cases.MARGIN, "a keypoint on a rounding boundary of the depth gather"
    kd = dr.keypoint_depth(s["depth"], kp, sx, sy)
    case = dict(bank=kp, depth_bank=kd, first=first, second=second, T=Tr, cam=cam, threshold=E2E_THRESHOLD, scale_x=sx, scale_y=sy,
                n1=pr.SEQ_K, n2=pr.SEQ_K)
    m = cases.check_margins(case)
    assert cases.margins_ok(m), f"the sequence sits on a decision at this threshold, choose another: {m}"
    want = dr.pose_depth_nn_pairs(kp, kd, first, second, Tr, cam, E2E_THRESHOLD, sx, sy)
    mm = pipe.match_pairs(s["ex"]["descriptors"], s["ex"]["scores"], first=first, second=second, rule=s["rule"])
    mt, val, cnt = (mm[key].cpu().numpy() for key in ("matches", "value", "match_count"))
    rows = [dr.match_score_known(mt[p, :cnt[p]], val[p, :cnt[p]], w["gt_of_row"], w["gt_count"]) for p, w in enumerate(want)]
    st = dict(num_keypoints=pr.SEQ_K, match_count=cnt, **{key: [w[key] for w in want] for key in ("gt_count", "valid_count", "dist_sum", "dist_median")},
              **{key: [r[i] for r in rows] for i, key in enumerate(("tp", "fp", "fn", "unknown", "value_sum"))})
    return kd, want, ev.depth_repeatability_summary(st, "synthetic"), ev.depth_descriptor_quality_summary(st, "synthetic")


def same_summary(got, want, what):
    assert list(got) == list(want), what
    for key in got:
        if key == "all_results":
            assert len(got[key]) == len(want[key])
            for p, (a, b) in enumerate(zip(got[key], want[key])):
                same_summary(a, b, f"{what} pair {p}")
        elif isinstance(want[key], str) or isinstance(want[key], (int, np.integer)):
            assert got[key] == want[key], (what, key, got[key], want[key])
        elif "distance" in key and "match" not in key:
            assert abs(got[key] - want[key]) <= dr.ABS, (what, key, got[key], want[key])
        else:
            assert abs(got[key] - want[key]) <= 1e-12 * max(1.0, abs(want[key])), (what, key, got[key], want[key])


@pytest.mark.parametrize("spacing,num_pairs", [(1, 50), (5, 4)])
def test_evaluate_with_depth_equals_the_host_composition(T, seq, spacing, num_pairs):
    from sslam_amd import evaluation as ev
    from sslam_amd.harness import StreamingSequence
    s = seq
    kd, want, rep, dq = host_composition(T, s, spacing, num_pairs)
    n = len(want) + spacing
    got_kd = ev.gather_keypoint_depth(s["pipe"], s["depth"], s["ex"]["keypoints_pixel"], n).cpu().numpy()
    assert np.array_equal(got_kd[:n], kd[:n]) and (got_kd[n:] == -1).all()
    assert (kd == 0).any() and (kd > 0).any(), "the band without measurement is under some keypoint"
    kw = dict(spacing=spacing, num_pairs=num_pairs, threshold=E2E_THRESHOLD, sequence="synthetic", depth=s["depth"], camera=s["cam"])
    got = ev.evaluate(s["pipe"], None, s["poses"], tokens=s["toks"], **kw)
    print(f"spacing {spacing}: mean repeatability {got['repeatability']['mean_repeatability']:.4f}, valid keypoints per pair "
          f"{[r['valid_keypoints'] for r in got['repeatability']['all_results']]}, unknown matches per pair "
          f"{[r['num_unknown_matches'] for r in got['descriptor_quality']['all_results']]}")
    same_summary(got["repeatability"], rep, f"spacing {spacing} repeatability")
    same_summary(got["descriptor_quality"], dq, f"spacing {spacing} descriptor quality")
    assert 0 < min(r["valid_keypoints"] for r in rep["all_results"]) and max(r["valid_keypoints"] for r in rep["all_results"]) < pr.SEQ_K
    assert sum(r["num_unknown_matches"] for r in dq["all_results"]) > 0 and sum(r["fp"] for r in dq["all_results"]) > 0
    tensor = ev.evaluate(s["pipe"], None, s["poses"], tokens=s["toks"], **dict(kw, depth=T.from_numpy(s["depth"]).cuda()))
    result = StreamingSequence(s["pipe"], (1, 5), rule=s["rule"]).run(s["toks"])
    again = ev.evaluate_result(s["pipe"], result, s["poses"], **kw)
    for part in ("repeatability", "descriptor_quality"):
        assert repr(got[part]) == repr(tensor[part]), f"{part}: a device tensor of depth images gave another result"
        assert repr(got[part]) == repr(again[part]), f"{part}: evaluate and evaluate_result disagree"


def test_evaluate_without_depth_is_what_it_was(T, seq):
    from sslam_amd import evaluation as ev
    s, g = seq, pr.sequence("seq_s5")
    got = ev.evaluate(s["pipe"], None, s["poses"], spacing=g["spacing"], num_pairs=g["num_pairs"], tokens=s["toks"], sequence="synthetic")
    pr.check_summary(got["repeatability"], g["rep_summary"], g["rep_results"], pr.REP_SUMMARY_KEYS, pr.REP_RESULT_KEYS, True, "no depth")
    pr.check_summary(got["descriptor_quality"], g["dq_summary"], g["dq_results"], pr.DQ_SUMMARY_KEYS, pr.DQ_RESULT_KEYS, True, "no depth")
    none = ev.evaluate(s["pipe"], None, s["poses"], spacing=g["spacing"], num_pairs=g["num_pairs"], tokens=s["toks"], sequence="synthetic",
                       depth=None, camera=None)
    assert repr(none) == repr(got)


def test_drop_in_functions_equal_the_restatement(T, seq):
    import evaluation as dropin
    from sslam_amd import evaluation as ev
    s = seq
    sx, sy = cases.SCALE_448
    a, b = 2, 7
    k1 = (s["kp"][a] * np.array([sx, sy])).astype(np.float32)[:400]      # the reference's convention: keypoints in image pixels
    k2 = (s["kp"][b] * np.array([sx, sy])).astype(np.float32)
    Trel = ev.relative_transform(s["poses"][a], s["poses"][b])
    assert dr.gather_margin(k1) >= cases.MARGIN
    kd = dr.keypoint_depth(s["depth"][a:a + 1], k1[None])[0]
    m = dr.margins(k1, k2, kd, Trel[:3].reshape(12), s["cam"], E2E_THRESHOLD)
    assert cases.margins_ok(m), m
    w = dr.pose_depth_nn(k1, k2, kd, Trel[:3].reshape(12), s["cam"], E2E_THRESHOLD)
    for conv in (lambda x: x, lambda x: T.from_numpy(x).cuda()):
        r = dropin.compute_repeatability_depth(conv(k1), conv(k2), conv(s["depth"][a]), conv(Trel), s["cam"], threshold=E2E_THRESHOLD)
        assert list(r) == ["repeatability", "repeatable_count", "total_keypoints", "valid_keypoints", "mean_nn_distance", "median_nn_distance"]
        assert (r["repeatable_count"], r["total_keypoints"], r["valid_keypoints"]) == (w["gt_count"], 400, w["valid_count"])
        assert r["repeatability"] == w["gt_count"] / w["valid_count"] and 0 < w["gt_count"] < w["valid_count"] < 400
        assert abs(r["mean_nn_distance"] - w["dist_sum"] / w["valid_count"]) <= dr.ABS and abs(r["median_nn_distance"] - w["dist_median"]) <= dr.ABS
        gt = dropin.compute_ground_truth_matches_depth(conv(k1), conv(k2), conv(s["depth"][a]), conv(Trel), s["cam"], E2E_THRESHOLD)
        assert isinstance(gt, np.ndarray if isinstance(conv(k1), np.ndarray) else T.Tensor)
        gt = gt if isinstance(gt, np.ndarray) else gt.cpu().numpy()
        assert gt.dtype == np.int64 and np.array_equal(gt, w["gt_matches"][:w["gt_count"]])


def test_a_captured_replay_equals_the_direct_launches(T, seq):
    """The gather, the nearest-point launch and the score launch in ONE single-stream graph, replayed once."""
    from sslam_amd import evaluation as ev
    from sslam_amd import lib
    s = seq
    pipe, kp = s["pipe"], s["ex"]["keypoints_pixel"]
    pairs = ev.pair_list(len(s["kp"]), 5, 4)
    first, second = (T.tensor(v, dtype=T.int32, device="cuda") for v in ([a for a, _ in pairs], [b for _, b in pairs]))
    Tr = T.from_numpy(ev.pair_transforms(s["poses"], pairs).reshape(-1, 12)).cuda()
    depth = T.from_numpy(s["depth"]).cuda()
    mm = pipe.match_pairs(s["ex"]["descriptors"], s["ex"]["scores"], first=first, second=second, rule=s["rule"])
    sx, sy = pipe.depth_scales(s["cam"])

    def launches(kd, nn, sc):
        lib.keypoint_depth(depth, kp, sx, sy, out=kd)
        lib.pose_depth_nn_pairs(kp, kd, first, second, Tr, s["cam"], sx, sy, E2E_THRESHOLD, out=nn)
        lib.match_score_known_pairs(mm["matches"], mm["value"], mm["match_count"], nn[2], nn[1], out=sc)

    def buffers():
        sh = lib.pose_depth_score_shapes(len(pairs), pr.SEQ_K)
        return (T.full(tuple(kp.shape[:2]), -5, dtype=T.int32, device="cuda"),
                tuple(T.full(sh[key][0], -5, dtype=sh[key][1], device="cuda") for key in lib.POSE_DEPTH_SCORE_KEYS),
                tuple(T.full(sh[key][0], -5, dtype=sh[key][1], device="cuda") for key in lib.MATCH_KNOWN_SCORE_KEYS))
    direct, out = buffers(), buffers()
    launches(*direct)
    T.cuda.synchronize()
    graph = T.cuda.CUDAGraph()
    n0 = lib.launch_count()
    with T.cuda.graph(graph):
        launches(*out)
    assert lib.launch_count() - n0 == 3, "three launches"
    for t in (out[0],) + out[1] + out[2]:
        t.fill_(-5)                                                       # what the capture may have written is gone
    graph.replay()
    T.cuda.synchronize()
    names = ("kp_depth",) + lib.POSE_DEPTH_SCORE_KEYS + lib.MATCH_KNOWN_SCORE_KEYS
    for key, a, b in zip(names, (direct[0],) + direct[1] + direct[2], (out[0],) + out[1] + out[2]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{key}: the replayed capture gave other bytes"
    assert int(direct[1][3].min()) > 0 and int(direct[2][3].sum()) > 0, "rows with ground truth and unknown matches were there to compare"


def test_run_directory_scores_with_the_depth_pngs(T, tmp_path):
    """run_directory(evaluate={"depth": True}) on a written TUM tree: the 'evaluation' entry equals evaluate_result with the
    depth images and the camera the sequence's name selects."""
    import synth
    from sslam_amd import evaluation as ev
    from sslam_amd.harness import run_directory
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    from sslam_amd.tum import TUMSequence, camera_for
    name, g, k = "rgbd_dataset_freiburg1_desk", 5, 12
    synth.write_tum_sequence(str(tmp_path / name))
    tum = TUMSequence(str(tmp_path), name)
    n = len(tum)
    depth = tum.load_depth_raw(range(n))
    cam = ev.Camera(fx=517.3 / 20, fy=516.5 / 20, cx=318.6 / 20, cy=255.3 / 20, width=32, height=24)      # the fixture's frames are 32 x 24
    pipe = SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    toks = T.from_numpy(synth.token_sequence(n, g)).cuda()
    kw = dict(pipe=pipe, tokens_fn=lambda a, b: toks[a:b], chunk=4, decode_workers=2)
    got = run_directory(str(tmp_path), name, (1, 3), evaluate=dict(num_pairs=4, threshold=20.0, depth=True, camera=cam), **kw)
    assert set(got["evaluation"]) == {1, 3}
    for sp in (1, 3):
        direct = ev.evaluate_result(pipe, got, tum.poses, spacing=sp, num_pairs=4, threshold=20.0, sequence=name, depth=depth, camera=cam)
        assert repr(got["evaluation"][sp]) == repr(direct)
        assert "valid_keypoints" in got["evaluation"][sp]["repeatability"]["all_results"][0]
        assert "pairs_without_ground_truth" in got["evaluation"][sp]["descriptor_quality"]
    assert camera_for(name).fx == 517.3
    with pytest.raises(ValueError, match="camera describes"):          # the name's 640 x 480 camera does not fit 32 x 24 frames
        run_directory(str(tmp_path), name, (1,), evaluate=dict(num_pairs=4, depth=True), **kw)
