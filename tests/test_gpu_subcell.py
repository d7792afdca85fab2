"""GPU tests of sub-cell keypoint localisation: sslx_subcell_keypoints of libsslam_ext.so through sslam_amd.lib, and every host
layer that carries the refined keypoints - SequencePipeline.extract, the steppers of sslam_amd.online, evaluation.evaluate,
odometry.odometry, the two drop-ins.

Reference: tests/subcell_ref.py, the header restated in numpy float32.  Every comparison is of BYTES: the feature sets no
tolerance anywhere.  Every launch goes into poisoned outputs between guard bands, from inputs between bands of NaN bits
(tests/guarded.py); inputs are compared with their host copies after the call; launches are counted."""
import ctypes as C

import numpy as np
import pytest

import ext_table as et
import guarded
import subcell_cases as sc
import subcell_ref as ref

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = ("kp_xy_sub", "kp_pixel_sub", "flags")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _same(got, want, what):
    for key, g, w in zip(KEYS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key)
        bad = np.flatnonzero(g.reshape(-1).view(np.uint32) != w.reshape(-1).view(np.uint32))
        assert bad.size == 0, f"{what}: {key} differs from the restatement in {bad.size} elements, the first at flat index {bad[0]}: " \
                              f"{g.reshape(-1)[bad[0]]!r} for {w.reshape(-1)[bad[0]]!r}"


def run(T, sal, idx, what):
    """One guarded launch -> (kp_xy_sub, kp_pixel_sub, flags) as numpy.  Under a guarded.Placement every operand takes its place."""
    from sslam_amd import lib
    n, k = idx.shape
    ws, ds = guarded.guarded_input(T, sal, name="sal")
    wi, di = guarded.guarded_input(T, idx, name="idx")
    outs = [guarded.guarded(T, shape, dt, name=name) for name, (shape, dt) in zip(KEYS, lib.subcell_shapes(n, k).values())]
    n0, m0 = lib.ext_launch_count(), lib.launch_count()
    back = lib.subcell_keypoints(ds, di, out=tuple(mid for _, mid in outs))
    assert lib.ext_launch_count() - n0 == 1 and lib.launch_count() == m0, "one launch, of the second library"
    assert all(b is mid for b, (_, mid) in zip(back, outs))
    for name, (whole, mid) in zip(KEYS, outs):
        guarded.assert_guards(whole, mid, f"{what} {name}")
        guarded.assert_written(mid, f"{what} {name}")
    guarded.assert_guards(ws, ds, f"{what} sal")
    guarded.assert_guards(wi, di, f"{what} idx")
    assert np.array_equal(ds.cpu().numpy().view(np.uint32), sal.view(np.uint32)) and np.array_equal(di.cpu().numpy(), idx), "an input was written"
    return tuple(mid.cpu().numpy() for _, mid in outs)


# n_frames, G, K: the grids 1, 2, 3 (no interior cell below 3), 28 and 64; K = 1, 5, 500 and 4096; n_frames * K = 255, 256 and 257
# around one workgroup
SHAPES = [(1, 1, 1), (3, 1, 5), (1, 2, 1), (3, 2, 5), (1, 3, 5), (3, 3, 1), (1, 28, 1), (1, 28, 500), (3, 28, 500), (3, 64, 5),
          (1, 64, 4096), (3, 28, 85), (1, 28, 256), (2, 28, 128), (1, 28, 257)]


def _field(n, g, k, seed):
    """A random field with bumps, and idx: random cells, the cells of the largest values among them."""
    rng = np.random.default_rng(seed)
    sal = rng.random((n, g, g), dtype=F)
    for f in range(n):
        sal[f] = np.maximum(sal[f], ref.bump_field(g, rng.uniform(0, g - 1), rng.uniform(0, g - 1), 1.0))
    idx = rng.integers(0, g * g, (n, k)).astype(np.int32)
    top = np.argsort(-sal.reshape(n, -1), axis=1, kind="stable")[:, :max(1, k // 2)].astype(np.int32)
    idx[:, :top.shape[1]] = top
    return sal, idx


@pytest.mark.parametrize("n,g,k", SHAPES)
def test_shapes_equal_the_restatement(T, n, g, k):
    sal, idx = _field(n, g, k, 100 * g + k)
    got = run(T, sal, idx, f"{n} x {g} x {k}")
    want = ref.subcell_keypoints(sal, idx)
    _same(got, want, f"{n} frames, G = {g}, K = {k}")
    if g >= 28 and k >= 85:
        assert (want[2] == 3).any() and (want[2] == 0).any(), "the shape refines some keypoints on both axes and leaves some"
    if g <= 2:
        assert (want[2] == 0).all(), "no interior cell: nothing is refined"


CASES = sc.cases()


@pytest.mark.parametrize("index", range(len(CASES)))
def test_planted_cases_equal_the_restatement(T, index):
    case = CASES[index]
    sc.check_decisions(case)
    _same(run(T, case["sal"], case["idx"], case["name"]), ref.subcell_keypoints(case["sal"], case["idx"]), case["name"])


@pytest.fixture(scope="module")
def seq(T):
    import pose_depth_cases
    import pose_eval_ref as pr
    import synth
    from sslam_amd import evaluation as ev
    from sslam_amd.pipeline import ExtractorConfig, MatchRule, SequencePipeline
    inp = pr.sequence_inputs()
    kw = dict(input_size=16 * pr.SEQ_GRID, num_keypoints=pr.SEQ_K)
    make = lambda **more: SequencePipeline(ExtractorConfig(**kw, **more), inp["selector"], inp["refiner"], device="cuda")
    toks = T.from_numpy(inp["tokens"]).cuda()
    imgs = T.from_numpy(synth.image_sequence(pr.SEQ_FRAMES, 48, 64)).cuda()
    off, sub = make(), make(subcell=True)
    return dict(off=off, sub=sub, make=make, toks=toks, imgs=imgs, poses=inp["poses"], depth=pose_depth_cases.sequence_depth(), cam=ev.Camera(),
                rule=MatchRule.mnn_ratio(0.9), k=pr.SEQ_K, g=pr.SEQ_GRID, ex_off=off.extract(toks, imgs), ex_sub=sub.extract(toks, imgs))


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_the_real_path_equals_the_restatement(T, seq):
    """saliency and idx as pipe.extract leaves them on synthetic tokens, G = 28, K = 500."""
    sal, idx = seq["ex_off"]["saliency"][:3].cpu().numpy(), seq["ex_off"]["idx"][:3].cpu().numpy()
    want = ref.subcell_keypoints(sal, idx)
    _same(run(T, sal, idx, "real path"), want, "real path")
    fl = want[2]
    print(f"real path: of {fl.size} keypoints {int((fl == 3).sum())} refined on both axes, {int((fl == 1).sum())} on x only, "
          f"{int((fl == 2).sum())} on y only, {int((fl == 0).sum())} on neither")
    # a frame's NMS survivors are few beside K = 500: the pad arm fills the list with non-maxima, which stay where they are
    assert (fl == 3).any() and (fl == 0).any() and (fl & ref.FLAG_RANGE == 0).all()
    cell = np.stack([idx % 28, idx // 28], -1).astype(F)
    assert np.abs(want[0] - cell).max() <= 0.5 and (np.abs(want[0] - cell) > 0).any()


@pytest.mark.parametrize("mode", ["lo", "hi"])
def test_every_pointer_at_its_least_alignment(T, mode):
    """Each operand at the alignment include/sslam_ext.h states and no better, just past and just before a 256-byte boundary:
    the same bytes as the aligned launch."""
    sal, idx = _field(3, 28, 85, 5)
    want = ref.subcell_keypoints(sal, idx)
    with guarded.placed(guarded.Placement(et.ALIGN["sslx_subcell_keypoints"], mode)) as p:
        got = run(T, sal, idx, f"placed {mode}")
    assert sorted(r["name"] for r in p.made) == sorted(et.ALIGN["sslx_subcell_keypoints"])
    for r in p.made:
        a = r["align"]
        assert r["middle"].data_ptr() % 256 == (a if mode == "lo" else 256 - a), r["name"]
    _same(got, want, f"placed {mode}")


def _raw_call(T, ptrs, n, g, k):
    from sslam_amd import lib
    return lib.ext().sslx_subcell_keypoints(ptrs[0], n, g, ptrs[1], k, ptrs[2], ptrs[3], ptrs[4], C.c_void_p(T.cuda.current_stream().cuda_stream))


def test_every_refusal_comes_before_the_launch_and_writes_nothing(T):
    from sslam_amd import lib
    n, g, k = 2, 4, 5
    sal, idx = _field(n, g, k, 9)
    _, ds = guarded.guarded_input(T, sal)
    _, di = guarded.guarded_input(T, idx)
    outs = [guarded.guarded(T, shape, dt) for shape, dt in lib.subcell_shapes(n, k).values()]
    base = [ds.data_ptr(), di.data_ptr()] + [mid.data_ptr() for _, mid in outs]
    aligns = list(et.ALIGN["sslx_subcell_keypoints"].values())
    refusals = []
    for i in range(5):
        refusals.append((f"NULL pointer {i}", [None if j == i else C.c_void_p(v) for j, v in enumerate(base)], (n, g, k), lib.E_INVALID))
        refusals.append((f"pointer {i} at half its alignment", [C.c_void_p(v + (aligns[j] // 2 if j == i else 0)) for j, v in enumerate(base)],
                         (n, g, k), lib.E_INVALID))
    ok = [C.c_void_p(v) for v in base]
    for shape in ((0, g, k), (-1, g, k), (n, 0, k), (n, -3, k), (n, g, 0), (n, g, -1)):
        refusals.append((f"sizes {shape}", ok, shape, lib.E_INVALID))
    for shape in ((n, 65, k), (n, 2 ** 16, k), (n, g, 4097), (2 ** 20, g, 4096), (2 ** 31 - 1, g, 2)):
        refusals.append((f"sizes {shape}", ok, shape, lib.E_UNSUPPORTED))
    n0 = lib.ext_launch_count()
    for what, ptrs, shape, code in refusals:
        assert _raw_call(T, ptrs, *shape) == code, what
    T.cuda.synchronize()
    assert lib.ext_launch_count() == n0, "a refusal launched"
    for name, (whole, mid) in zip(KEYS, outs):
        assert bool((whole.view(T.int32) == guarded.SENTINEL).all()), f"a refusal wrote {name}"
    # the same pointers with the sizes they were made for: accepted, one launch
    assert _raw_call(T, ok, n, g, k) == lib.OK and lib.ext_launch_count() == n0 + 1
    # the wrapper's own refusals, on device tensors, before the library is called
    with pytest.raises(ValueError):
        lib.subcell_keypoints(ds, di[:1])
    with pytest.raises(ValueError):
        lib.subcell_keypoints(ds, di, out=(outs[0][1], outs[1][1], outs[2][1][:1]))
    with pytest.raises(ValueError, match="different devices|CUDA"):
        lib.subcell_keypoints(ds, di.cpu())
    assert lib.ext_launch_count() == n0 + 1


# ------------------------------------------------------------------------------------------------------------------ the layers
def test_subcell_leaves_every_other_output_as_it_was(T, seq):
    from sslam_amd import lib
    s = seq
    a, b = s["ex_off"], s["ex_sub"]
    assert list(b) == list(a) + list(lib.SUBCELL_KEYS)
    for key in a:
        assert _bytes_equal(a[key], b[key]), f"extract: {key} changed under subcell=True"
    want = ref.subcell_keypoints(a["saliency"].cpu().numpy(), a["idx"].cpu().numpy())
    _same(tuple(b[key].cpu().numpy() for key in lib.SUBCELL_KEYS), want, "extract")
    assert s["sub"].geometry_keypoints(b) is b["keypoints_subpixel"] and s["off"].geometry_keypoints(a) is a["keypoints_pixel"]
    first, second = [0, 1, 5, -1], [1, 2, 0, 3]
    for rule in (None, s["rule"]):
        kw = {} if rule is None else {"rule": rule}
        m_off, m_sub = s["off"].match(a["descriptors"], a["scores"], a["intensity"], **kw), s["sub"].match(b["descriptors"], b["scores"], b["intensity"], **kw)
        p_off = s["off"].match_pairs(a["descriptors"], a["scores"], a["intensity"], first=first, second=second, **kw)
        p_sub = s["sub"].match_pairs(b["descriptors"], b["scores"], b["intensity"], first=first, second=second, **kw)
        for got, was, what in ((m_sub, m_off, "match"), (p_sub, p_off, "match_pairs")):
            assert list(got) == list(was)
            for key in was:
                assert _bytes_equal(was[key], got[key]), f"{what}: {key} changed under subcell=True"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_subcell_descriptors_are_the_gather_at_the_refined_keypoints(T, seq, precision):
    from sslam_amd import lib
    s = seq
    pipe = s["make"](subcell=True, subcell_descriptors=True, precision=precision)
    base = s["make"](subcell=True, precision=precision)
    toks = s["toks"][:3]
    want_base = {k: v.clone() for k, v in base.extract(toks, s["imgs"][:3]).items()}
    got = {k: v.clone() for k, v in pipe.extract(toks, s["imgs"][:3]).items()}
    for key in want_base:
        if key != "descriptors":
            assert _bytes_equal(want_base[key], got[key]), f"{key} changed under subcell_descriptors=True"
    assert not _bytes_equal(want_base["descriptors"], got["descriptors"]), "the descriptors are gathered elsewhere"
    if precision == "fp32":
        feat = pipe.features(toks)
        by_hand = lib.gather_refine(feat, got["keypoints_subpatch"], pipe.refiner.packed, pipe.refiner.n_blocks)
    else:
        feat, _ = pipe.features(toks, bf16_copy=True)
        by_hand = lib.gather_refine_bf16(feat, got["keypoints_subpatch"], pipe.refiner.packed_bf16, pipe.refiner.n_blocks)
    assert _bytes_equal(by_hand, got["descriptors"])
    unrefined = (got["subcell_flags"] == 0)
    assert bool(unrefined.any()) and _bytes_equal(want_base["descriptors"][unrefined], got["descriptors"][unrefined]), \
        "a keypoint that was not refined keeps its descriptor"


@pytest.mark.parametrize("use_graph", [False, True])
def test_steppers_return_the_batch_extract(T, seq, use_graph):
    from sslam_amd import lib
    from sslam_amd.online import FrameStepper
    s = seq
    ex = s["ex_sub"]
    n = 4
    for spacings in (None, (1, 2)):
        st = FrameStepper(s["sub"], 48, 64, use_graph=use_graph, tokens_in=True, spacings=spacings)
        for i in range(n):
            n0 = lib.ext_launch_count()
            out = st.step(s["imgs"][i], s["toks"][i])
            if use_graph and i:
                assert lib.ext_launch_count() == n0, "a replayed step makes no library call"
            for key in ("keypoints_pixel", "idx", "descriptors", "intensity") + lib.SUBCELL_KEYS:
                assert _bytes_equal(out[key], ex[key][i]), f"frame {i}: {key} (graph {use_graph}, spacings {spacings})"
        if spacings is not None:
            for j in (n - 2, n - 1):
                row = st.frame(j)
                for key in lib.SUBCELL_KEYS + ("keypoints_pixel",):
                    assert _bytes_equal(row[key], ex[key][j]), f"bank row {j}: {key}"
    plain = FrameStepper(s["off"], 48, 64, use_graph=False, tokens_in=True)
    assert not set(lib.SUBCELL_KEYS) & set(plain.step(s["imgs"][0], s["toks"][0])), "a pipeline without subcell returns what it returned"


E2E = dict(threshold=12.0, hypotheses=64, seed=5)          # tests/test_gpu_pose_ransac.py's: the cell centres of the 16-px grid still pass 12 px


def _same_odometry(a, b, what):
    assert list(a) == list(b), what
    for key in a:
        if key == "pairs":
            assert a[key] == b[key], (what, key)
        elif isinstance(a[key], dict) or a[key] is None:
            assert repr(a[key]) == repr(b[key]), (what, key)
        else:
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (what, key)


def test_odometry_and_evaluate_read_the_refined_bank(T, seq):
    from sslam_amd import evaluation as ev
    from sslam_amd import odometry as od
    from sslam_amd.harness import StreamingSequence
    s = seq
    sub, off, ex = s["sub"], s["off"], s["ex_sub"]
    n = 6
    kw = dict(camera=s["cam"], poses=s["poses"][:n], **E2E)
    got = od.odometry(sub, tokens=s["toks"][:n], depth=s["depth"][:n], rule=s["rule"], refine=True, **kw)
    # the same stages by hand, on the refined bank
    pairs = od.consecutive_pairs(n, 1, None)
    first, second = [a for a, _ in pairs], [b for _, b in pairs]
    bank = ex["keypoints_subpixel"][:n].contiguous()
    kd = ev.gather_keypoint_depth(sub, s["depth"][:n], bank, n)
    mm = sub.match_pairs(ex["descriptors"][:n], ex["scores"][:n], first=first, second=second, rule=s["rule"])
    est = sub.estimate_poses(bank, kd, first, second, mm, s["cam"], E2E["threshold"], E2E["hypotheses"], E2E["seed"])
    fin = sub.refine_poses(bank, kd, first, second, mm, s["cam"], est, E2E["threshold"])
    assert got["ransac"]["T"][:, :3].tobytes() == est["T"].cpu().numpy().reshape(-1, 3, 4).tobytes()
    assert got["T"][:, :3].tobytes() == fin["T"].cpu().numpy().reshape(-1, 3, 4).tobytes()
    assert (got["inlier_count"] >= 3).all()
    # subcell=False is the pipeline without the feature, byte for byte; and it is another result
    cells = od.odometry(sub, tokens=s["toks"][:n], depth=s["depth"][:n], rule=s["rule"], refine=True, subcell=False, **kw)
    _same_odometry(cells, od.odometry(off, tokens=s["toks"][:n], depth=s["depth"][:n], rule=s["rule"], refine=True, **kw), "subcell=False")
    assert cells["T"].tobytes() != got["T"].tobytes()
    result = StreamingSequence(sub, (1,), rule=s["rule"]).run(s["toks"][:n])
    assert set(("keypoints_subpatch", "keypoints_subpixel", "subcell_flags")) <= set(result["frames"])
    _same_odometry(od.odometry_result(sub, result, depth=s["depth"][:n], refine=True, **kw), got, "odometry_result")
    with pytest.raises(ValueError, match="subcell"):
        od.odometry(off, tokens=s["toks"][:n], depth=s["depth"][:n], subcell=True, **kw)
    # evaluate: the depth lookups and both scores on the refined bank
    ekw = dict(spacing=1, num_pairs=n - 1, threshold=E2E["threshold"], sequence="synthetic", depth=s["depth"][:n], camera=s["cam"])
    e_sub = ev.evaluate(sub, None, s["poses"][:n], tokens=s["toks"][:n], **ekw)
    Tr = T.from_numpy(np.ascontiguousarray(ev.pair_transforms(s["poses"][:n], pairs).reshape(-1, 12))).cuda()
    sc_ = sub.pose_depth_scores(bank, kd, first, second, Tr, s["cam"], E2E["threshold"], matches=mm)
    for p, r in enumerate(e_sub["repeatability"]["all_results"]):
        assert r["repeatable_count"] == int(sc_["gt_count"][p]) and r["valid_keypoints"] == int(sc_["valid_count"][p]), p
        assert r["mean_nn_distance"] == float(sc_["dist_sum"][p]) / int(sc_["valid_count"][p])
    for p, r in enumerate(e_sub["descriptor_quality"]["all_results"]):
        assert r["tp"] == int(sc_["tp"][p]) and r["fp"] == int(sc_["fp"][p]), p
    e_cells = ev.evaluate(sub, None, s["poses"][:n], tokens=s["toks"][:n], subcell=False, **ekw)
    assert repr(e_cells) == repr(ev.evaluate(off, None, s["poses"][:n], tokens=s["toks"][:n], **ekw))
    assert repr(e_cells["repeatability"]) != repr(e_sub["repeatability"])
    assert repr(ev.evaluate_result(sub, result, s["poses"][:n], **ekw)) == repr(e_sub)
    assert repr(ev.evaluate_result(sub, result, s["poses"][:n], subcell=False, **ekw)) == repr(e_cells)


@pytest.mark.parametrize("use_graph", [False, True])
def test_pose_frame_stepper_reads_the_refined_bank(T, seq, use_graph):
    from sslam_amd import odometry as od
    from sslam_amd.online import PoseFrameStepper
    s = seq
    n = 4
    kw = dict(camera=s["cam"], **E2E)
    want = od.odometry(s["sub"], tokens=s["toks"][:n], depth=s["depth"][:n], refine=True, **kw)
    cells = od.odometry(s["sub"], tokens=s["toks"][:n], depth=s["depth"][:n], refine=True, subcell=False, **kw)
    st = PoseFrameStepper(s["sub"], 48, 64, 480, 640, use_graph=use_graph, tokens_in=True, refine=True, **kw)
    depth = T.from_numpy(s["depth"]).cuda()
    for i in range(n):
        out = st.step(s["imgs"][i], depth[i], s["toks"][i])
        assert _bytes_equal(out["keypoints_subpixel"], s["ex_sub"]["keypoints_subpixel"][i])
        if i == 0:
            continue
        assert out["pose"]["T"].cpu().numpy().tobytes() == want["ransac"]["T"][i - 1][:3].tobytes(), f"frame {i}: RANSAC's pose"
        assert out["pose"]["refined"]["T"].cpu().numpy().tobytes() == want["T"][i - 1][:3].tobytes(), f"frame {i}: the refined pose"
    assert want["T"].tobytes() != cells["T"].tobytes(), "the refined bank gives another pose than the cell centres"


def test_the_sharded_runner_refuses_subcell(T, seq):
    from sslam_amd.shard import ShardedSequenceRunner
    s = seq
    ShardedSequenceRunner(s["off"].extract, s["off"].match, alloc_fn=s["off"].alloc_extract)
    with pytest.raises(ValueError, match="sub-cell"):
        ShardedSequenceRunner(s["sub"].extract, s["sub"].match, alloc_fn=s["sub"].alloc_extract)
    # a wrapped pipeline is seen by what it extracts
    sub = s["sub"]
    wrapped = ShardedSequenceRunner(lambda t, i, out=None: sub.extract(t, i, out=out), lambda d, sc_, it, sp: sub.match(d, sc_, it, sp),
                                    alloc_fn=lambda rows: sub.alloc_extract(rows, True))
    with pytest.raises(ValueError, match="sub-cell"):
        wrapped.run(s["toks"][:3], s["imgs"][:3])
    off = s["off"]
    plain = ShardedSequenceRunner(lambda t, i, out=None: off.extract(t, i, out=out), lambda d, sc_, it, sp: off.match(d, sc_, it, sp))
    assert "matches" in plain.run(s["toks"][:3], s["imgs"][:3])


def test_extract_judges_its_buffers_before_any_launch(T, seq):
    from sslam_amd import lib
    s = seq
    out = s["off"].alloc_extract(2, True)          # buffers without the three keys, handed to a pipeline with subcell
    for v in out.values():
        v.view(T.uint8).fill_(0xA5)
    n0, m0 = lib.launch_count(), lib.ext_launch_count()
    with pytest.raises(ValueError, match="keypoints_subpatch"):
        s["sub"].extract(s["toks"][:2], s["imgs"][:2], out=out)
    T.cuda.synchronize()
    assert (lib.launch_count(), lib.ext_launch_count()) == (n0, m0), "the refusal came after a launch"
    assert all(bool((v.view(T.uint8) == 0xA5).all()) for v in out.values()), "the refusal wrote into the caller's buffers"


def test_run_directory_puts_depths_scores_and_odometry_on_one_bank(T, seq, tmp_path):
    """run_directory(evaluate=...) on a pipeline with subcell: the one depth gather, the scores and the odometry all read the
    refined bank, or with "subcell": False all three the cell centres - then the result of the pipeline without the feature."""
    import synth
    from sslam_amd import evaluation as ev
    from sslam_amd import odometry as od
    from sslam_amd.harness import run_directory
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    from sslam_amd.tum import TUMSequence
    name, g, k = "rgbd_dataset_freiburg1_desk", 5, 12
    synth.write_tum_sequence(str(tmp_path / name))
    tum = TUMSequence(str(tmp_path), name)
    n = len(tum)
    depth = tum.load_depth_raw(range(n))
    cam = ev.Camera(fx=517.3 / 20, fy=516.5 / 20, cx=318.6 / 20, cy=255.3 / 20, width=32, height=24)      # the fixture's frames are 32 x 24
    make = lambda **more: SequencePipeline(ExtractorConfig(input_size=16 * g, num_keypoints=k, **more), synth.selector_state(0),
                                           synth.refiner_state(0), device="cuda")
    off, sub = make(), make(subcell=True)
    toks = T.from_numpy(synth.token_sequence(n, g)).cuda()
    kw = dict(tokens_fn=lambda a, b: toks[a:b], chunk=4, decode_workers=2)
    base = dict(num_pairs=4, threshold=20.0, depth=True, camera=cam, odometry=True, refine=True)
    got = run_directory(str(tmp_path), name, (1, 3), pipe=sub, evaluate=base, **kw)
    cells = run_directory(str(tmp_path), name, (1, 3), pipe=sub, evaluate=dict(base, subcell=False), **kw)
    was = run_directory(str(tmp_path), name, (1, 3), pipe=off, evaluate=base, **kw)
    assert {"keypoints_subpatch", "keypoints_subpixel", "subcell_flags"} <= set(got["frames"]) and "keypoints_subpixel" not in was["frames"]
    for sp in (1, 3):
        for choice, res in ((None, got), (False, cells)):
            direct = ev.evaluate_result(sub, res, tum.poses, spacing=sp, num_pairs=4, threshold=20.0, sequence=name, depth=depth, camera=cam,
                                        subcell=choice)
            assert repr(res["evaluation"][sp]) == repr(direct), (sp, choice)
            _same_odometry(res["odometry"][sp], od.odometry_result(sub, res, depth=depth, camera=cam, poses=tum.poses, spacing=sp, num_pairs=4,
                                                                   threshold=20.0, refine=True, subcell=choice), f"spacing {sp}, subcell {choice}")
        assert repr(cells["evaluation"][sp]) == repr(was["evaluation"][sp]), "subcell: False is the pipeline without the feature"
        _same_odometry(cells["odometry"][sp], was["odometry"][sp], f"spacing {sp}: subcell False against the pipeline without")
    assert repr(got["evaluation"]) != repr(cells["evaluation"]) and got["odometry"][1]["T"].tobytes() != cells["odometry"][1]["T"].tobytes()
    with pytest.raises(ValueError, match="subcell"):          # before the sequence is run
        run_directory(str(tmp_path), name, (1,), pipe=off, evaluate=dict(base, subcell=True), **kw)
    with pytest.raises(ValueError, match="subcell"):
        run_directory(str(tmp_path), name, (1,), pipe=sub, evaluate=dict(base, subcell="yes"), **kw)


def test_the_drop_ins_equal_the_restatement(T, seq):
    import evaluation as dropin
    from models.keypoint_selector import KeypointSelector
    a = seq["ex_off"]
    sal, idx = a["saliency"][:2].cpu().numpy(), a["idx"][:2].cpu().numpy()
    want = ref.subcell_keypoints(sal, idx)[0]
    kp = a["keypoints_patch"][:2]
    sel = KeypointSelector(hidden_dim=256).cuda()
    with T.no_grad():
        got = sel.refine_keypoints(a["saliency"][:2].unsqueeze(-1), kp)
        outside = sel.refine_keypoints(a["saliency"][:1].unsqueeze(-1), T.tensor([[[28.0, 3.0], [-1.0, 0.0]]], device="cuda"))
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert outside.cpu().numpy().tobytes() == np.zeros((1, 2, 2), F).tobytes(), "a keypoint outside the grid aliases no cell"
    odd = T.tensor([[[3.5, 3.0], [float("nan"), 2.0], [4.0, float("inf")], [5.0, 6.0]]], device="cuda")
    with T.no_grad():
        got_odd = sel.refine_keypoints(a["saliency"][:1].unsqueeze(-1), odd).cpu().numpy()
    assert got_odd[0, :3].tobytes() == np.zeros((3, 2), F).tobytes(), "a fractional, NaN or infinite keypoint is truncated to no cell"
    assert got_odd[0, 3].tobytes() == ref.subcell_keypoints(sal[:1], np.array([[6 * 28 + 5]], np.int32))[0][0, 0].tobytes()
    with pytest.raises(ValueError, match="whole cells"):          # the eager path refuses the same keypoints
        sel.refine_keypoints(a["saliency"][:1].unsqueeze(-1).requires_grad_(True), odd)
    assert dropin.refine_keypoints_subcell(a["saliency"][0], odd[0]).cpu().numpy().tobytes() == got_odd[0].tobytes()
    eager = sel.refine_keypoints(a["saliency"][:2].unsqueeze(-1).requires_grad_(True), kp)          # the autograd path, on the device
    differ = int((eager.detach().cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum())
    print(f"eager torch ops on the device: {differ} of {want.size} coordinates differ from the restatement in their bits")
    assert eager.requires_grad and differ == 0
    one = dropin.refine_keypoints_subcell(sal[0], kp[0].cpu().numpy())
    assert isinstance(one, np.ndarray) and one.tobytes() == want[0].tobytes()
    dev = dropin.refine_keypoints_subcell(a["saliency"][1], kp[1])
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == want[1].tobytes()
