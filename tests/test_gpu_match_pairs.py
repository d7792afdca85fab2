"""GPU tests of the pair-list matcher and of the online stepper over several spacings.  Everything is BIT FOR BIT: per pair the
kernels' arithmetic is that of the strided entries, so there are no tolerances anywhere in this file.

* `SequencePipeline.match_pairs` on 27 frames: every pair of the five spacings in ONE list (the single-evaluation form), a
  5-pair list (the two-pass form) and each form forced, against `match(spacing=s)` row by row and against the oracle's
  match_with_quality pair by pair; lists no strided call can express (reversed, self, duplicate, shuffled, one against ten);
  absent pairs (-1) among present ones; `lib.sim_argmax_pairs` against `lib.sim_argmax` with every optional output.
* `FrameStepper(spacings=...)`: against `StreamingSequence.run` over the same frames, with and without the captured graph, over
  a ring that wraps, against the one-spacing stepper, with the bf16 HIP ViT inside, and after the pipeline replaced its buffers.
"""
import numpy as np
import pytest

import synth
from oracle import ora

pytestmark = pytest.mark.gpu

SPACINGS = (1, 5, 10, 15, 20)
N = 27
CLI = dict(saliency_weight=0.3, min_saliency=0.5, min_descriptor_sim=0.7, min_intensity=0.15)   # tests/test_gpu_harness.py
FRAME_KEYS = ("idx", "descriptors", "intensity", "scores", "saliency", "keypoints_pixel")
MATCH_KEYS = ("matches", "quality", "match_count", "nn12", "nn21", "sim")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def pipe(T):
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    return SequencePipeline(ExtractorConfig(**CLI), synth.selector_state(0), synth.refiner_state(0), device="cuda")


@pytest.fixture(scope="module")
def seq(T, pipe):
    """27 extracted frames: the device dict, its host copy for the oracle, and match(spacing=s) for the five spacings."""
    toks = T.from_numpy(synth.token_sequence(N, 28)).cuda()
    imgs = T.from_numpy(synth.image_sequence(N)).cuda()
    ex = pipe.extract(toks, imgs)
    fr = {k: ex[k].cpu().numpy() for k in ("descriptors", "scores", "intensity")}
    strided = {s: {k: v.clone() for k, v in pipe.match(ex["descriptors"], ex["scores"], ex["intensity"], spacing=s).items()}
               for s in SPACINGS}
    return dict(toks=toks, imgs=imgs, ex=ex, fr=fr, strided=strided)


_ORACLE = {}


def _oracle_pair(fr, i, j):
    if (i, j) not in _ORACLE:
        _ORACLE[(i, j)] = ora.match_with_quality(fr["descriptors"][i], fr["descriptors"][j], fr["scores"][i], fr["scores"][j],
                                                 CLI["saliency_weight"], CLI["min_saliency"], CLI["min_descriptor_sim"],
                                                 fr["intensity"][i], fr["intensity"][j], CLI["min_intensity"])
    return _ORACLE[(i, j)]


def _match_pairs(T, pipe, seq, pairs, host_lists=False):
    first, second = [p[0] for p in pairs], [p[1] for p in pairs]
    if not host_lists:
        first, second = (T.tensor(x, dtype=T.int32, device="cuda") for x in (first, second))
    ex = seq["ex"]
    return pipe.match_pairs(ex["descriptors"], ex["scores"], ex["intensity"], first=first, second=second)


def _check_vs_oracle(res, pairs, fr):
    """Counts, index pairs and quality bits of every listed pair; the slots past the count are zero."""
    mm = {k: res[k].cpu().numpy() for k in ("matches", "quality", "match_count")}
    assert mm["match_count"].shape == (len(pairs),) and mm["matches"].dtype == np.int64
    total = 0
    for row, (i, j) in enumerate(pairs):
        want_m, want_q = _oracle_pair(fr, i, j)
        c = int(mm["match_count"][row])
        assert c == len(want_m), (row, i, j, c, len(want_m))
        assert np.array_equal(mm["matches"][row, :c], want_m), (row, i, j)
        assert np.array_equal(mm["quality"][row, :c].view(np.uint32), want_q.view(np.uint32)), (row, i, j)
        assert not mm["matches"][row, c:].any() and not mm["quality"][row, c:].view(np.uint32).any(), (row, i, j)
        total += c
    return total


def _check_vs_strided(T, res, pairs, strided):
    for row, (i, j) in enumerate(pairs):
        for key in MATCH_KEYS:
            assert T.equal(res[key][row], strided[j - i][key][i]), (key, row, i, j)


ALL_PAIRS = [(i, i + s) for s in SPACINGS for i in range(N - s)]
FIVE_PAIRS = [(3, 3 + s) for s in SPACINGS]


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("pairs", [ALL_PAIRS, FIVE_PAIRS], ids=["every_pair", "five_pairs"])
def test_every_spacing_as_one_list(T, pipe, seq, pairs, variant):
    """All pairs (i, i + s) of the five spacings in one list: 26 + 22 + 17 + 12 + 7 = 84 rows over 27 frames, which is past
    the 16 pairs from which the matcher evaluates S once; the 5-pair list evaluates it once per direction.  variant 1 / 2
    force either form on either list (SSLAM_M1_VARIANT).  Rows equal match(spacing=s), computed without any knob, and the oracle."""
    from sslam_amd import lib
    assert len(ALL_PAIRS) == 84 and len(FIVE_PAIRS) == 5
    assert lib.lib().sslam_sim_argmax_workspace_bytes(500, len(ALL_PAIRS)) > 0 == lib.lib().sslam_sim_argmax_workspace_bytes(500, 5)
    n0 = lib.launch_count()
    if variant:
        with lib.knobs(SSLAM_M1_VARIANT=variant):
            res = _match_pairs(T, pipe, seq, pairs)
    else:
        res = _match_pairs(T, pipe, seq, pairs)
    single = variant == 2 or (variant == 0 and len(pairs) >= 16)
    assert lib.launch_count() - n0 == (3 if single else 2), "one launch pair (+ the key decode of the single-evaluation form)"
    _check_vs_strided(T, res, pairs, seq["strided"])
    assert _check_vs_oracle(res, pairs, seq["fr"]) > 0


def test_host_lists_are_uploaded_once_and_give_the_same_rows(T, pipe, seq):
    a = _match_pairs(T, pipe, seq, ALL_PAIRS)
    b = _match_pairs(T, pipe, seq, ALL_PAIRS, host_lists=True)
    for key in MATCH_KEYS:
        assert T.equal(a[key], b[key]), key


_rng = np.random.default_rng(11)
UNSTRIDED = {
    "reversed": [(i + s, i) for s in SPACINGS for i in range(N - s)],
    "reversed_few": [(9, 4), (26, 6), (1, 0)],
    "self": [(4, 4)],
    "self_among_others": [(i, i) for i in range(0, N, 3)] + [(0, 1), (7, 2)] + [(i, i) for i in range(1, N, 3)],
    "listed_twice": [(2, 9), (5, 6), (2, 9)],
    "listed_twice_long": [(2, 9)] * 9 + [(i, i + 1) for i in range(12)] + [(2, 9)],
    "shuffled": [ALL_PAIRS[i] for i in _rng.permutation(len(ALL_PAIRS))],
    "one_against_ten": [(13, j) for j in (0, 2, 5, 7, 11, 14, 17, 20, 23, 26)],
    "ten_against_one": [(j, 13) for j in (0, 2, 5, 7, 11, 14, 17, 20, 23, 26)],
}


@pytest.mark.parametrize("name", sorted(UNSTRIDED))
def test_lists_no_strided_call_can_express(T, pipe, seq, name):
    pairs = UNSTRIDED[name]
    res = _match_pairs(T, pipe, seq, pairs)
    _check_vs_oracle(res, pairs, seq["fr"])
    if name.startswith("listed_twice"):
        rows = [r for r, p in enumerate(pairs) if p == (2, 9)]
        for key in MATCH_KEYS:
            assert all(T.equal(res[key][rows[0]], res[key][r]) for r in rows[1:]), key
    if name.startswith("self"):
        row = pairs.index((4, 4)) if (4, 4) in pairs else 1
        i = pairs[row][0]
        assert pairs[row] == (i, i)
        # a frame against itself: every keypoint's best is a copy of itself, and the first of equal rows wins
        d = seq["fr"]["descriptors"][i]
        first_copy = np.array([int(np.flatnonzero((d == d[k]).all(axis=1))[0]) for k in range(d.shape[0])])
        assert np.array_equal(res["nn12"][row].cpu().numpy(), first_copy) and T.equal(res["nn12"][row], res["nn21"][row])


ABSENT = {
    # two-pass form (fewer than 16 pairs) and single-evaluation form; -1 in first, in second, in both, first and last rows too
    "few": [(-1, 3), (0, 1), (2, 7), (4, -1), (-1, -1), (5, 6), (12, -1)],
    "many": [(-1, -1)] + [(i, i + 1) for i in range(8)] + [(-1, 4), (9, -1)] + [(i, i + 5) for i in range(10)] + [(3, -1), (-1, 0)],
}


@pytest.mark.parametrize("name", sorted(ABSENT))
def test_absent_pairs_give_zero_rows_and_leave_the_others_alone(T, pipe, seq, name):
    from sslam_amd import lib
    pairs = ABSENT[name]
    present = [p for p in pairs if -1 not in p]
    assert (len(pairs) >= 16) == (name == "many") == (len(present) >= 16)
    res = _match_pairs(T, pipe, seq, pairs)
    alone = _match_pairs(T, pipe, seq, present)
    _check_vs_oracle(alone, present, seq["fr"])
    row_alone = 0
    for row, p in enumerate(pairs):
        if -1 in p:
            assert int(res["match_count"][row]) == 0, (row, p)
            for key in ("matches", "quality", "nn12", "nn21", "sim"):
                assert not res[key][row].view(T.int32).any(), (key, row, p)
        else:
            for key in MATCH_KEYS:
                assert T.equal(res[key][row], alone[key][row_alone]), (key, row, p)
            row_alone += 1
    # every optional output of an absent pair is 0.0f too
    first, second = (T.tensor([p[k] for p in pairs], dtype=T.int32, device="cuda") for k in (0, 1))
    nn12, s12, nn21, s21, sec = lib.sim_argmax_pairs(seq["ex"]["descriptors"], first, second, want_s21=True, want_second=True,
                                                      workspace=pipe.workspace(0, len(pairs)))
    for row, p in enumerate(pairs):
        if -1 in p:
            for t in (nn12, s12, nn21, s21, sec):
                assert not t[row].view(T.int32).any(), (row, p)
        else:
            assert T.equal(nn12[row], res["nn12"][row]) and T.equal(nn21[row], res["nn21"][row]) and T.equal(s12[row], res["sim"][row])


@pytest.mark.parametrize("s,m", [(5, 22), (1, 5), (20, 7)])
def test_sim_argmax_pairs_equals_the_strided_entry(T, pipe, seq, s, m):
    """Library level, every optional output requested: 22 pairs take the single-evaluation form, 5 and 7 the two-pass form."""
    from sslam_amd import lib
    d = seq["ex"]["descriptors"]
    k = d.shape[1]
    want = lib.sim_argmax(d, k * lib.D_OUT, k, d[s:], k * lib.D_OUT, k, m, want_s21=True, want_second=True, workspace=pipe.workspace(0, m))
    want = [t.clone() for t in want]
    first = T.arange(0, m, dtype=T.int32, device="cuda")
    got = lib.sim_argmax_pairs(d, first, first + s, want_s21=True, want_second=True, workspace=pipe.workspace(0, m))
    for name, a, b in zip(("nn12", "s12", "nn21", "s21", "second12"), got, want):
        assert T.equal(a.view(T.int32), b.view(T.int32)), name
    lean = lib.sim_argmax_pairs(d, first, first + s, workspace=pipe.workspace(0, m))
    assert lean[3] is None and lean[4] is None
    assert all(T.equal(a.view(T.int32), b.view(T.int32)) for a, b in zip(lean[:3], want[:3]))


# ------------------------------------------------------------------------------------------------------- the online stepper
def _step_through(T, st, imgs, toks, want, spacings, use_graph, rounds=2, frame_keys=FRAME_KEYS):
    """Every step of `rounds` passes over the frames against a StreamingSequence.run result of the same frames."""
    from sslam_amd import lib
    n = imgs.shape[0]
    for rnd in range(rounds):
        for t in range(n):
            n0 = lib.launch_count()
            o = st.step(imgs[t], None if toks is None else toks[t])
            calls = lib.launch_count() - n0
            if use_graph and (rnd or t):
                assert calls == 0, "a replayed step issues no library call"
            if not use_graph:
                assert calls > 0
            for k in frame_keys:
                assert T.equal(o[k], want["frames"][k][t]), (k, t)
            assert o["pair_first"] == [t - s if t >= s else -1 for s in spacings], t
            assert o["matches"].shape == (len(spacings), 500, 2) and o["quality"].shape == (len(spacings), 500)
            assert o["match_count"].shape == (len(spacings),)
            for row, s in enumerate(spacings):
                if t < s:
                    assert o["pair_first"][row] == -1 and int(o["match_count"][row]) == 0, (t, s)
                    assert not o["matches"][row].any() and not o["quality"][row].view(T.int32).any(), (t, s)
                else:
                    for key in ("matches", "quality", "match_count"):
                        assert T.equal(o[key][row], want[s][key][t - s]), (key, t, s)
        st.reset()                                  # a second pass after reset(): no spacing has an earlier frame again


@pytest.mark.parametrize("use_graph", [False, True])
def test_stepper_over_the_five_spacings_equals_the_batched_harness(T, pipe, seq, use_graph):
    from sslam_amd.harness import StreamingSequence
    from sslam_amd.online import FrameStepper
    want = StreamingSequence(pipe, SPACINGS).run(seq["toks"], seq["imgs"])
    assert sum(int(want[1]["match_count"][i]) for i in range(N - 1)) > 0
    st = FrameStepper(pipe, 480, 640, use_graph=use_graph, tokens_in=True, spacings=SPACINGS)
    assert st.bank["descriptors"].shape == (21, 500, 128) and st.bank["keypoints_pixel"].shape == (21, 500, 2)
    with pytest.raises(ValueError, match="tokens"):
        st.step(seq["imgs"][0])
    st.reset()
    _step_through(T, st, seq["imgs"], seq["toks"], want, SPACINGS, use_graph)
    # the bank names the earlier frames of the last step's pairs
    for t in range(N):
        st.step(seq["imgs"][t], seq["toks"][t])
    for i in (N - 1, N - 5, N - 20):
        assert T.equal(st.frame(i)["keypoints_pixel"], want["frames"]["keypoints_pixel"][i]), i
        assert T.equal(st.frame(i)["descriptors"], want["frames"]["descriptors"][i]), i
    with pytest.raises(ValueError, match="bank"):
        st.frame(N - 21)


@pytest.mark.parametrize("use_graph", [False, True])
def test_stepper_ring_wraps_around(T, pipe, seq, use_graph):
    """spacings (1, 2, 5) over 13 frames: 5 ring slots + the static one, every ring slot rewritten at least twice."""
    from sslam_amd.harness import StreamingSequence
    from sslam_amd.online import FrameStepper
    sp, n = (1, 2, 5), 13
    want = StreamingSequence(pipe, sp).run(seq["toks"][:n], seq["imgs"][:n])
    st = FrameStepper(pipe, 480, 640, use_graph=use_graph, tokens_in=True, spacings=sp)
    assert st.bank["descriptors"].shape[0] == 6
    _step_through(T, st, seq["imgs"][:n], seq["toks"][:n], want, sp, use_graph)


def test_spacing_order_is_the_callers(T, pipe, seq):
    from sslam_amd.harness import StreamingSequence
    from sslam_amd.online import FrameStepper
    sp, n = (5, 1, 3), 9
    want = StreamingSequence(pipe, sp).run(seq["toks"][:n], seq["imgs"][:n])
    st = FrameStepper(pipe, 480, 640, use_graph=True, tokens_in=True, spacings=sp)
    _step_through(T, st, seq["imgs"][:n], seq["toks"][:n], want, sp, True, rounds=1)


@pytest.mark.parametrize("use_graph", [False, True])
def test_one_spacing_equals_the_legacy_stepper(T, pipe, seq, use_graph):
    from sslam_amd.online import FrameStepper
    old = FrameStepper(pipe, 480, 640, use_graph=use_graph, tokens_in=True)
    new = FrameStepper(pipe, 480, 640, use_graph=use_graph, tokens_in=True, spacings=(1,))
    for t in range(6):
        a = {k: (v.clone() if v is not None else None) for k, v in old.step(seq["imgs"][t], seq["toks"][t]).items()}
        b = new.step(seq["imgs"][t], seq["toks"][t])
        assert set(a) | {"pair_first"} == set(b)
        for k in a:
            if k in ("matches", "quality", "match_count"):
                if t == 0:
                    assert a[k] is None and not b[k].view(T.int32).any()
                else:
                    assert T.equal(a[k], b[k][0]), (k, t)
            else:
                assert T.equal(a[k], b[k]), (k, t)
        assert t == 0 or int(b["match_count"][0]) > 0


def test_stepper_over_two_spacings_with_the_bf16_vit_inside(T):
    """8 frames: the range in which a one-frame step and a batch run the same form of the bf16 ViT, so the same bits."""
    from sslam_amd.harness import StreamingSequence
    from sslam_amd.online import FrameStepper
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    from sslam_amd.vit import DinoV3ViT
    T.manual_seed(3)
    n, sp = 8, (1, 3)
    imgs = T.from_numpy(synth.image_sequence(n)).cuda()
    pv = SequencePipeline(ExtractorConfig(**CLI), synth.selector_state(0), synth.refiner_state(0), device="cuda",
                          vit=DinoV3ViT().cuda().eval(), vit_precision="bf16")
    ran = pv.run(imgs)
    want = StreamingSequence(pv, sp).run(pv.tokens_from_images(imgs), imgs)
    for k in FRAME_KEYS:
        assert T.equal(want["frames"][k], ran[k]), k
    assert T.equal(want[1]["matches"], ran["matches"]) and T.equal(want[1]["match_count"], ran["match_count"])
    for use_graph in (False, True):
        st = FrameStepper(pv, 480, 640, use_graph=use_graph, spacings=sp)
        _step_through(T, st, imgs, None, want, sp, use_graph, rounds=1)


def test_multi_spacing_graph_survives_the_pipeline_replacing_its_buffers(T):
    """The captured multi-spacing step bakes in the pipeline's scratch as the one-spacing step does.  Capture at one frame, push
    a 27-frame batch through the SAME pipeline so that it replaces its scratch, fill what the allocator got back with junk, and
    keep stepping: the replay still gives the batched rows (tests/test_gpu_harness.py covers the one-spacing path this way)."""
    from sslam_amd.harness import StreamingSequence
    from sslam_amd.online import FrameStepper
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    imgs = T.from_numpy(synth.image_sequence(N)).cuda()
    toks = T.from_numpy(synth.token_sequence(N, 28)).cuda()
    pv = SequencePipeline(ExtractorConfig(**CLI), synth.selector_state(0), synth.refiner_state(0), device="cuda")
    st = FrameStepper(pv, 480, 640, use_graph=True, tokens_in=True, spacings=SPACINGS)
    first = [{k: (v.clone() if hasattr(v, "clone") else v) for k, v in st.step(imgs[t], toks[t]).items()} for t in range(2)]
    ws_bytes = 0 if pv._ws is None else pv._ws.numel()            # (no reference kept here: the stepper's own must keep it alive)
    big = pv.run(imgs, tokens=toks)
    assert pv._ws.numel() > ws_bytes, "the batch was meant to outgrow the scratch"
    del big
    want = StreamingSequence(pv, SPACINGS).run(toks, imgs)
    T.cuda.synchronize()
    junk = [T.full((sz,), 0xA5, dtype=T.uint8, device="cuda") for sz in (1 << 12, 1 << 16, 1 << 20, 1 << 22, 1 << 24, 1 << 26) for _ in range(3)]
    T.cuda.synchronize()
    assert int(first[1]["match_count"][0]) == int(want[1]["match_count"][0]) and T.equal(first[1]["matches"][0], want[1]["matches"][0])
    from sslam_amd import lib
    for t in range(2, N):
        n0 = lib.launch_count()
        o = st.step(imgs[t], toks[t])
        assert lib.launch_count() == n0
        for k in ("idx", "descriptors", "intensity", "scores"):
            assert T.equal(o[k], want["frames"][k][t]), (k, t)
        for row, s in enumerate(SPACINGS):
            if t >= s:
                for key in ("matches", "quality", "match_count"):
                    assert T.equal(o[key][row], want[s][key][t - s]), (key, t, s)
            else:
                assert int(o["match_count"][row]) == 0
    assert all(int(j[0]) == 0xA5 and int(j[-1]) == 0xA5 for j in junk), "the replay wrote into memory it no longer owns"
