"""CPU side of tests/test_gpu_select_range.py: the case lists of tests/select_range_cases.py reach what they are for - every
radius 0..8 against every grid, K choice and percentile, every arm of the selection kernel at each radius 5..8 - and the numpy
restatement that says so agrees with the oracle on every one of them, index for index and score bit for score bit."""
import numpy as np
import pytest

import select_range_cases as sc
from oracle import ora


def _frames(case):
    return [sc.restate(m, case["K"], case["radius"], case["pct"]) for m in case["sal"]]


def _agrees_with_oracle(case, restated):
    kp, scores, idx, st = ora.select_keypoints(case["sal"], case["K"], case["radius"], case["pct"])
    for f, r in enumerate(restated):
        assert st[f] == r["status"], (case["tag"], f)
        assert np.array_equal(idx[f], r["idx"]), (case["tag"], f, r["arm"])
        assert np.array_equal(scores[f].view(np.uint32), r["scores"].view(np.uint32)), (case["tag"], f, r["arm"])
        g = case["sal"].shape[1]
        assert np.array_equal(kp[f, :, 0], (r["idx"] % g).astype(np.float32)) and np.array_equal(kp[f, :, 1], (r["idx"] // g).astype(np.float32))


@pytest.mark.parametrize("g", sc.GRIDS)
def test_sweep_covers_the_declared_range_and_matches_the_oracle(g):
    cases = sc.sweep_cases(g)
    n = g * g
    assert {c["radius"] for c in cases} == set(sc.RADII)
    assert all(1 <= c["K"] <= n for c in cases), "no frame of the sweep may be left out of the comparison"
    assert all(c["sal"].shape[1:] == (g, g) and c["sal"].dtype == np.float32 for c in cases)
    assert {c["radius"] for c in cases if c["radius"] > g} or g >= 8
    assert any(c["radius"] == g for c in cases) or g > 8
    assert any(c["radius"] == g - 1 for c in cases) or g > 9
    for r in sc.RADII:
        mine = [c for c in cases if c["radius"] == r]
        assert {c["kind"] for c in mine} == set(sc.KINDS)
        assert {c["sal"].shape[0] for c in mine} == {1, 3}
    arms = set()
    for c in cases:
        res = _frames(c)
        assert not any(r["status"] for r in res), c["tag"]
        _agrees_with_oracle(c, res)
        arms |= {r["arm"] for r in res}
    if g >= 5:
        assert arms >= {"topk", "pad", "none"}, arms
    if g == 64:
        assert any(c["K"] == 4096 and c["radius"] == 8 and c["sal"].shape[0] == 3 for c in cases)


def test_every_radius_meets_every_k_choice_percentile_and_window_relation():
    seen = {r: (set(), set()) for r in sc.RADII}
    rel, arms = set(), set()
    for g in sc.GRIDS:
        for c in sc.sweep_cases(g):
            if g in (2, 5, 28):                              # the percentile arm is rare among random draws: arm_cases() plants it
                arms |= {x["arm"] for x in _frames(c)}
            seen[c["radius"]][0].add(c["k_name"])
            seen[c["radius"]][1].add(c["pct"])
            rel.add("above" if c["radius"] > g else "equal" if c["radius"] == g else "one_below" if c["radius"] == g - 1 else "inside")
    for r, (ks, ps) in seen.items():
        assert ks == set(sc.K_NAMES) and ps == set(sc.PCTS), (r, ks, ps)
    assert rel == {"above", "equal", "one_below", "inside"}
    assert arms == set(sc.ARMS), arms


def test_map_kinds_are_what_their_names_say():
    for g in (2, 5, 28):
        rng = np.random.Generator(np.random.PCG64(1))
        const = sc.make_map("constant", g, 3, rng)
        assert all(np.unique(f).size == 1 for f in const) and const[1].max() < 0.05 < 0.1 < const[0].min()
        one = sc.make_map("one_above_floor", g, 3, rng)
        assert all(int((f > 0.1).sum()) == 1 and int((f > 0.05).sum()) == 1 for f in one)
        twin = sc.make_map("twin_max", g, 3, rng)
        for f in twin:
            ys, xs = np.nonzero(f == f.max())
            assert len(ys) == 2 and ys[0] == ys[1] and abs(int(xs[0]) - int(xs[1])) == 1
            assert int((sc.nms(f, 8) == f.max()).sum()) == 2, "both cells of the repeated maximum survive v == mx"


def test_every_arm_is_reached_at_each_radius_5_to_8():
    cases = sc.arm_cases()
    tsels = set()
    for r in (5, 6, 7, 8):
        reached = set()
        for c in (c for c in cases if c["radius"] == r):
            res = _frames(c)
            _agrees_with_oracle(c, res)
            assert all(x["arm"] == c["arm"] for x in res), (c["tag"], [x["arm"] for x in res])
            assert all(x["status"] == c.get("status", 0) for x in res), c["tag"]
            if c["arm"] == "pct":
                assert all(x["tsel"] == c["tsel"] and 0 < x["nv"] < c["K"] for x in res), (c["tag"], res[0]["tsel"])
                tsels.add(c["tsel"])
            if c["arm"] == "pad":
                assert all(0 < x["nv"] < c["K"] for x in res)
            reached.add("status" if c.get("status") else c["arm"])
        assert reached == {"topk", "pct", "pad", "none", "status"}, (r, reached)
    assert len(tsels) >= 2


def test_status_cases_flag_exactly_the_frames_the_grid_cannot_supply():
    cases = sc.status_cases()
    assert {(c["sal"].shape[1], c["radius"]) for c in cases} == {(g, r) for g in (1, 2, 5) for r in (0, 8)}
    flagged = clean = 0
    for c in cases:
        n = c["sal"].shape[1] ** 2
        assert c["K"] in (n + 1, 4096)
        res = _frames(c)
        _agrees_with_oracle(c, res)
        for x in res:
            assert x["status"] == int(c["K"] - x["nv"] > n), c["tag"]
            assert len(x["idx"]) == c["K"]
        assert all(x["status"] for x in res) or c["K"] == n + 1
        assert res[1]["status"] == 1 and res[1]["arm"] == "none", "the frame below both floors is flagged at n + 1 too"
        flagged += sum(x["status"] for x in res)
        clean += sum(1 - x["status"] for x in res)
    assert flagged and clean


def test_restated_quantile_is_the_oracles():
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (1, 2, 3, 4, 25, 81, 784, 4096):
        v = rng.random(n).astype(np.float32)
        for q in sc.PCTS + sc.LOWER:
            assert sc.quantile32(np.sort(v), q).view(np.uint32) == ora.quantile(v, q).view(np.uint32), (n, q)
