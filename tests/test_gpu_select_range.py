"""sslam_select_keypoints over the whole range include/sslam_hip.h declares, bit for bit against the CPU oracle: every nms_radius
0..8 (windows wider than the grid included) on grids from 1 x 1 to 64 x 64, one and three frames a launch, with and without the
optional idx / kp_pixel outputs; every arm of the kernel at each radius 5..8; K beyond the grid (status 1, every slot compared);
and the reference's own outputs at radius 4..8 (tests/golden/select_range.npz).  The inputs are those of
tests/select_range_cases.py; tests/test_select_range_inputs.py shows on the CPU what they reach.  No tolerances in this file."""
import os

import numpy as np
import pytest

import select_range_cases as sc
from oracle import ora

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def hip(T):
    from sslam_amd import lib
    lib.lib()
    return lib


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(T, hip, case, every_slot=False):
    """One case through the entry, once with idx / kp_pixel and once with both NULL, against the oracle.  every_slot: compare the
    frames with status 1 too (the repeat of the best point is deterministic); otherwise no frame may carry the flag."""
    sal, K, radius, pct = case["sal"], case["K"], case["radius"], case["pct"]
    okp, osc, oidx, ost = ora.select_keypoints(sal, K, radius, pct)
    if not every_slot:
        assert K <= sal.shape[1] ** 2 and not ost.any(), case["tag"]
    opx = ora.patch_to_pixel(okp)
    d = T.from_numpy(sal).cuda()
    before = hip.launch_count()
    for want_both in (True, False):
        kp, scores, idx, px, st = hip.select_keypoints(d, K, radius, pct, want_idx=want_both, want_pixel=want_both)
        tag = (case["tag"], want_both)
        assert np.array_equal(st.cpu().numpy(), ost), tag
        assert np.array_equal(bits(kp.cpu().numpy()), bits(okp)), tag
        assert np.array_equal(bits(scores.cpu().numpy()), bits(osc)), tag
        if want_both:
            assert np.array_equal(idx.cpu().numpy(), oidx), tag
            assert np.array_equal(bits(px.cpu().numpy()), bits(opx)), tag
        else:
            assert idx is None and px is None
    assert hip.launch_count() - before == 2


@pytest.mark.parametrize("g", sc.GRIDS)
def test_grid_sweep(T, hip, g):
    """Every radius 0..8 with every map kind at this grid; K <= n, so every frame of every launch is compared."""
    cases = sc.sweep_cases(g)
    assert len(cases) >= len(sc.RADII) * len(sc.KINDS)
    for case in cases:
        _check(T, hip, case)


def test_every_arm_at_radius_5_to_8(T, hip):
    cases = sc.arm_cases()
    assert {c["radius"] for c in cases} == {5, 6, 7, 8}
    for case in cases:
        _check(T, hip, case, every_slot=bool(case.get("status")))


def test_more_keypoints_than_the_grid_can_supply(T, hip):
    """K = n + 1 and K = 4096 at G = 1, 2, 5, radius 0 and 8: status and all K slots, the repeated best point included."""
    cases = sc.status_cases()
    assert len(cases) == 12
    for case in cases:
        _check(T, hip, case, every_slot=True)


def test_drop_in_selector_takes_the_declared_range(T, hip):
    """The wrapper does not narrow the header's range: the drop-in KeypointSelector passes radius 8, a window wider than the grid
    and a 1 x 1 grid through to the entry and returns the oracle's keypoints (the pipeline hands its nms_radius over unchecked)."""
    from models.keypoint_selector import KeypointSelector
    sel = KeypointSelector(384, 256)
    for g, radius in ((2, 8), (17, 8), (33, 5), (1, 3)):
        case = next(c for c in sc.sweep_cases(g) if c["radius"] == radius and c["kind"] == "uniform")
        with T.no_grad():
            kp, scores = sel.select_keypoints(T.from_numpy(case["sal"]).cuda().unsqueeze(-1), case["K"], radius, case["pct"])
        okp, osc, _, ost = ora.select_keypoints(case["sal"], case["K"], radius, case["pct"])
        assert not ost.any()
        assert np.array_equal(bits(kp.cpu().numpy()), bits(okp)) and np.array_equal(bits(scores.cpu().numpy()), bits(osc)), case["tag"]


def test_reference_goldens_at_radius_4_to_8_on_gpu(T, hip):
    """The reference's own indices and scores (tests/golden/make_golden_select_range.py) straight against the HIP kernel."""
    g = np.load(os.path.join(GOLD, "select_range.npz"))
    for s in range(int(g["count"])):
        m, (G, K, radius), pct = g[f"s{s}_map"], (int(v) for v in g["g_k_radius"][s]), float(g["pct"][s])
        kp, scores, idx, px, st = hip.select_keypoints(T.from_numpy(m[None]).cuda(), K, radius, pct)
        assert int(st[0]) == 0, s
        assert np.array_equal(idx.cpu().numpy()[0], g[f"s{s}_idx"].astype(np.int32)), (s, G, K, radius, pct)
        assert np.array_equal(bits(scores.cpu().numpy()[0]), bits(g[f"s{s}_scores"])), (s, G, K, radius, pct)
