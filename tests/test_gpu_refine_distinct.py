"""The distinct-row work list of the fused gather + descriptor MLP (sslam_gather_refine_ws): every distinct keypoint of a
frame runs through the MLP once, the repeated slots are copied.  Bar: BIT-EXACT against the CPU oracle
ora.refine(ora.gather(feat, kp), rsd) and against the direct launch of the same library, with the output buffer pre-filled
with a sentinel in every case; the device-side distinct counts equal the number of distinct coordinate bit patterns.

Run on the GPU box: python -m pytest tests/test_gpu_refine_distinct.py -m gpu -q
"""
import numpy as np
import pytest

import synth
from oracle import ora

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)
KNOB = "SSLAM_REFINE_DISTINCT"
ONE_ROUND_ROWS = 256 * 3 * 32         # the launches up to this size stay on the direct form (one round of MLP workgroups)


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


@pytest.fixture(scope="module")
def rsd():
    return synth.refiner_state(0)


@pytest.fixture(scope="module")
def packed(T, hip, rsd):
    return T.from_numpy(hip.pack_refiner(ora.refiner_weight_list(rsd, 2), 2)).cuda()


def features(seed, grid, frames):
    return ora.bn_tokens(synth.tokens(seed, grid, frames))[0].reshape(frames, grid, grid, 384)


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.nonzero((g != w).any(axis=-1).ravel())[0]
        raise AssertionError(f"{what}: {bad.size} of {g.size // g.shape[-1]} rows differ; first rows {bad[:8].tolist()}")


def distinct_per_frame(kp):
    """Number of distinct (x, y) BIT patterns in every frame."""
    keys = np.ascontiguousarray(kp, np.float32).view(np.uint64).reshape(kp.shape[0], kp.shape[1])
    return np.array([len(np.unique(k)) for k in keys])


def run(T, hip, knob, packed, feat, kp, form):
    """form 1 / 0: the work list / the direct launch, forced; None: the library's own choice.  Returns the descriptors, the
    number of kernel launches and (work list only) the device-side counts."""
    if form is not None:
        knob(KNOB, form)
    n, K = kp.shape[0], kp.shape[1]
    need = int(hip.lib().sslam_gather_refine_workspace_bytes(n, K))
    ws = T.zeros(max(need, 4 * (n + 1)), dtype=T.uint8, device="cuda")
    out = T.full((n, K, 128), float(SENTINEL), dtype=T.float32, device="cuda")
    before = hip.launch_count()
    hip.gather_refine(T.from_numpy(feat).cuda(), T.from_numpy(np.ascontiguousarray(kp)).cuda(), packed, 2, out=out, workspace=ws)
    T.cuda.synchronize()
    launches = hip.launch_count() - before
    counts = None
    if launches > 1:
        c, total = hip.gather_refine_counts(ws, n)
        counts = c.cpu().numpy()
        assert int(total.cpu()) == int(counts.sum())
    return out.cpu().numpy(), launches, counts


def check(T, hip, knob, packed, rsd, feat, kp, want_counts=None):
    """Work list against the oracle and against the direct launch; device-side counts against the coordinate bits."""
    want = ora.refine(ora.gather(feat, kp), rsd)
    got, launches, counts = run(T, hip, knob, packed, feat, kp, 1)
    assert launches == 4, "the work-list form is four launches"
    assert not (got == SENTINEL).any(), "a slot was left unwritten"
    assert_bits(got, want, "work list vs oracle")
    direct, launches, _ = run(T, hip, knob, packed, feat, kp, 0)
    assert launches == 1
    assert_bits(got, direct, "work list vs direct launch")
    assert np.array_equal(counts, distinct_per_frame(kp))
    if want_counts is not None:
        assert np.array_equal(counts, want_counts)
    return counts


def test_frames_without_duplicates(T, hip, knob, packed, rsd):
    feat = features(61, 28, 2)
    rng = np.random.Generator(np.random.PCG64(7))
    cells = np.stack([rng.permutation(28 * 28)[:500] for _ in range(2)])
    kp = np.stack([cells % 28, cells // 28], axis=-1).astype(np.float32)
    check(T, hip, knob, packed, rsd, feat, kp, want_counts=[500, 500])


@pytest.mark.parametrize("grid,K,frames", [(28, 500, 3), (40, 1024, 2)])
def test_natural_keypoints_and_device_side_counts(T, hip, knob, packed, rsd, grid, K, frames):
    """What select_keypoints emits: the count of every frame equals the number of distinct cells the oracle selected."""
    feat = features(30 + grid, grid, frames)
    sal = ora.selector_saliency(feat, synth.selector_state(0))
    kp, _, idx, st = ora.select_keypoints(sal, K)
    assert not st.any()
    want = np.array([len(np.unique(idx[f])) for f in range(frames)])
    assert (want < K).all(), "these frames end in the pad: they repeat keypoints"
    check(T, hip, knob, packed, rsd, feat, kp, want_counts=want)


def test_all_keypoints_in_one_cell(T, hip, knob, packed, rsd):
    feat = features(62, 28, 2)
    kp = np.empty((2, 100, 2), np.float32)
    kp[0], kp[1] = (5.0, 9.0), (27.0, 0.0)
    check(T, hip, knob, packed, rsd, feat, kp, want_counts=[1, 1])


def test_more_keypoints_than_cells(T, hip, knob, packed, rsd):
    """status = 1: K exceeds the cell count, the best point fills the rest."""
    feat = features(63, 16, 2)
    sal = ora.selector_saliency(feat, synth.selector_state(0))
    kp, _, idx, st = ora.select_keypoints(sal, 500)
    assert st.tolist() == [1, 1]
    check(T, hip, knob, packed, rsd, feat, kp, want_counts=[len(np.unique(i)) for i in idx])


def test_fractional_coordinates_repeated_bit_for_bit(T, hip, knob, packed, rsd):
    feat = features(64, 28, 3)
    rng = np.random.Generator(np.random.PCG64(11))
    base = (rng.random((3, 150, 2)) * 29 - 1).astype(np.float32)        # also border and out-of-range coordinates
    pick = rng.integers(0, 150, size=(3, 333))
    kp = np.stack([base[f][pick[f]] for f in range(3)])
    kp[:, :150] = base                                                   # every base point at least once
    counts = check(T, hip, knob, packed, rsd, feat, kp)
    assert (counts == 150).all()


def test_signed_zeros_are_not_merged(T, hip, knob, packed, rsd):
    feat = features(65, 28, 1)
    kp = np.array([[[0.0, 3.0], [-0.0, 3.0], [4.0, 0.0], [4.0, -0.0], [-0.0, -0.0], [0.0, 0.0], [0.0, 3.0], [-0.0, 3.0],
                    [0.0, -0.0], [-0.0, 0.0]]], np.float32)
    check(T, hip, knob, packed, rsd, feat, kp, want_counts=[8])


def test_rows_not_a_multiple_of_the_tile(T, hip, knob, packed, rsd):
    feat = features(66, 28, 3)
    sal = ora.selector_saliency(feat, synth.selector_state(0))
    kp, _, _, _ = ora.select_keypoints(sal, 37)
    kp[1, 20:] = kp[1, :17]                                              # 111 rows, 94 distinct: neither a multiple of 32
    counts = check(T, hip, knob, packed, rsd, feat, kp)
    assert counts.sum() % 32 and kp.shape[0] * kp.shape[1] % 32


def test_one_frame_one_keypoint(T, hip, knob, packed, rsd):
    feat = features(67, 28, 1)
    check(T, hip, knob, packed, rsd, feat, np.array([[[13.25, 7.5]]], np.float32), want_counts=[1])


@pytest.mark.parametrize("frames,launches", [(ONE_ROUND_ROWS // 512, 1), (ONE_ROUND_ROWS // 512 + 1, 4)])
def test_form_follows_the_row_count(T, hip, knob, packed, rsd, frames, launches):
    """No knob: a batch of exactly one round of MLP workgroups takes the direct launch, one frame more the work list."""
    K = 512
    assert (frames * K <= ONE_ROUND_ROWS) == (launches == 1)
    feat = features(68, 24, frames)
    idx = np.random.Generator(np.random.PCG64(frames)).integers(0, 24 * 24, size=(frames, K))     # cells repeat in every frame
    kp = np.stack([idx % 24, idx // 24], axis=-1).astype(np.float32)
    got, n_launches, counts = run(T, hip, knob, packed, feat, kp, None)
    assert n_launches == launches
    assert not (got == SENTINEL).any()
    assert_bits(got, ora.refine(ora.gather(feat, kp), rsd), "descriptors vs oracle")
    if launches == 4:
        assert np.array_equal(counts, [len(np.unique(i)) for i in idx])
    assert hip.workspace_bytes(frames, 24, K, 0) >= int(hip.lib().sslam_gather_refine_workspace_bytes(frames, K))


def test_entry_without_workspace_and_short_workspace_run_direct(T, hip, knob, packed, rsd):
    feat = features(69, 28, 2)
    sal = ora.selector_saliency(feat, synth.selector_state(0))
    kp, _, _, _ = ora.select_keypoints(sal, 500)
    want = ora.refine(ora.gather(feat, kp), rsd)
    knob(KNOB, 1)
    import ctypes as C
    f, k = T.from_numpy(feat).cuda(), T.from_numpy(kp).cuda()
    stream = C.c_void_p(T.cuda.current_stream().cuda_stream)
    for ws_bytes in (None, 0, 256):
        out = T.full((2, 500, 128), float(SENTINEL), dtype=T.float32, device="cuda")
        before = hip.launch_count()
        if ws_bytes is None:
            rc = hip.lib().sslam_gather_refine(f.data_ptr(), 2, 28, k.data_ptr(), 500, packed.data_ptr(), 2, out.data_ptr(), stream)
        else:
            ws = T.zeros(256, dtype=T.uint8, device="cuda")
            rc = hip.lib().sslam_gather_refine_ws(f.data_ptr(), 2, 28, k.data_ptr(), 500, packed.data_ptr(), 2, out.data_ptr(),
                                                  ws.data_ptr() if ws_bytes else None, ws_bytes, stream)
        T.cuda.synchronize()
        assert rc == 0 and hip.launch_count() - before == 1
        assert_bits(out.cpu().numpy(), want, "direct launch vs oracle")
