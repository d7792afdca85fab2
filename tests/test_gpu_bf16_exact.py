"""GPU tests that hold the bf16 THROUGHPUT mode's two kernels to the exact oracle BIT FOR BIT, on order-free inputs.

tests/orderfree.py builds operands on which every product and every partial sum, in any order, is exact in fp32 (proved on the
CPU by tests/test_orderfree_inputs.py).  On such inputs the accumulation order of a bf16 MFMA kernel cannot show, the fp32
epilogues are the oracle's own, and `sslam_selector_saliency_bf16` / `sslam_refine_bf16` / `sslam_gather_refine_bf16` have to
return the oracle's bits: one mis-indexed weight or feature element, one wrong tile, column or row tail is a failure, where the
tolerance tests of test_gpu_bf16_mode.py (2e-4 after the sigmoid; self-chosen row exclusions) would let it pass.

Launch forms reached here (every SSLAM_CONVBF_* knob; the knob fixture restores each after the test):
  * halo form, image-row groups np = 5 (G = 5, 16; G = 14 at one frame), 6 (G = 14, 24, 28; G = 40 at one frame), 7 (G = 40 at two
    frames, G = 60 at one), 8 (G = 60 at two frames).  G = 128 would need np = 9, G = 160 np = 10, G = 192 np = 11: two image
    buffers of 9 x 64 rows are 165 888 bytes, above the 163 840 bytes of LDS a workgroup can have, so the instantiations for 9
    and 10 could never launch and are gone - all three grids take the default fallback (stage form, variant 2), one launch;
  * SSLAM_CONVBF_TAIL = 2: rounds of two 256-cell tiles, the rest as 128-cell tiles (one full: G = 24 x 2 frames; two full:
    G = 16 x 5; one ragged: G = 40 x 1, G = 60 x 1);
  * SSLAM_CONVBF_NO_HALO = 1 with SSLAM_CONVBF_VARIANT = 0, 1, 2; hidden size 128.
"""
import numpy as np
import pytest

import orderfree
import synth
from oracle import ora

pytestmark = pytest.mark.gpu


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


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ saliency CNN
_sel_cache = {}


def sel_case(grid, frames, hidden):
    """(feat, sd, oracle saliency) of one order-free case; the last case is kept (the knob parameters run back to back)."""
    key = (grid, frames, hidden)
    if key not in _sel_cache:
        _sel_cache.clear()
        feat, sd, logits, bounds = orderfree.selector_case(grid, grid, frames, hidden)
        want = ora.selector_saliency(feat, sd)
        # the oracle itself sits on the exact logit (CPU-proved on small grids; repeated here at this grid)
        u, inv = np.unique(logits, return_inverse=True)
        exact = np.array([ora.sigmoid(v) for v in u], np.float32)[inv].reshape(logits.shape)
        np.testing.assert_array_equal(bits(want), bits(exact))
        _sel_cache[key] = (feat, sd, want)
    return _sel_cache[key]


def run_selector_bf16(T, hip, feat, sd, hidden, packed=None, groups=None):
    """One launch of the bf16 saliency kernel.  groups: the form that has to run - the 64-row groups of the halo form, 0 for the
    stage form - checked against the library's own dispatch (sslam_selector_bf16_halo_groups, which the entry launches by)."""
    if groups is not None:
        got = hip.selector_bf16_halo_groups(feat.shape[0], feat.shape[1], hidden)
        assert got == groups, f"G={feat.shape[1]} x {feat.shape[0]}: the library launches form {got}, the case list says {groups}"
    w1p = dev(T, hip.pack_conv3x3_bf16(sd["conv.0.weight"]) if packed is None else packed).view(T.bfloat16)
    fb = hip.to_bf16(dev(T, feat))
    n0 = hip.launch_count()
    sal = hip.selector_saliency_bf16(fb, w1p, dev(T, sd["conv.0.bias"]), dev(T, sd["conv.2.weight"].reshape(-1)),
                                     dev(T, sd["conv.2.bias"]), hidden).cpu().numpy()
    assert hip.launch_count() == n0 + 1, "one launch"
    return sal


def assert_same_cells(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} cells differ from the exact oracle, first at (frame, y, x) = " \
                          f"{bad[:5].tolist()}, max |d| = {np.abs(got - want).max():.3e}"


FORMS = {"halo": {}, "halo_tail2": {"SSLAM_CONVBF_TAIL": 2},
         "stage_v0": {"SSLAM_CONVBF_NO_HALO": 1, "SSLAM_CONVBF_VARIANT": 0},
         "stage_v1": {"SSLAM_CONVBF_NO_HALO": 1, "SSLAM_CONVBF_VARIANT": 1},
         "stage_v2": {"SSLAM_CONVBF_NO_HALO": 1, "SSLAM_CONVBF_VARIANT": 2}}
# (grid, frames) -> np of the halo form; every launch checks it against the library's dispatch (run_selector_bf16)
GRIDS = {(5, 2): 5, (14, 1): 5, (14, 3): 6, (16, 5): 5, (24, 2): 6, (28, 3): 6, (40, 1): 6, (40, 2): 7, (60, 1): 7, (60, 2): 8}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("grid,frames", list(GRIDS))
def test_selector_bf16_bit_exact(T, hip, knob, grid, frames, form):
    for k, v in FORMS[form].items():
        knob(k, v)
    feat, sd, want = sel_case(grid, frames, 256)
    groups = GRIDS[(grid, frames)] if form.startswith("halo") else 0
    assert_same_cells(run_selector_bf16(T, hip, feat, sd, 256, groups=groups), want, f"G={grid} x {frames}, {form}")


@pytest.mark.parametrize("grid,frames", [(28, 2), (14, 1), (40, 1), (5, 3), (60, 1)])
def test_selector_bf16_hidden_128_bit_exact(T, hip, grid, frames):
    feat, sd, want = sel_case(grid, frames, 128)
    assert_same_cells(run_selector_bf16(T, hip, feat, sd, 128, groups=0), want, f"G={grid} x {frames}, hs=128")


@pytest.mark.parametrize("grid", [128, 160, 192])
def test_selector_bf16_large_grids_bit_exact(T, hip, grid):
    """Default knobs at grids whose halo image does not fit the LDS (np = 9, 10, 11): the fallback a caller with a large grid gets.
    One launch each, of the stage form (both asserted in run_selector_bf16)."""
    feat, sd, want = sel_case(grid, 1, 256)
    assert_same_cells(run_selector_bf16(T, hip, feat, sd, 256, groups=0), want, f"G={grid}, default knobs")


_exact_cache = {}


@pytest.mark.parametrize("throughput", [False, True])
@pytest.mark.parametrize("grid", [128, 160, 192])
def test_exact_selector_large_grids(T, hip, knob, grid, throughput):
    """The exact kernel past G = 64, random synthetic weights, against the oracle bit for bit: the few-frame form a single frame
    takes by default, and (SSLAM_CONV_LATENCY_ROWS = 0) the throughput forms and their fallbacks for images that do not fit."""
    if throughput:
        knob("SSLAM_CONV_LATENCY_ROWS", 0)
    if grid not in _exact_cache:
        _exact_cache.clear()
        sd = synth.selector_state(0)
        feat = ora.bn_tokens(synth.tokens(300 + grid, grid, 1))[0].reshape(1, grid, grid, 384)
        _exact_cache[grid] = (feat, sd, ora.selector_saliency(feat, sd))
    feat, sd, want = _exact_cache[grid]
    sal = hip.selector_saliency(dev(T, feat), dev(T, hip.pack_conv3x3(sd["conv.0.weight"])), dev(T, sd["conv.0.bias"]),
                                dev(T, sd["conv.2.weight"].reshape(-1)), dev(T, sd["conv.2.bias"]), 256).cpu().numpy()
    assert_same_cells(sal, want, f"exact kernel, G={grid}, throughput={throughput}")


# ---- mutation checks: one operand changed before upload moves exactly the cells whose receptive field contains it ----------
def packed_index(hs, n, c, tap):
    """Position of conv.0.weight[n, c, tap] in the packed bf16 image, restated from the documented layout
    [stage = chunk*9 + tap][k-step (8)][n/32][half (2)][row (32)][8] with 128-channel chunks (include/sslam_hip.h)."""
    chunk, k = divmod(c, 128)
    return (((((chunk * 9 + tap) * 8 + k // 16) * (hs // 32) + n // 32) * 2 + (k % 16) // 8) * 32 + n % 32) * 8 + k % 8


def bf16_bits(v):
    return np.uint16(np.float32(v).view(np.uint32) >> 16)


MUT_FORMS = {**FORMS, "hidden_128": {}}


@pytest.mark.parametrize("form", list(MUT_FORMS))
def test_selector_bf16_one_feature_element(T, hip, knob, form):
    """One feature element changed: the output moves in exactly the cells the oracle moves, all inside its 3 x 3 neighbourhood."""
    for k, v in MUT_FORMS[form].items():
        knob(k, v)
    hidden = 128 if form == "hidden_128" else 256
    grid, frames = 28, 3
    feat, sd, want = sel_case(grid, frames, hidden)
    f, y, x, c = 1, 9, 27, 200                      # right-hand border: the neighbourhood is cut, and row-major neighbours are not in it
    mut = feat.copy()
    mut[f, y, x, c] = np.float32(-2.0) if feat[f, y, x, c] != -2.0 else np.float32(2.0)
    want_mut = ora.selector_saliency(mut, sd)
    moved = bits(want_mut) != bits(want)
    window = np.zeros_like(moved)
    window[f, y - 1:y + 2, x - 1:x + 2] = True
    assert moved.sum() >= 4 and not (moved & ~window).any(), moved.sum()
    got, got_mut = run_selector_bf16(T, hip, feat, sd, hidden), run_selector_bf16(T, hip, mut, sd, hidden)
    np.testing.assert_array_equal(bits(got_mut) != bits(got), moved)
    assert_same_cells(got_mut, want_mut, f"{form}, mutated feature")


@pytest.mark.parametrize("form", list(MUT_FORMS))
def test_selector_bf16_one_packed_weight_element(T, hip, knob, form):
    """One element of the PACKED bf16 weight image changed (at the position the documented layout gives conv.0.weight[n, c, tap]):
    the kernel returns what the oracle returns for the state dict with that one weight changed - the cells whose tap holds a
    non-zero feature in channel c, and no others."""
    for k, v in MUT_FORMS[form].items():
        knob(k, v)
    hidden = 128 if form == "hidden_128" else 256
    grid, frames = 28, 3
    feat, sd, want = sel_case(grid, frames, hidden)
    c, tap = 333, 5                                 # tap 5: (ky, kx) = (1, 2), the right-hand neighbour
    n = hidden - 27 + int(np.flatnonzero(sd["conv.2.weight"].reshape(-1)[hidden - 27:])[0])   # a hidden channel the 1x1 layer reads
    packed = hip.pack_conv3x3_bf16(sd["conv.0.weight"])
    old = sd["conv.0.weight"][n, c, tap // 3, tap % 3]
    new = np.float32(3 / 64) if old != np.float32(3 / 64) else np.float32(-3 / 64)
    at = packed_index(hidden, n, c, tap)
    assert packed[at] == bf16_bits(old), "the packed image does not hold this weight where the documented layout puts it"
    packed = packed.copy()
    packed[at] = bf16_bits(new)
    sd_mut = dict(sd)
    sd_mut["conv.0.weight"] = sd["conv.0.weight"].copy()
    sd_mut["conv.0.weight"][n, c, tap // 3, tap % 3] = new
    want_mut = ora.selector_saliency(feat, sd_mut)
    moved = bits(want_mut) != bits(want)
    reach = np.zeros_like(moved)
    reach[:, :, :-1] = feat[:, :, 1:, c] != 0       # cells whose right-hand neighbour has a non-zero channel c
    assert moved.sum() > 100 and not (moved & ~reach).any(), moved.sum()
    got_mut = run_selector_bf16(T, hip, feat, sd, hidden, packed=packed)
    assert_same_cells(got_mut, want_mut, f"{form}, mutated packed weight")
    np.testing.assert_array_equal(bits(got_mut) != bits(run_selector_bf16(T, hip, feat, sd, hidden)), moved)


# ------------------------------------------------------------------------------------------- descriptor MLP, depth 0
# rows -> tiles of 64: 1, 2, 8, 9, 13, 24, 31 tiles, each with a full and with a ragged last tile; rows = 1.
# (frames, K) of the fused entry; the x_in entry runs the same frames * K rows
REFINE_ROWS = [(1, 1), (2, 32), (2, 50), (1, 128), (2, 256), (1, 500), (3, 192), (3, 171), (2, 416), (2, 400), (3, 512), (3, 500),
               (2, 992), (3, 650)]


def assert_same_rows(got, want, what):
    bad = np.unique(np.argwhere(bits(got) != bits(want))[:, 0])
    if bad.size:
        cols = np.unique(np.argwhere(bits(got) != bits(want))[:, 1])
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ from the exact oracle (tiles {np.unique(bad // 64).tolist()[:12]}, "
                             f"{cols.size} columns, first rows {bad[:8].tolist()}), max |d| = {np.abs(got - want).max():.3e}")


@pytest.mark.parametrize("grid", [17, 28])
@pytest.mark.parametrize("frames,K", REFINE_ROWS)
def test_refine_bf16_depth0_bit_exact(T, hip, grid, frames, K):
    """n_blocks = 0: gather, tile fill, both GEMM shapes (three column tiles per wave, then one), weight fragment order, row tail
    and XCD tile permutation of the bf16 descriptor kernel, against ora.gather + ora.refine with no tolerance."""
    feat, kp, sd, x, _, desc, _ = orderfree.refiner_case(1000 * grid + frames * K, grid, frames, K)
    want = ora.refine(ora.gather(feat, kp).reshape(-1, 384), sd, n_blocks=0)
    np.testing.assert_array_equal(bits(want), bits(desc))                     # the oracle sits on the builder's exact value
    packed = dev(T, hip.pack_refiner_bf16(ora.refiner_weight_list(sd, 0), 0))
    got = hip.refine_bf16(dev(T, x), packed, 0).cpu().numpy()
    assert_same_rows(got, want, f"refine_bf16, {frames * K} rows")
    fused = hip.gather_refine_bf16(dev(T, feat), dev(T, kp), packed, 0).cpu().numpy().reshape(-1, 128)
    assert_same_rows(fused, want, f"gather_refine_bf16, {frames} x {K} keypoints, G={grid}")


def test_refine_bf16_one_feature_element(T, hip):
    """One feature element changed: exactly the rows whose keypoint blends that cell (with a non-zero weight) move."""
    grid, frames, K = 17, 3, 300
    feat, kp, sd, x, _, _, _ = orderfree.refiner_case(5, grid, frames, K)
    f, y, xx = 1, 6, 11
    c = int(np.argmax(np.abs(sd["input_proj.weight"]).sum(0)))                # a channel input_proj reads
    mut = feat.copy()
    mut[f, y, xx, c] = np.float32(8.0) if feat[f, y, xx, c] != 8.0 else np.float32(-8.0)
    want, want_mut = (ora.refine(ora.gather(a, kp).reshape(-1, 384), sd, n_blocks=0) for a in (feat, mut))
    moved = (bits(want) != bits(want_mut)).any(-1)
    near = np.zeros((frames, K), bool)
    near[f] = (np.abs(kp[f, :, 0] - xx) < 1) & (np.abs(kp[f, :, 1] - y) < 1)
    assert moved.sum() >= 2 and not (moved & ~near.ravel()).any(), (moved.sum(), near.sum())
    packed = dev(T, hip.pack_refiner_bf16(ora.refiner_weight_list(sd, 0), 0))
    got, got_mut = (hip.gather_refine_bf16(dev(T, a), dev(T, kp), packed, 0).cpu().numpy().reshape(-1, 128) for a in (feat, mut))
    np.testing.assert_array_equal((bits(got) != bits(got_mut)).any(-1), moved)
    assert_same_rows(got_mut, want_mut, "mutated feature")


def test_refine_bf16_one_packed_weight_element(T, hip):
    """One element of the packed bf16 image of output_proj changed, at the position the documented fragment order
    [k-step][n/32][half][row (32)][8] gives output_proj.weight[n, k]: the kernel follows the oracle with that weight changed -
    column n moves (and with it the norm of the rows whose hidden unit k is active), nothing else does."""
    grid, frames, K = 28, 2, 300
    feat, kp, sd, x, _, _, _ = orderfree.refiner_case(6, grid, frames, K)
    n, k = 77, 200
    packed = hip.pack_refiner_bf16(ora.refiner_weight_list(sd, 0), 0).copy()
    base = 384 * 384 * 2 + 2 * 384 * 4                                         # input_proj: weights + two fp32 vectors
    at = ((((k // 16) * (128 // 32) + n // 32) * 2 + (k % 16) // 8) * 32 + n % 32) * 8 + k % 8
    w16 = packed[base:base + 128 * 384 * 2].view(np.uint16)
    old = sd["output_proj.weight"][n, k]
    new = np.float32(2.0) if old != 2.0 else np.float32(-2.0)
    assert w16[at] == bf16_bits(old)
    w16[at] = bf16_bits(new)
    sd_mut = dict(sd)
    sd_mut["output_proj.weight"] = sd["output_proj.weight"].copy()
    sd_mut["output_proj.weight"][n, k] = new
    want, want_mut = ora.refine(x, sd, n_blocks=0), ora.refine(x, sd_mut, n_blocks=0)
    hid = np.maximum(x.astype(np.float64) @ sd["input_proj.weight"].astype(np.float64).T + sd["input_proj.bias"], 0)
    moved = (bits(want) != bits(want_mut)).any(-1)
    np.testing.assert_array_equal(moved, hid[:, k] > 0)
    assert 20 < moved.sum() < moved.size
    got_mut = hip.refine_bf16(dev(T, x), dev(T, packed), 0).cpu().numpy()
    assert_same_rows(got_mut, want_mut, "mutated packed output_proj weight")
