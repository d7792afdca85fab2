"""Entries run with operands past 2^31 bytes and at their stated size limits (include/sslam_hip.h, SIZE LIMITS; tests/size_table.py),
bit for bit against the CPU oracle.

An operand of that size is built on the device from 7 repeating frames plus frames of their own at the positions where an address
computation can go wrong - frame 0, the frame holding byte 2^31, the last frame of a launch group and the first of the next, the
last frame of all (tests/periodic.py).  The oracle runs on those at most 13 distinct frames only; the comparison runs on the device
over the whole output, as integer bits, and prints "0 mismatching frames of N".  After the passing comparison every case changes
one input element of the LAST frame, takes the oracle's new result for that frame and compares again: the output changes there
(the oracle's result differs and the device's equals it) and nowhere else (every other frame still equals its expectation).

Every test frees what it allocated and asserts its peak of device memory below 24 GiB.  One test at a time.

The bf16 ViT's 32-bit tile index crosses 2^31 only above 24 GiB of one operand: it has a row in tests/size_table.py, its refusal is
checked without a device, and it has no case here.  profiles/size_limits.txt holds the audit, the measured durations and peaks.
"""
import contextlib

import numpy as np
import pytest

import periodic as pd
import size_table as st
import synth
from oracle import ora

pytestmark = pytest.mark.gpu

GIB24 = 24 << 30


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def hip():
    from sslam_amd import lib
    return lib


@contextlib.contextmanager
def _memory(T, what):
    """Reset the peak, run the case, free its tensors, hold the peak below 24 GiB."""
    T.cuda.synchronize()
    T.cuda.empty_cache()
    T.cuda.reset_peak_memory_stats()
    try:
        yield
    finally:
        T.cuda.synchronize()
        peak = T.cuda.max_memory_allocated()
        T.cuda.empty_cache()
        print(f"{what}: peak {peak / 2 ** 30:.2f} GiB of device memory")
    assert peak < GIB24, f"{what}: peak {peak} bytes"


def _dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_far_end(T, name, n, marked, expected, expected_changed, run):
    """The second half of every case: `run()` returns the output for the operand whose last frame was changed; `expected_changed` is
    the oracle's result for that frame (numpy, one frame)."""
    last = pd.n_distinct(marked) - 1
    assert marked[-1] == n - 1
    old = expected[last].cpu().numpy()
    assert old.shape == expected_changed.shape and not np.array_equal(old.view(np.uint8), np.ascontiguousarray(expected_changed).view(np.uint8)), \
        f"{name}: the change of the last frame's input does not show in the oracle's output"
    out2 = run()
    bad, first = pd.mismatches(out2, expected, marked)
    assert bad == [n - 1], f"{name}: after changing the last frame's input the output differs from the old expectation in frames {bad[:8]}"
    exp2 = expected.clone()
    exp2[last] = _dev(T, expected_changed).view(exp2.dtype)
    pd.report(out2, exp2, marked, name + ", last frame changed")


# ------------------------------------------------------------------------------------------------------------------ A0
def _tables(T, hip, h, w, size, bicubic=False):
    tabs = []
    for n_in in (w, h):
        b, c, k = hip.resample_table(n_in, size, bicubic)
        tabs.append((_dev(T, b), _dev(T, c), k))
    return tabs


def _patch_rows(chw, size):
    """(d, 3, size, size) fp32 -> (d, (size/16)^2, 768) fp32 in the patch entry's order (rounded to bf16 by the caller)."""
    d, g = chw.shape[0], size // 16
    return np.ascontiguousarray(chw.reshape(d, 3, g, 16, g, 16).transpose(0, 2, 4, 1, 3, 5).reshape(d, g * g, 768))


def _a0_images(h, w, count, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(count, h, w, 3), dtype=np.uint8)


def _a0(T, hip, h, w, size, n, patch, lead, expect_cut):
    name = f"A0 {'patch' if patch else 'fp32'} {h}x{w}->{size}, {n} frames, base + {lead}"
    fb = st.a0_frame_bytes(h, w)
    group = st.a0_per_group(h, w)
    assert group == expect_cut and n > group, (group, expect_cut)
    assert n * fb > 1 << 31, "the operand passes 2^31 bytes"
    marked = pd.marks(n, fb, group)
    assert {0, (1 << 31) // fb, group - 1, group, n - 1} <= set(marked)
    imgs = _a0_images(h, w, pd.n_distinct(marked), h * 31 + w)
    chw = np.stack([ora.resize_rgb(im, size)[1] for im in imgs])
    th, tv = _tables(T, hip, h, w, size)
    assert th[2] <= 7, "the tiled kernel's tap count"
    with _memory(T, name):
        buf = T.empty((n * fb + lead,), dtype=T.uint8, device="cuda")
        assert buf.data_ptr() % 256 == 0
        x = pd.build(_dev(T, imgs), n, marked, out=buf[lead:].view(n, h, w, 3))
        assert x.data_ptr() % 4 == lead % 4
        if patch:
            expected = _dev(T, _patch_rows(chw, size)).to(T.bfloat16)             # one rounding to nearest even
            run = lambda: hip.preprocess_u8_patches(x, size, th, tv)
        else:
            expected = _dev(T, chw)
            run = lambda: hip.preprocess_u8(x, size, th, tv)
        n0 = hip.launch_count()
        out = run()
        assert out is not None and hip.launch_count() > n0
        pd.report(out, expected, marked, name)
        del out
        # the last byte of the whole operand
        x[n - 1, h - 1, w - 1, 2] ^= 0xFF
        changed = imgs[-1].copy()
        changed[h - 1, w - 1, 2] ^= 0xFF
        new = ora.resize_rgb(changed, size)[1][None]
        new = _patch_rows(new, size)[0] if patch else new[0]
        if patch:
            new = T.from_numpy(new).to(T.bfloat16).view(T.int16).numpy()
            expected = expected.view(T.int16)
            run_bits = lambda: run().view(T.int16)
        else:
            run_bits = run
        _check_far_end(T, name, n, marked, expected, new, run_bits)
        del x, buf, expected


@pytest.mark.parametrize("patch", [False, True], ids=["fp32", "patch"])
def test_a0_cut_by_frame_count_past_2_31(T, hip, patch):
    """112 x 112 -> 48: 37 632 bytes a frame, 7 bilinear taps (the tiled kernel).  65 535 + 9 frames = 2.47 GB: the first group's
    offsets pass 2^31, the second group has one whole round of eight XCDs and one frame more."""
    _a0(T, hip, 112, 112, 48, 65535 + 9, patch, 0, 65535)


@pytest.mark.parametrize("patch,lead", [(False, 0), (True, 0), (False, 1)], ids=["fp32_aligned", "patch_aligned", "fp32_base+1"])
def test_a0_odd_frame_size_cut_at_multiples_of_four(T, hip, patch, lead):
    """111 x 111 -> 48: 36 963 bytes a frame, no multiple of 4 - groups of 65 532, so that the second group's base stays dword
    aligned: the patch form, which serves aligned groups only, answers the whole batch.  From a base 1 byte off every group takes
    the general kernel, with more than 65 535 frames in the call."""
    _a0(T, hip, 111, 111, 48, 65532 + 9, patch, lead, 65532)


def test_a0_cut_by_bytes_at_the_production_frame_size(T, hip):
    """480 x 640 -> 224, 7 taps both ways: groups of 0xfffffff0 / 921 600 = 4 660 frames."""
    _a0(T, hip, 480, 640, 224, 4660 + 9, False, 0, 4660)


# ------------------------------------------------------------------------------------------------------------------ A9
@pytest.mark.parametrize("n,fast", [(65535 + 9, True), (0xfffffff0 // (112 * 112 * 3) + 9, False)], ids=["fast_past_2_31", "fallback_past_4GiB"])
def test_a9_bank_past_2_31(T, hip, n, fast):
    """112 x 112 frames resampled to 80 (bicubic, 7 taps both ways), 3 keypoints a frame.  2.47 GB: intensity_fast_kernel with byte
    offsets past 2^31 in its one descriptor; more than 0xfffffff0 bytes: the fall-back intensity_kernel with 64-bit addresses."""
    h = w = 112
    size, K, fb = 80, 3, 112 * 112 * 3
    name = f"A9 {n} frames ({'fast' if fast else 'fall-back'})"
    th, tv = _tables(T, hip, h, w, size, bicubic=True)
    assert th[2] <= 7 and tv[2] <= 7
    assert st.a9_fast(n, h, w, K, th[2], tv[2]) == fast and n * fb > 1 << 31
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    imgs = _a0_images(h, w, d, 977)
    rng = np.random.default_rng(5)
    kp = (rng.random((d, K, 2)) * size).astype(np.float32)
    kp[:, 0] = [size - 1, size - 1]                                               # the frame's last source bytes
    kp[:, 1] = [0, 0]
    want = np.stack([ora.intensity(imgs[i], size, kp[i]) for i in range(d)])
    with _memory(T, name):
        x = pd.build(_dev(T, imgs), n, marked)
        kpd = pd.build(_dev(T, kp), n, marked)
        expected = _dev(T, want)
        run = lambda: hip.keypoint_intensity(x, size, th, tv, kpd)
        pd.report(run(), expected, marked, name)
        x[n - 1, h - 1, w - 1, 1] ^= 0xFF
        changed = imgs[-1].copy()
        changed[h - 1, w - 1, 1] ^= 0xFF
        _check_far_end(T, name, n, marked, expected, ora.intensity(changed, size, kp[-1]), run)
        del x, kpd, expected


# ------------------------------------------------------------------------------------------------------------------ A2
def _bn_params(T, rng):
    return [rng.standard_normal(384).astype(np.float32) * s + o for s, o in ((0.2, 1.0), (0.3, 0.0), (0.5, 0.0))] + \
           [(rng.random(384) + 0.5).astype(np.float32)]


@pytest.mark.parametrize("cells,group,train,form", [(9, 1, True, "reg <4, 49, 0>"), (16 * 49 + 1, 1, True, "reg <4, 100, 0>"),
                                                    (16 * 100 + 1, 1, True, "reg <2, 200, 25>"), (9, 2, True, "sweep, group 2"),
                                                    (9, 2, False, "sweep, eval")],
                         ids=["reg49", "reg100", "reg200", "sweep_group2", "sweep_eval"])
def test_bn_tokens_past_2_31(T, hip, cells, group, train, form):
    """Tokens past 2^31 bytes at the smallest cell count each form takes.  A `frame` of the periodic operand is one statistics
    group: with group = 2 it is two frames, and the period 14 frames."""
    n_prefix = 5
    t = cells + n_prefix
    fb = group * t * 384 * 4
    n = (1 << 31) // fb + 9                                                       # groups
    name = f"bn_tokens {form}: {n * group} frames of {cells} cells"
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    rng = np.random.default_rng(cells * 3 + group)
    toks = (rng.standard_normal((d, group, t, 384)) * 1.5 + 0.25).astype(np.float32)
    gamma, beta, rmean, rvar = _bn_params(T, rng)

    def oracle(tk):
        o, m, v = ora.bn_tokens(tk.reshape(-1, t, 384), n_prefix, group, gamma, beta, rmean, rvar, train=train)
        return o.reshape(-1, group, cells, 384), m, v

    want, wmean, wvar = oracle(toks)
    with _memory(T, name):
        x = pd.build(_dev(T, toks), n, marked)
        assert x.numel() * 4 > 1 << 31
        params = [_dev(T, a) for a in (gamma, beta, rmean, rvar)]

        def run():
            o, m, v = hip.bn_tokens(x.view(n * group, t, 384), n_prefix, group, *params, train, 1e-5)
            return o.view(n, group, cells, 384), m, v

        expected = _dev(T, want)
        out, mean, var = run()
        pd.report(out, expected, marked, name)
        if train:
            pd.report(mean, _dev(T, wmean), marked, name + ", batch mean")
            pd.report(var, _dev(T, wvar), marked, name + ", batch variance")
        del out, mean, var
        # the last float of the whole operand
        x[n - 1, group - 1, t - 1, 383] += 3.0
        changed = toks[-1:].copy()
        changed[0, group - 1, t - 1, 383] += np.float32(3.0)
        _check_far_end(T, name, n, marked, expected, oracle(changed)[0][0], lambda: run()[0])
        del x, expected


# ------------------------------------------------------------------------------------------------------------------ A3
@pytest.mark.parametrize("G,n_want,form", [(7, 57065, "the halo form over frame borders"), (30, 3106, "the per-frame halo form")], ids=["G7", "G30"])
def test_selector_fp32_at_its_byte_cap(T, hip, G, n_want, form):
    """The largest n_frames sslam_selector_saliency accepts - at G = 7 57 065 frames, 4.295 GB of fp32 features under one 32-bit
    descriptor; at G = 30, the smallest grid whose 128-cell tiles no longer fit the halo image across a frame border (the per-frame
    tiling of the halo form), 3 106 frames - and one frame more, refused with nothing launched and nothing written."""
    n = st.LIMITS["sslam_selector_saliency"]["largest"](G=G)
    assert n == n_want and (n + 1) * G * G * 1536 > 0xffffffff >= n * G * G * 1536
    name = f"selector fp32, G = {G}, {n} frames"
    fb = G * G * 1536
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    sd = synth.selector_state(0)
    feat = (np.random.default_rng(G).standard_normal((d, G, G, 384)) * 0.8).astype(np.float32)
    want = ora.selector_saliency(feat, sd)
    w = [_dev(T, hip.pack_conv3x3(sd["conv.0.weight"])), _dev(T, sd["conv.0.bias"]), _dev(T, sd["conv.2.weight"].reshape(-1)),
         _dev(T, sd["conv.2.bias"])]
    with _memory(T, name):
        whole = T.empty((n + 1, G, G, 384), dtype=T.float32, device="cuda")
        x = pd.build(_dev(T, feat), n, marked, out=whole[:n])
        whole[n] = x[0]
        expected = _dev(T, want)
        run = lambda: hip.selector_saliency(x, *w, 256)
        pd.report(run(), expected, marked, name)
        # one frame more
        sal = T.full((n + 1, G, G), -(2.0 ** 100), dtype=T.float32, device="cuda")
        n0 = hip.launch_count()
        with pytest.raises(hip.SslamHipError, match="unsupported"):
            hip.selector_saliency(whole, *w, 256, out=sal)
        assert hip.launch_count() == n0 and bool((sal == -(2.0 ** 100)).all()), "a refused call launches and writes nothing"
        del sal
        # the last float of the accepted operand
        x[n - 1, G - 1, G - 1, 383] += 2.0
        changed = feat[-1:].copy()
        changed[0, G - 1, G - 1, 383] += np.float32(2.0)
        _check_far_end(T, name, n, marked, expected, ora.selector_saliency(changed, sd)[0], run)
        del x, whole, expected


def test_selector_bf16_at_its_byte_cap(T, hip):
    """G = 7: the largest n_frames sslam_selector_saliency_bf16 accepts - 114 130 frames, 4.295 GB of bf16 features - on order-free
    operands (tests/orderfree.py: every product and partial sum exact in any order), where the bf16 kernel equals the exact oracle bit
    for bit; one frame more is refused."""
    import orderfree
    G = 7
    n = st.LIMITS["sslam_selector_saliency_bf16"]["largest"](G=G)
    assert n == 114130 and (n + 1) * G * G * 768 > 0xffffffff >= n * G * G * 768
    name = f"selector bf16, G = {G}, {n} frames"
    marked = pd.marks(n, G * G * 768)
    d = pd.n_distinct(marked)
    feat, sd, _, _ = orderfree.selector_case(G, G, d + 1, 256)
    feat[d] = feat[d - 1]                                                          # the last: the changed last frame
    feat[d, G - 1, G - 1, 383] = 2.0 if feat[d, G - 1, G - 1, 383] != 2.0 else -2.0
    want = ora.selector_saliency(feat, sd)
    w = [_dev(T, hip.pack_conv3x3_bf16(sd["conv.0.weight"])).view(T.bfloat16), _dev(T, sd["conv.0.bias"]), _dev(T, sd["conv.2.weight"].reshape(-1)),
         _dev(T, sd["conv.2.bias"])]
    with _memory(T, name):
        fb = hip.to_bf16(_dev(T, feat))
        assert T.equal(fb.float(), _dev(T, feat)), "order-free features are bf16 values"
        whole = T.empty((n + 1, G, G, 384), dtype=T.bfloat16, device="cuda")
        x = pd.build(fb[:d], n, marked, out=whole[:n])
        whole[n] = fb[0]
        expected = _dev(T, want[:d])
        run = lambda: hip.selector_saliency_bf16(x, *w, 256)
        pd.report(run(), expected, marked, name)
        sal = T.full((n + 1, G, G), -(2.0 ** 100), dtype=T.float32, device="cuda")
        n0 = hip.launch_count()
        with pytest.raises(hip.SslamHipError, match="unsupported"):
            hip.selector_saliency_bf16(whole, *w, 256, out=sal)
        assert hip.launch_count() == n0 and bool((sal == -(2.0 ** 100)).all()), "a refused call launches and writes nothing"
        del sal
        x[n - 1] = fb[d]
        _check_far_end(T, name, n, marked, expected, want[d], run)
        del x, whole, expected, fb


# ------------------------------------------------------------------------------------------------------------- A4 / A5
def test_select_keypoints_bank_past_2_31(T, hip):
    """A saliency bank past 2^31 bytes at the largest grid (64 x 64: 16 KB a frame, the fewest frames) and K = 4."""
    G, K = 64, 4
    fb = G * G * 4
    n = (1 << 31) // fb + 9
    name = f"select_keypoints, G = {G}, K = {K}: {n} frames"
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    sal = np.random.default_rng(64).random((d + 1, G, G)).astype(np.float32) * 0.9 + 0.05
    sal[d] = sal[d - 1]
    sal[d, G - 1, G - 1] = 0.99                                                    # the last cell of the last frame becomes its maximum

    def oracle(a):
        kp, sc, idx, stt = ora.select_keypoints(a, K)
        return kp, sc, idx, ora.patch_to_pixel(kp), stt

    want = oracle(sal)
    with _memory(T, name):
        sd_ = _dev(T, sal)
        x = pd.build(sd_[:d], n, marked)
        assert x.numel() * 4 > 1 << 31
        run = lambda: hip.select_keypoints(x, K)
        for got, w_, what in zip(run(), want, ("kp", "scores", "idx", "pixel", "status")):
            pd.report(got, _dev(T, w_[:d]), marked, f"{name}, {what}")
        x[n - 1] = sd_[d]
        _check_far_end(T, name + ", idx", n, marked, _dev(T, want[2][:d]), want[2][d], lambda: run()[2])
        _check_far_end(T, name + ", scores", n, marked, _dev(T, want[1][:d]), want[1][d], lambda: run()[1])
        del x, sd_


# ------------------------------------------------------------------------------------------------------------- A6 / A7
@pytest.mark.parametrize("distinct_rows", [0, 1], ids=["direct", "distinct_rows"])
def test_gather_refine_bank_past_2_31(T, hip, knob, distinct_rows):
    """A feature bank past 2^31 bytes at the smallest grid the entry takes (2 x 2: 6 KB a frame) and K = 2, in the direct launch and
    in the distinct-row form (the second keypoint of every other distinct frame repeats the first: a duplicate row)."""
    knob("SSLAM_REFINE_DISTINCT", distinct_rows)
    G, K = 2, 2
    fb = G * G * 1536
    n = (1 << 31) // fb + 9
    name = f"gather_refine ({'distinct rows' if distinct_rows else 'direct'}), G = {G}, K = {K}: {n} frames"
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    rng = np.random.default_rng(22)
    feat = rng.standard_normal((d + 1, G, G, 384)).astype(np.float32)
    kp = rng.random((d + 1, K, 2)).astype(np.float32)
    kp[::2, 1] = kp[::2, 0]
    feat[d], kp[d] = feat[d - 1], kp[d - 1]
    feat[d, G - 1, G - 1, 383] += np.float32(4.0)                                  # the last float of the bank
    rsd = synth.refiner_state(0)
    want = ora.refine(ora.gather(feat, kp), rsd)
    packed = _dev(T, hip.pack_refiner(ora.refiner_weight_list(rsd, 2), 2))
    with _memory(T, name):
        fd = _dev(T, feat)
        x, kpd = pd.build(fd[:d], n, marked), pd.build(_dev(T, kp[:d]), n, marked)
        assert x.numel() * 4 > 1 << 31
        assert (hip.lib().sslam_gather_refine_workspace_bytes(n, K) > 0) == bool(distinct_rows)
        expected = _dev(T, want[:d])
        run = lambda: hip.gather_refine(x, kpd, packed, 2)
        pd.report(run(), expected, marked, name)
        x[n - 1] = fd[d]
        _check_far_end(T, name, n, marked, expected, want[d], run)
        del x, kpd, fd, expected


def test_gather_refine_bf16_bank_past_2_31(T, hip):
    """The fused bf16 entry on the same bank shape, on order-free operands (depth-0 refiner, tests/orderfree.py), where it equals
    ora.gather + ora.refine bit for bit."""
    import orderfree
    G, K = 2, 2
    fb = G * G * 1536
    n = (1 << 31) // fb + 9
    name = f"gather_refine_bf16, G = {G}, K = {K}: {n} frames"
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    feat, kp, sd, _, _, _, _ = orderfree.refiner_case(2031, G, d + 1, K)
    feat[d], kp[d] = feat[d - 1], kp[d - 1]
    kp[d] = [[G - 1, G - 1], [0, 0]]                                               # the first keypoint reads the bank's last cell alone
    feat[d, G - 1, G - 1] = -feat[d, G - 1, G - 1] + np.float32(4.0)
    want = ora.refine(ora.gather(feat, kp).reshape(-1, 384), sd, n_blocks=0).reshape(d + 1, K, 128)
    packed = _dev(T, hip.pack_refiner_bf16(ora.refiner_weight_list(sd, 0), 0))
    with _memory(T, name):
        fd = _dev(T, feat)
        x, kpd = pd.build(fd[:d], n, marked), pd.build(_dev(T, kp[:d]), n, marked)
        expected = _dev(T, want[:d])
        run = lambda: hip.gather_refine_bf16(x, kpd, packed, 0)
        pd.report(run(), expected, marked, name)
        x[n - 1], kpd[n - 1] = fd[d], _dev(T, kp[d])
        _check_far_end(T, name, n, marked, expected, want[d], run)
        del x, kpd, fd, expected


# ------------------------------------------------------------------------------------------------- depth gather, sub-cell
def test_keypoint_depth_bank_past_2_31(T, hip):
    """A depth bank past 2^31 bytes (120 x 160 uint16: 38 400 bytes a frame), 3 keypoints a frame: the corners and one inside."""
    import pose_depth_ref as dr
    h, w, K = 120, 160, 3
    fb = h * w * 2
    n = (1 << 31) // fb + 9
    name = f"keypoint_depth, {h} x {w}: {n} frames"
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    rng = np.random.default_rng(16)
    depth = rng.integers(1, 65536, size=(d + 1, h, w)).astype(np.uint16)
    kp = (rng.random((d + 1, K, 2)) * [w - 1, h - 1]).astype(np.float32)
    kp[:, 0], kp[:, 1] = [w - 1, h - 1], [0, 0]
    depth[d], kp[d] = depth[d - 1], kp[d - 1]
    depth[d, h - 1, w - 1] ^= 0x5555                                                 # the last pixel of the bank
    want = dr.keypoint_depth(depth, kp)
    with _memory(T, name):
        dd = _dev(T, depth.view(np.int16))
        x = pd.build(dd[:d], n, marked)
        kpd = pd.build(_dev(T, kp[:d]), n, marked)
        assert x.numel() * 2 > 1 << 31
        expected = _dev(T, want[:d])
        run = lambda: hip.keypoint_depth(x.view(T.uint16), kpd)
        pd.report(run(), expected, marked, name)
        x[n - 1] = dd[d]
        _check_far_end(T, name, n, marked, expected, want[d], run)
        del x, kpd, dd, expected


def test_subcell_keypoints_bank_past_2_31(T, hip):
    """A saliency bank past 2^31 bytes (64 x 64) and 4 cells a frame: the frame's last interior cell, a border cell, the last cell,
    one outside the grid."""
    import subcell_ref as sr
    G, K = 64, 4
    fb = G * G * 4
    n = (1 << 31) // fb + 9
    name = f"subcell_keypoints, G = {G}: {n} frames"
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    rng = np.random.default_rng(65)
    sal = rng.random((d + 1, G, G)).astype(np.float32)
    idx = np.tile(np.int32([(G - 2) * G + G - 2, 5, G * G - 1, G * G]), (d + 1, 1))
    idx[:, 1] = rng.integers(0, G * G, size=d + 1)
    sal[:, G - 2, G - 2] = 2.0                                                      # a strict maximum: both axes refined
    sal[d], idx[d] = sal[d - 1], idx[d - 1]
    sal[d, G - 1, G - 2] = 1.5                                                      # in the bank's last row: the y-neighbour of keypoint 0
    want = sr.subcell_keypoints(sal, idx)
    with _memory(T, name):
        sd_ = _dev(T, sal)
        x, ix = pd.build(sd_[:d], n, marked), pd.build(_dev(T, idx[:d]), n, marked)
        assert x.numel() * 4 > 1 << 31
        run = lambda: hip.subcell_keypoints(x, ix)
        for got, w_, what in zip(run(), want, ("kp_xy_sub", "kp_pixel_sub", "flags")):
            pd.report(got, _dev(T, w_[:d]), marked, f"{name}, {what}")
        x[n - 1] = sd_[d]
        _check_far_end(T, name + ", kp_xy_sub", n, marked, _dev(T, want[0][:d]), want[0][d], lambda: run()[0])
        del x, ix, sd_


# ------------------------------------------------------------------------------------------------------------------ M1
@pytest.mark.parametrize("width", [128, 256])
def test_sim_argmax_pairs_bank_past_2_31(T, hip, width):
    """A descriptor bank past 2^31 bytes (K = 64 rows a frame) and every pair (i, i + 1) of it in one call, the pair of the last two
    frames named first, through sslam_sim_argmax_pairs and both finalize entries (M1's with an intensity bank; the ratio rule).  A pair's result depends on the two slots it names: the oracle runs once per distinct couple of slots.  The
    outputs are a few MB per array: compared on the host."""
    K = 64
    fb = K * width * 4
    n = (1 << 31) // fb + 9
    name = f"sim_argmax_pairs, width {width}: bank of {n} frames"
    marked = pd.marks(n, fb)
    d = pd.n_distinct(marked)
    desc = np.random.default_rng(width).standard_normal((d, K, width)).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=-1, keepdims=True)
    firsts = np.array([n - 2] + list(range(n - 2)), dtype=np.int32)
    slot = pd.slots(n, marked).numpy()
    couple = slot[firsts] * d + slot[firsts + 1]

    rng = np.random.default_rng(width + 1)
    scores, inten = rng.random((d, K)).astype(np.float32), rng.random((d, K)).astype(np.float32)
    M1 = (0.3, 0.5, 0.1, 0.15)                                  # saliency weight, min saliency, min similarity, min intensity
    RATIO = 0.95

    def oracle(bank):
        """Per listed pair: nn12, s12, nn21, s21 and the two finalize stages (M1 with intensity; the ratio rule), zero-padded."""
        import match_rules_cases as mrc
        exp = [np.zeros((len(firsts), K) + tail, dt) for dt, tail in ((np.int32, ()), (np.float32, ()), (np.int32, ()), (np.float32, ()),
                                                                       (np.int64, (2,)), (np.float32, ()), (np.int32, (1,)),
                                                                       (np.int64, (2,)), (np.float32, ()), (np.int32, (1,)))]
        exp[6], exp[9] = exp[6][:, 0], exp[9][:, 0]              # the two counts: one per pair
        for c in np.unique(couple):
            a, b = c // d, c % d
            rows = couple == c
            for e, v in zip(exp, ora.sim_argmax(bank[a], bank[b])):
                e[rows] = v
            m, q = ora.match_with_quality(bank[a], bank[b], scores[a], scores[b], M1[0], M1[1], M1[2], inten[a], inten[b], M1[3])
            pad = np.zeros((K, 2), np.int64), np.zeros(K, np.float32)
            pad[0][:len(m)], pad[1][:len(m)] = m, q
            exp[4][rows], exp[5][rows], exp[6][rows] = pad[0], pad[1], len(m)
            m, v = mrc.oracle_rule(mrc.RATIO, bank[a], bank[b], RATIO)
            pad = np.zeros((K, 2), np.int64), np.zeros(K, np.float32)
            pad[0][:len(m)], pad[1][:len(m)] = m, v
            exp[7][rows], exp[8][rows], exp[9][rows] = pad[0], pad[1], len(m)
        return exp

    def wrong_pairs(got, exp):
        bad = np.zeros(len(firsts), bool)
        for g, e in zip(got, exp):
            bad |= (np.ascontiguousarray(g).view(np.uint8).reshape(len(firsts), -1) != np.ascontiguousarray(e).view(np.uint8).reshape(len(firsts), -1)).any(axis=1)
        return firsts[bad].tolist()

    want = oracle(desc)
    assert 0 < want[6].max() and want[6].min() < K and 0 < want[9].max() and want[9].min() < K, "both finalize stages keep some rows and drop some"
    with _memory(T, name):
        bank = pd.build(_dev(T, desc), n, marked)
        sbank, ibank = pd.build(_dev(T, scores), n, marked), pd.build(_dev(T, inten), n, marked)
        assert bank.numel() * 4 > 1 << 31
        first = _dev(T, firsts)

        def run():
            nn12, s12, nn21, s21, sec = hip.sim_argmax_pairs(bank, first, first + 1, want_s21=True, want_second=True)
            m1 = hip.match_finalize_pairs(nn12, s12, nn21, first, first + 1, sbank, ibank, 1.0 - M1[0], M1[0], M1[1], M1[2], M1[3])
            m2 = hip.match_finalize_rule_pairs(nn12, s12, sec, nn21, first, first + 1, n, hip.RULE_RATIO_BEST, RATIO)
            return [a.cpu().numpy() for a in (nn12, s12, nn21, s21) + tuple(m1) + tuple(m2)]

        bad = wrong_pairs(run(), want)
        assert not bad, f"{name}: {len(bad)} mismatching pairs of {len(firsts)}, first frames {bad[:8]}"
        print(f"{name}: 0 mismatching pairs of {len(firsts)}")
        # the last row of the last frame becomes the copy of the first row of frame n - 2: pair (n - 2, n - 1) changes, no other
        bank[n - 1, K - 1] = bank[n - 2, 0]
        changed = desc.copy()
        changed[slot[n - 1], K - 1] = changed[slot[n - 2], 0]
        want2 = oracle(changed)
        assert want2[0][0, 0] == K - 1 != want[0][0, 0], "the oracle sees the change"
        got2 = run()
        assert wrong_pairs(got2, want) == [n - 2] and not wrong_pairs(got2, want2)
        print(f"{name}, last frame changed: 0 mismatching pairs of {len(firsts)}")
        del bank, first, sbank, ibank


# ------------------------------------------------------------------------------------------------------------------ A1
def test_vit_f32_at_its_hidden_activation_cap(T, hip):
    """64 x 64 frames (T = 21 tokens): the largest frame count sslam_vit_forward_f32 accepts - its MLP hidden activation, 6 144
    bytes a token, is then 0xfffffff0 bytes or just below, and the per-layer GEMM's 32-bit A offsets pass 2^31 and reach the cap -
    and one frame more refused.  The marked frame `byte 2^31` is the one whose hidden rows hold that byte.  Every frame equals the same
    frame from a 9-frame batch bit for bit (launch groups change no bit: the claim of test_fp32_tokens_do_not_depend_on_the_launch_groups,
    the one place where results of the code under test serve as the expectation); the distinct frames are held to the float64
    reference within the BARS["f32"] of tests/test_gpu_vit_reference.py."""
    import foreign_vit
    import test_gpu_vit_reference as vr
    from oracle import ora_vit
    from sslam_amd.vit_hip import HipViTF32
    size, t = 64, 21
    n = st.LIMITS["sslam_vit_forward_f32"]["largest"](size=size)
    assert n * t * 6144 <= 0xfffffff0 < (n + 1) * t * 6144 and n * t * 6144 > 1 << 31
    name = f"fp32 ViT, {n} frames of {size} x {size}"
    marked = pd.marks(n, t * 6144)
    assert len(marked) == 3 and 0 < marked[1] < n - 1
    d = pd.n_distinct(marked)
    vit = foreign_vit.random_vit(1).cuda()
    hv = HipViTF32(vit)
    imgs = T.randn(d + 1, 3, size, size, generator=T.Generator().manual_seed(641)).cuda()      # the last: the changed last frame
    imgs[d] = imgs[d - 1]
    imgs[d, 2, size - 1, size - 1] += 1.5

    def nine(frames):
        """Tokens of `frames` from 9-frame launches (one-pass attention, as every launch above 8 frames)."""
        out = []
        with T.no_grad():
            for a in range(0, frames.shape[0], 9):
                batch = frames[a:a + 9]
                pad = T.cat([batch, frames[:9 - batch.shape[0]]]) if batch.shape[0] < 9 else batch
                out.append(hv.forward_features(pad.contiguous(), chunk=9)[:batch.shape[0]].clone())
        return T.cat(out)

    small = nine(imgs)                                                                     # also points hv.w at the RoPE tables of G = 4
    want = ora_vit.forward(vit, imgs, "exact")
    vr._check(f"{name}: the distinct frames in 9-frame launches", small, want, "f32")
    with _memory(T, name):
        whole = T.empty((n + 1, 3, size, size), dtype=T.float32, device="cuda")
        x = pd.build(imgs[:d], n, marked, out=whole[:n])
        whole[n] = imgs[0]
        ws = T.empty(hip.vit_f32_workspace_bytes(n + 1, size), dtype=T.uint8, device="cuda")
        run = lambda: hip.vit_forward_f32(x, hv.w, ws)
        out = run()
        pd.report(out, small[:d], marked, name)
        picks = list(range(pd.P, 2 * pd.P)) + marked                                   # frames 7..13 hold slots 0..6
        assert pd.slots(n, marked)[picks].tolist() == list(range(d))
        vr._check(f"{name}: frames {picks} of the large launch", out[T.tensor(picks, device='cuda')], want[:d], "f32")
        del out
        # one frame more
        tok = T.full((n + 1, t, 384), -(2.0 ** 100), dtype=T.float32, device="cuda")
        n0 = hip.launch_count()
        with pytest.raises(hip.SslamHipError, match="unsupported"):
            hip.vit_forward_f32(whole, hv.w, ws, out=tok)
        assert hip.launch_count() == n0 and bool((tok == -(2.0 ** 100)).all()), "a refused call launches and writes nothing"
        del tok
        # one pixel of the last frame
        x[n - 1] = imgs[d]
        _check_far_end(T, name, n, marked, small[:d], small[d].cpu().numpy(), run)
        vr._check(f"{name}: the changed last frame", run()[n - 1:], want[d:], "f32")
        del x, whole, ws
