"""The size contract without a device: tests/size_table.py holds every exported entry and is what the headers state; a call one
above each stated limit is refused with the stated code before anything is launched (dummy, aligned, never dereferenced
pointers); no layer above the entries hands one of them more than it accepts; tests/periodic.py, the helper of the GPU tests,
finds one changed element where it is and nothing where nothing changed."""
import ctypes as C
import os
import re

import pytest
import torch

import periodic as pd
import size_table as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [0x10000 * (i + 1) for i in range(16)]       # never dereferenced: every call below is refused before the launch
E_UNSUPPORTED = -2


# ---------------------------------------------------------------------------------------------------------------- the table
def test_every_export_has_a_row_or_a_reason():
    from sslam_amd import lib
    for exports, rows, free in ((lib.EXPORTS, st.LIMITS, {**st.NO_LIMIT, **{e: "host only" for e in st.HOST_ONLY}}),
                                (lib.EXT_EXPORTS, st.EXT_LIMITS, st.EXT_NO_LIMIT)):
        assert not set(rows) & set(free), sorted(set(rows) & set(free))
        missing = [e for e in exports if e not in rows and e not in free]
        assert not missing, f"entries without a row in tests/size_table.py: {missing}"
        assert not sorted((set(rows) | set(free)) - set(exports)), "rows of entries that are not exported"
        assert all(isinstance(why, str) and why for why in free.values())
    for row in list(st.LIMITS.values()) + list(st.EXT_LIMITS.values()):
        assert row["limits"] and callable(row["largest"]) and row["widths"] and set(row["widths"].values()) <= {31, 32, 64}, row
        assert all(code == E_UNSUPPORTED for _, code in row["limits"])


@pytest.mark.parametrize("header,ext,title", [("sslam_hip.h", False, "SIZE LIMITS, every entry that launches a kernel"),
                                              ("sslam_ext.h", True, "SIZE LIMITS")])
def test_the_headers_state_the_table(header, ext, title):
    text = open(os.path.join(ROOT, "include", header)).read()
    start = text.index(title)
    block = text[start:text.index("*/", start)]
    stated = re.sub(r"\n \*\s+", " ", block)
    lines = st.header_lines(ext)
    for line in lines:
        assert line + " " in stated + " ", f"include/{header} does not state: {line}"
    assert len(re.findall(r"\bss(?:lam|lx)_\w+: ", stated)) == len(lines), "the header's block has a line the table lacks"


def test_the_contract_is_named_in_the_design():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "correct over the whole range it accepts and refuses one past it" in text
    audit = open(os.path.join(ROOT, "profiles", "size_limits.txt")).read()
    for kernel in ("preprocess_fast_kernel", "intensity_fast_kernel", "bn_tokens_reg_kernel", "bn_tokens_kernel", "halo_tile", "gemm_f32_rows_kernel"):
        assert kernel in audit, kernel


# ---------------------------------------------------------------------------------------------- one above every stated limit
def _L():
    from sslam_amd import lib
    return lib, lib.lib()


def _refused(call, what):
    lib, _ = _L()
    before = lib.launch_count()
    assert call() == E_UNSUPPORTED, what
    assert lib.launch_count() == before, f"{what}: a refused call launches nothing"


@pytest.mark.parametrize("G", [1, 7, 28, 40, 64])
def test_selector_byte_caps(G):
    lib, L = _L()
    for entry, call in (("sslam_selector_saliency", lambda n: L.sslam_selector_saliency(P[0], n, G, P[1], P[2], P[3], P[4], 256, P[5], None)),
                        ("sslam_selector_saliency_ws", lambda n: L.sslam_selector_saliency_ws(P[0], n, G, P[1], P[2], P[3], P[4], 256, P[5], P[6], 1 << 40, None)),
                        ("sslam_selector_saliency_bf16", lambda n: L.sslam_selector_saliency_bf16(P[0], n, G, P[1], P[2], P[3], P[4], 256, P[5], None))):
        n = st.LIMITS[entry]["largest"](G=G)
        width = 4 if "bf16" not in entry else 2
        assert n * G * G * 384 * width <= 0xffffffff < (n + 1) * G * G * 384 * width
        _refused(lambda: call(n + 1), f"{entry} G = {G}, {n + 1} frames")
    assert st.LIMITS["sslam_selector_saliency"]["largest"](G=7) == 57065


@pytest.mark.parametrize("size", [16, 64, 224, 448])
def test_vit_hidden_activation_caps(size):
    lib, L = _L()
    w32, w16 = lib.VitWeightsF32(), lib.VitWeights()
    t = (size // 16) ** 2 + 5
    n = st.LIMITS["sslam_vit_forward_f32"]["largest"](size=size)
    assert n * t * 6144 <= 0xfffffff0 < (n + 1) * t * 6144
    if size == 448:
        assert n == 885, "886 x 789 x 6 144 bytes is 20 480 bytes above 2^32"
    _refused(lambda: L.sslam_vit_forward_f32_form(P[0], n + 1, size, C.byref(w32), P[1], 1 << 62, P[2], 0, None), f"fp32 ViT, {n + 1} frames of {size}")
    _refused(lambda: L.sslam_vit_forward_f32(P[0], n + 1, size, C.byref(w32), P[1], 1 << 62, P[2], None), f"fp32 ViT, {n + 1} frames of {size}")
    nb = st.LIMITS["sslam_vit_forward"]["largest"](size=size)
    assert nb * t * 1536 <= 0x7fffffff * 64 < (nb + 1) * t * 1536
    if nb + 1 <= 0x7fffffff:
        _refused(lambda: L.sslam_vit_forward(P[0], nb + 1, size, C.byref(w16), P[1], 1 << 62, P[2], None), f"bf16 ViT, {nb + 1} frames of {size}")
        _refused(lambda: L.sslam_vit_forward_patches(P[0], nb + 1, size, C.byref(w16), P[1], 1 << 62, P[2], None), f"bf16 ViT, patch rows, {nb + 1} frames")


def test_bn_tokens_rows_of_a_group():
    lib, L = _L()
    top = st.LIMITS["sslam_bn_tokens"]["largest"]()
    assert top == 0x7fffffff - 16 * 7, "the sweep kernel steps an int row index up to 16 * 7 past the last row"
    f = C.c_float(1e-5)
    for group, cells in ((1, top + 1), (2, top // 2 + 1), (top + 1, 1), (65536, 32768)):
        assert group * cells > top
        t = cells + 5
        if t > 0x7fffffff:
            t, pre = 0x7fffffff, 0x7fffffff - cells
        else:
            pre = 5
        n = group
        _refused(lambda: L.sslam_bn_tokens(P[0], n, t, pre, group, P[1], P[2], P[3], P[4], 1, f, P[5], P[6], P[7], None), f"bn_tokens {group} x {cells}")
        _refused(lambda: L.sslam_bn_tokens_bf16copy(P[0], n, t, pre, group, P[1], P[2], P[3], P[4], 0, f, P[5], P[8], P[6], P[7], None),
                 f"bn_tokens_bf16copy {group} x {cells}")


@pytest.mark.parametrize("n1,n2", [(1, 1), (128, 128), (129, 64), (500, 500), (64, 1024), (4096, 4096)])
def test_matcher_and_validation_grid_packing(n1, n2):
    lib, L = _L()
    ll = C.c_longlong
    big = st.LIMITS["sslam_sim_argmax"]["largest"](n1=n1, n2=n2)
    rows = st.LIMITS["sslam_sim_argmax_rows"]["largest"](n1=n1)
    assert big * ((max(n1, n2) + 127) // 128) <= 0x7ffffff0 // 8 < (big + 1) * ((max(n1, n2) + 127) // 128)
    s1, s2 = ll(n1 * 128), ll(n2 * 128)
    for d in (128, 256):
        _refused(lambda: L.sslam_sim_argmax_d(P[0], s1, n1, P[1], s2, n2, big + 1, P[2], P[3], P[4], None, None, d, None), "sim_argmax_d")
        _refused(lambda: L.sslam_sim_argmax_ws_d(P[0], s1, n1, P[1], s2, n2, big + 1, P[2], P[3], P[4], None, None, P[5], ll(1 << 62), d, None), "sim_argmax_ws_d")
        _refused(lambda: L.sslam_sim_argmax_rows_d(P[0], s1, n1, P[1], s2, n2, rows + 1, P[2], P[3], None, d, None), "sim_argmax_rows_d")
        _refused(lambda: L.sslam_row_lse_d(P[0], s1, n1, P[1], s2, n2, rows + 1, P[2], C.c_float(0.1), P[3], P[4], P[5], d, None), "row_lse_d")
    _refused(lambda: L.sslam_sim_argmax(P[0], s1, n1, P[1], s2, n2, big + 1, P[2], P[3], P[4], None, None, None), "sim_argmax")
    _refused(lambda: L.sslam_sim_argmax_ws(P[0], s1, n1, P[1], s2, n2, big + 1, P[2], P[3], P[4], None, None, P[5], ll(1 << 62), None), "sim_argmax_ws")
    _refused(lambda: L.sslam_sim_argmax_rows(P[0], s1, n1, P[1], s2, n2, rows + 1, P[2], P[3], None, None), "sim_argmax_rows")
    _refused(lambda: L.sslam_row_lse(P[0], s1, n1, P[1], s2, n2, rows + 1, P[2], C.c_float(0.1), P[3], P[4], P[5], None), "row_lse")
    # the pair-list forms: K rows both ways
    K = n1
    kbig = st.LIMITS["sslam_sim_argmax_pairs"]["largest"](n1=K, n2=K)
    fs = ll(K * 128)
    _refused(lambda: L.sslam_sim_argmax_pairs(P[0], fs, 9, K, P[1], P[2], kbig + 1, P[3], P[4], P[5], None, None, P[6], ll(1 << 62), None), "sim_argmax_pairs")
    _refused(lambda: L.sslam_sim_argmax_pairs_d(P[0], fs, 9, K, P[1], P[2], kbig + 1, P[3], P[4], P[5], None, None, P[6], ll(1 << 62), 256, None), "sim_argmax_pairs_d")
    _refused(lambda: L.sslam_sim_argmax_rows_pairs(P[0], fs, 9, K, P[1], P[2], kbig + 1, P[3], P[4], None, None), "sim_argmax_rows_pairs")
    _refused(lambda: L.sslam_sim_argmax_rows_pairs_d(P[0], fs, 9, K, P[1], P[2], kbig + 1, P[3], P[4], None, 256, None), "sim_argmax_rows_pairs_d")
    _refused(lambda: L.sslam_row_lse_pairs(P[0], fs, 9, K, P[1], P[2], kbig + 1, P[3], C.c_float(0.1), P[4], P[5], P[6], None), "row_lse_pairs")
    _refused(lambda: L.sslam_row_lse_pairs_d(P[0], fs, 9, K, P[1], P[2], kbig + 1, P[3], C.c_float(0.1), P[4], P[5], P[6], 256, None), "row_lse_pairs_d")


@pytest.mark.parametrize("K", [1, 3, 500, 4096])
def test_keypoint_depth_and_subcell_keypoint_counts(K):
    lib, L = _L()
    X = lib.ext()
    n = st.LIMITS["sslam_keypoint_depth"]["largest"](K=K)
    assert n * K <= 0x7fffffff < (n + 1) * K and n == st.EXT_LIMITS["sslx_subcell_keypoints"]["largest"](K=K)
    if n + 1 > 0x7fffffff:
        return                                              # K = 1: no int names a count above the limit
    _refused(lambda: L.sslam_keypoint_depth(P[0], n + 1, 480, 640, P[1], K, C.c_double(1.0), C.c_double(1.0), P[2], None), f"keypoint_depth K = {K}")
    before = X.sslx_launch_count()
    assert X.sslx_subcell_keypoints(P[0], n + 1, 28, P[1], K, P[2], P[3], P[4], None) == E_UNSUPPORTED
    assert X.sslx_launch_count() == before


def test_edge_pool_grid_dimensions():
    lib, L = _L()
    _refused(lambda: L.sslam_edge_pool(P[0], 65536, 32, P[1], P[2], None), "edge_pool 65 536 frames")
    _refused(lambda: L.sslam_edge_pool(P[0], 1, 65536 * 16, P[1], P[2], None), "edge_pool 65 536 cell rows")


@pytest.mark.parametrize("entry", ["sslam_preprocess_u8", "sslam_preprocess_u8_patches"])
def test_a0_frame_bytes_and_workgroup_count(entry):
    lib, L = _L()
    fn = getattr(L, entry)
    call = lambda n, h, w, size, ks=3: fn(P[0], n, h, w, size, P[1], P[2], ks, P[3], P[4], ks, P[5], None)
    # a frame above 2^31 - 1 bytes: 26 755 x 26 755 x 3 = 2 147 490 075 (the general kernel's tile needs h <= ~40 size: size = 26 752)
    h = w = 26755
    assert st.a0_frame_bytes(h, w) > 0x7fffffff >= st.a0_frame_bytes(h - 1, w)
    _refused(lambda: call(1, h, w, 26752), f"{entry}: one frame of {h} x {w}")
    # more than 2^31 - 1 workgroups in a group: size 8192 is 128 x 256 tall tiles and 128 x 512 short ones
    size = 8192
    assert st.a0_tiles(4, 4, size, 3) == (128 * 256, 128 * 512, True)
    assert st.a0_workgroups(32760, 4, 4, size, 3) <= 0x7fffffff < st.a0_workgroups(32761, 4, 4, size, 3)
    _refused(lambda: call(32761, 4, 4, size), f"{entry}: 32 761 frames to {size}")
    _refused(lambda: call(1 << 20, 4, 4, size), f"{entry}: 2^20 frames to {size} (the first group is refused)")


def test_a0_group_cut():
    """per_group as preprocess_launch computes it, at the shapes the GPU tests run and at its edges."""
    assert st.a0_per_group(112, 112) == 65535 and st.a0_per_group(111, 111) == 65532 and st.a0_per_group(480, 640) == 4660
    assert st.a0_per_group(1, 1) == 65532 and st.a0_per_group(2, 2) == 65535
    assert st.a0_per_group(26754, 26754) == 2 and st.a0_per_group(26755, 26755) == 1 and st.a0_per_group(18919, 18919) == 3
    for h, w in ((111, 111), (1, 1), (16383, 16383), (37, 53)):
        fb, g = st.a0_frame_bytes(h, w), st.a0_per_group(h, w)
        assert fb & 3 and g >= 4 and (g * fb) % 4 == 0 and g * fb <= 0xfffffff0, "an odd frame size: every group's base keeps the call's alignment"
    fb = st.a0_frame_bytes(18919, 18919)
    assert fb & 3 and st.a0_per_group(18919, 18919) == 0xfffffff0 // fb < 4, "fewer than 4 frames a group: cut as they fit (odd bases take the general kernel)"
    src = open(os.path.join(ROOT, "semantic-slam-master_amd", "csrc", "resample.hip")).read()
    for text in ("std::min<long long>(65535, std::max<long long>(1, 0xfffffff0LL / fbytes))", "if ((fbytes & 3) && per_group >= 4) per_group &= ~3;",
                 "bytes <= 0xfffffff0LL && total <= 0x7fffff00LL"):
        assert text in src, f"tests/size_table.py restates a line the dispatch code no longer has: {text}"
    assert st.a9_fast(65544, 112, 112, 3, 7, 7) and not st.a9_fast(114140, 112, 112, 3, 7, 7) and not st.a9_fast(9, 112, 112, 3, 9, 7)


# ------------------------------------------------------------------------------------- no layer above exceeds a table limit
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_no_layer_hands_an_entry_more_than_it_accepts(precision):
    import bench
    from sslam_amd.pipeline import ExtractorConfig
    from sslam_amd.vit_hip import HipViT, HipViTF32
    assert bench.WORKLOADS
    for name, (n, h, w, size, K) in bench.WORKLOADS.items():
        cfg = ExtractorConfig(input_size=size, num_keypoints=K, precision=precision)
        lg, G = cfg.launch_group(), cfg.grid
        assert 1 <= lg <= st.LIMITS["sslam_selector_saliency_ws"]["largest"](G=G), name
        assert lg <= st.LIMITS["sslam_selector_saliency_bf16"]["largest"](G=G), name
        assert G * G <= st.LIMITS["sslam_bn_tokens"]["largest"]() and G * G <= st.LIMITS["sslam_select_keypoints"]["largest"]() >= K, name
        assert lg <= st.LIMITS["sslam_keypoint_depth"]["largest"](K=K) and lg <= st.EXT_LIMITS["sslx_subcell_keypoints"]["largest"](K=K), name
        assert lg <= st.LIMITS["sslam_sim_argmax_pairs"]["largest"](n1=K, n2=K) and n <= st.LIMITS["sslam_sim_argmax_rows_pairs"]["largest"](n1=K), name
        # A0 cuts by itself; what reaches it in one call is the 16 * vit_chunk span of tokens_from_images
        assert st.a0_frame_bytes(h, w) <= st.LIMITS["sslam_preprocess_u8"]["largest"](), name
        for vit, entry in ((HipViT, "sslam_vit_forward_patches"), (HipViTF32, "sslam_vit_forward_f32")):
            chunk = vit.chunk_frames(size)
            assert 1 <= chunk <= st.LIMITS[entry]["largest"](size=size), (name, entry)
            span = 16 * chunk
            tv = 2 * ((h + size - 1) // size) + 3                     # a bound on the bilinear tap count, for the tile sizes only
            assert st.a0_workgroups(span, h, w, size, tv) <= 0x7fffffff, name


# ------------------------------------------------------------------------------------------------- the helper, on CPU tensors
def test_marks_and_slots():
    m = pd.marks(65544, 37632, group=65535)
    assert m == [0, (1 << 31) // 37632, 65534, 65535, 65543] and pd.n_distinct(m) == 12
    assert pd.marks(20, 10) == [0, 19] and pd.marks(3000, 1 << 20, group=1000) == [0, 999, 1000, 1999, 2000, 2048, 2999]
    s = pd.slots(30, [0, 9, 10, 29]).tolist()
    assert s[0] == 7 and s[9] == 8 and s[10] == 9 and s[29] == 10
    assert all(s[i] == i % 7 for i in range(30) if i not in (0, 9, 10, 29))


@pytest.fixture(scope="module")
def bank():
    """2 052 frames of 1 MiB + 4 bytes (float32): byte 2^31 lies in frame 2047, a second launch group starts at frame 1000."""
    n, words = 2052, (1 << 18) + 1
    marked = pd.marks(n, words * 4, group=1000)
    assert (1 << 31) // (words * 4) == 2047 and marked == [0, 999, 1000, 1999, 2000, 2047, 2051]
    g = torch.Generator().manual_seed(3)
    distinct = torch.randn((pd.n_distinct(marked), words), generator=g)
    distinct[1, 5] = float("nan")
    distinct[2, 6] = -0.0
    return n, marked, distinct, pd.build(distinct, n, marked)


def test_a_periodic_bank_equals_its_expectation(bank):
    n, marked, distinct, x = bank
    assert x.shape == (n, distinct.shape[1]) and x.numel() * 4 > 1 << 31
    assert pd.mismatches(x, distinct, marked) == ([], None)
    assert pd.report(x, distinct, marked, "bank") == f"bank: 0 mismatching frames of {n}"
    for f, slot in ((0, 7), (999, 8), (1000, 9), (2047, 12), (2051, 13), (1, 1), (2050, 2050 % 7)):
        assert torch.equal(x[f].view(torch.int32), distinct[slot].view(torch.int32)), f


@pytest.mark.parametrize("where", ["last frame", "first frame of the second group", "the element holding byte 2^31", "a periodic frame", "a sign of zero"])
def test_one_changed_element_is_reported_with_its_frame(bank, where):
    n, marked, distinct, x = bank
    words = distinct.shape[1]
    f, e = {"last frame": (n - 1, words - 1), "first frame of the second group": (1000, 0),
            "the element holding byte 2^31": (2047, ((1 << 31) - 2047 * words * 4) // 4), "a periodic frame": (1234, 77),
            "a sign of zero": (2 + 7 * 100, 6)}[where]
    if where == "the element holding byte 2^31":
        assert (f * words + e) * 4 <= 1 << 31 < (f * words + e + 1) * 4
    raw = x.view(torch.int32)
    keep = int(raw[f, e])
    raw[f, e] = -0x80000000 - keep if where == "a sign of zero" else keep ^ 1      # int32 bits of -0.0: flip the sign bit
    try:
        bad, first = pd.mismatches(x, distinct, marked)
        assert bad == [f] and first[0] == f and first[1] // 4 == f * words + e, (bad, first)
        byte = (f * words + e) * 4 + (3 if where == "a sign of zero" else 0)          # little endian: the sign is in the word's last byte
        with pytest.raises(AssertionError, match=rf"1 mismatching frames of {n}; the first is frame {f} .*offset {byte}\b"):
            pd.report(x, distinct, marked, where)
    finally:
        raw[f, e] = keep
    assert pd.mismatches(x, distinct, marked) == ([], None)


def test_a_skipped_or_repeated_far_end_does_not_pass_by_periodicity(bank):
    """What the marked frames are for: an output whose second group restarts at the first group's base, or whose last frame
    repeats the frame one period before it, is periodic everywhere - and wrong at the marked frames."""
    n, marked, distinct, x = bank
    y = x.clone()
    y[1000:2000] = x[0:1000]
    bad, _ = pd.mismatches(y, distinct, marked)
    assert 1000 in bad and 1999 in bad
    y = x.clone()
    y[n - 1] = x[n - 8]
    assert pd.mismatches(y, distinct, marked)[0] == [n - 1]
