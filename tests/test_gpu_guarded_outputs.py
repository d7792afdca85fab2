"""Where the kernels write: every older entry of libsslam_hip.so, launch form by launch form, run ONCE into poisoned, guarded
buffers (tests/guarded.py; the helper's own test is tests/test_guarded_helper.py).

The other GPU tests let the wrappers of sslam_amd/lib.py allocate the outputs with torch.empty, and many compute one shape in
several forms in a row: torch's caching allocator hands the freed block of the first form to the second, so an unwritten tail can
start out holding the right answer; an overrun lands in padding nobody looks at; what a kernel reads beyond an input is never a
NaN; a workspace is fresh or zero.  Here every case follows one recipe:

  1. every input lies between bands of NaN bits (uint8 images: between bands of one byte);
  2. every output the entry writes - the optional ones too - lies between sentinel bands in an allocation that is the sentinel
     throughout;
  3. every workspace the entry accepts has exactly the advertised size and is filled with one byte;
  4. the entry is called once;
  5. the bands of every output still hold the sentinel, the payload equals the oracle bit for bit over the WHOLE array (the
     zeroed tails of the finalize kernels and absent pairs included), and every input has the bits it had before the call.

A case with a workspace or a uint8 input runs a second time with the other fill (0x00 / 0xFF): identical bytes.

The C ABI's contract this file holds: an entry writes only inside its outputs, writes every element of
them, and never reads a workspace before writing it.  rank.hip, validate.hip and the distinct-row counts have guarded tests of
their own (test_gpu_match_rank.py, test_gpu_validation_edges.py, test_gpu_refine_distinct.py) and are not repeated.

Which kernel a shape reaches is read off the dispatch code named in each section.  Guard bands: 64 KiB (one 128 x 128 fp32
tile, more than any workgroup here writes at once), 256 KiB for descriptor width 256 and the ViT's 128 x 384 token tiles.

Run on the GPU box: python -m pytest tests/test_gpu_guarded_outputs.py -m gpu -q
"""
import ctypes as C
import os

import numpy as np
import pytest

import d256_cases
import guarded as gd
import match_rules_cases as mc
import orderfree
import synth
from oracle import ora
from oracle.ora_bf16 import bf16_round, refine_bf16_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILLS = (0x00, 0xFF)


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def hip(T):
    from sslam_amd import lib
    lib.lib()          # raises if libsslam_hip.so is not built: no fallback
    return lib


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _bytes(a):
    """The bytes of a numpy array, for comparisons that a NaN or a signed zero cannot slip through."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _host(T, t):
    """A device tensor as numpy; bf16 as its uint16 bit patterns."""
    t = t.detach().cpu().contiguous()
    return t.view(T.int16).numpy().view(np.uint16) if t.dtype == T.bfloat16 else t.numpy()


def _bf16_bits(a):
    return (bf16_round(a).view(np.uint32) >> 16).astype(np.uint16)


class Bufs:
    """The guarded inputs and outputs of ONE call.  An operand's name is its argument's name in include/sslam_hip.h: under a
    gd.Placement (tests/test_gpu_loose_operands.py) the name decides where the operand lies."""

    def __init__(self, T):
        self.T, self.ins, self.outs = T, [], []

    def i(self, name, array, fill=None, guard=gd.GUARD):
        """An input between bands of NaN bits (`fill`: a byte, for uint8 images) -> the device tensor."""
        whole, mid = gd.guarded_input(self.T, array, fill=fill, guard_bytes=guard, name=name)
        self.ins.append((name, whole, mid, mid.clone(), fill))
        return mid

    def frames(self, name, array, stride, fill=None, guard=gd.GUARD):
        """A strided input: the frames (or rows) array[0], array[1], .. lie |stride| elements apart in ONE guarded input, the gaps
        holding NaN bits (`fill`: a byte, for uint8 images) - gd.spread.  stride 0: frame 0 alone, which every pair reads.  A
        negative stride: the same layout, read backwards from its last frame.  -> (the device tensor, the address to hand to
        the entry: where the frame of pair 0 starts)."""
        if stride == 0:
            t = self.i(name, array[:1], fill=fill, guard=guard)
            return t, t.data_ptr()
        t = self.i(name, gd.spread(array, abs(stride), fill=fill), fill=fill, guard=guard)
        return t, t.data_ptr() + (t.element_size() * abs(stride) * (array.shape[0] - 1) if stride < 0 else 0)

    def o(self, name, shape, dtype=None, guard=gd.GUARD):
        """A sentinel-filled output between sentinel bands -> the device tensor."""
        whole, mid = gd.guarded(self.T, shape, dtype or self.T.float32, guard_bytes=guard, name=name)
        self.outs.append((name, whole, mid))
        return mid

    def check(self, what, unwritten=()):
        """After the call: guards of every output, every payload written (but those named in `unwritten`, which must be
        untouched), the inputs and their bands as they were."""
        T = self.T
        T.cuda.synchronize()
        for name, whole, mid in self.outs:
            gd.assert_guards(whole, mid, f"{what}: output {name}")
            if name in unwritten:
                idt, sentinel = gd._int_view(T, mid.dtype)
                assert bool((mid.reshape(-1).view(idt) == sentinel).all()), f"{what}: output {name} was written"
            else:
                gd.assert_written(mid, f"{what}: output {name}")
        for name, whole, mid, before, fill in self.ins:
            gd.assert_guards(whole, mid, f"{what}: input {name}", fill=fill)
            idt, _ = gd._int_view(T, mid.dtype)
            assert T.equal(mid.reshape(-1).view(idt), before.reshape(-1).view(idt)), f"{what}: input {name} was changed"


def assert_bits(T, got, want, what):
    """A device tensor against the oracle's numpy array: same shape, same bytes, over the whole array."""
    g, w = _host(T, got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if not np.array_equal(_bytes(g), _bytes(w)):
        bad = np.flatnonzero((g.reshape(-1).view(f"u{g.itemsize}") != w.reshape(-1).view(f"u{w.itemsize}")))
        raise AssertionError(f"{what}: {bad.size} of {g.size} elements differ from the oracle; the first at flat index {bad[0]} "
                             f"({g.reshape(-1)[bad[0]]!r} vs {w.reshape(-1)[bad[0]]!r}), the last at {bad[-1]}; shape {g.shape}")


def same_runs(T, runs, what):
    """The outputs of the run with workspace / band fill 0x00 and of the run with 0xFF: identical bytes."""
    if len(runs) == 2:
        for k, (a, b) in enumerate(zip(*runs)):
            assert (a is None) == (b is None), (what, k)
            assert a is None or np.array_equal(_bytes(_host(T, a)), _bytes(_host(T, b))), f"{what}: output {k} changes with the fill"


# ============================================================================================== A0 / A9 (resample.hip)
# preprocess_launch: the fast kernel needs <= 7 horizontal taps and a dword-aligned base, else the generic kernel runs (the patch
# entry returns SSLAM_E_UNSUPPORTED there and writes nothing); tiles of 32 output rows when 32 h / size + ksize_v + 2 <= 64, else
# of 16.  Bilinear taps = 2 ceil(w / size) + 1.  What the issue's four shapes reach, and the two added for what they miss:
#   (480, 640) -> 448   5 taps, 32-row tiles            (480, 640) -> 224   7 taps, 16-row tiles (69 rows do not fit)
#   (231, 517) -> 112  11 taps: generic (odd frame bytes)    (160, 360) -> 64   13 taps: generic
#   (100, 120) -> 128   3 taps, 32-row tiles - ADDED: none of the four reaches tap class 3 (it needs w <= size)
#   (231, 317) -> 112   7 taps, 16-row tiles, odd frame bytes - ADDED: the fast kernel with frames 1 and 2 at unaligned offsets
# A base at byte offset 1 or 2 sends every shape to the generic kernel.
A0_SHAPES = [(480, 640, 448), (480, 640, 224), (231, 517, 112), (160, 360, 64), (100, 120, 128), (231, 317, 112)]
A0_FRAMES, A0_K = 3, 300
_a0 = {}


def a0_case(h, w, size):
    if (h, w, size) not in _a0:
        _a0.clear()
        imgs = _rng(h * 1000 + size).integers(0, 256, size=(A0_FRAMES, h, w, 3), dtype=np.uint8)
        chw = np.stack([ora.resize_rgb(imgs[i], size)[1] for i in range(A0_FRAMES)])
        g16 = size // 16
        rows = chw.reshape(A0_FRAMES, 3, g16, 16, g16, 16).transpose(0, 2, 4, 1, 3, 5).reshape(A0_FRAMES, g16 * g16, 768)
        kp = (_rng(size).random((A0_FRAMES, A0_K, 2)) * (size + 8) - 4).astype(np.float32)      # also outside the image
        kp[:, :50] = np.floor(kp[:, :50]) + 0.5                                                  # round-half-even cases
        inten = np.stack([ora.intensity(imgs[i], size, kp[i]) for i in range(A0_FRAMES)])
        _a0[h, w, size] = dict(imgs=imgs, chw=chw, patches=_bf16_bits(rows), kp=kp, inten=inten)
    return _a0[h, w, size]


def _tables(b, hip, h, w, size, bicubic):
    out = []
    for n_in, tag in ((w, "h"), (h, "v")):
        bounds, coefs, ks = hip.resample_table(n_in, size, bicubic)
        out.append((b.i("bounds_" + tag, bounds), b.i("coefs_" + tag, coefs), ks))
    return out


def _image(b, imgs, base, fill):
    """The frames between bands of `fill`, their base `base` bytes past a 16-byte boundary (under a gd.Placement: past where
    that puts the operand)."""
    flat = np.concatenate([np.full(base, fill, np.uint8), imgs.reshape(-1)])
    view = b.i("img", flat, fill=fill)[base:].view(imgs.shape)
    assert gd.placement is not None or view.data_ptr() % 4 == base
    return view


@pytest.mark.parametrize("base", [0, 1, 2])
@pytest.mark.parametrize("h,w,size", A0_SHAPES)
def test_preprocess_u8(T, hip, h, w, size, base):
    case, runs = a0_case(h, w, size), []
    for fill in FILLS:
        b = Bufs(T)
        th, tv = _tables(b, hip, h, w, size, False)
        out = b.o("out_chw", (A0_FRAMES, 3, size, size))
        hip.preprocess_u8(_image(b, case["imgs"], base, fill), size, th, tv, out=out)
        b.check(f"preprocess_u8 {h}x{w}->{size} base {base} bands {fill:#04x}")
        assert_bits(T, out, case["chw"], "preprocess_u8")
        runs.append((out,))
    same_runs(T, runs, "preprocess_u8")


@pytest.mark.parametrize("base", [0, 1, 2])
@pytest.mark.parametrize("h,w,size", A0_SHAPES)
def test_preprocess_u8_patches(T, hip, h, w, size, base):
    """Where the fast kernel does not serve the call (more than 7 taps, an unaligned base) the entry declines and writes nothing."""
    case, runs = a0_case(h, w, size), []
    for fill in FILLS:
        b = Bufs(T)
        th, tv = _tables(b, hip, h, w, size, False)
        out = b.o("out_patches_bf16", (A0_FRAMES, (size // 16) ** 2, 768), T.bfloat16)
        img = _image(b, case["imgs"], base, fill)
        got = hip.preprocess_u8_patches(img, size, th, tv, out=out)
        fast = th[2] <= 7 and img.data_ptr() % 4 == 0
        assert gd.placement is not None or (img.data_ptr() % 4 == 0) == (base == 0)
        assert (got is not None) == fast, (th[2], base)
        b.check(f"preprocess_u8_patches {h}x{w}->{size} base {base} bands {fill:#04x}", unwritten=() if fast else ("out_patches_bf16",))
        if fast:
            assert_bits(T, out, case["patches"], "preprocess_u8_patches")
        runs.append((out,))
    same_runs(T, runs, "preprocess_u8_patches")


@pytest.mark.parametrize("base", [0, 1, 2])
@pytest.mark.parametrize("h,w,size", A0_SHAPES)
def test_keypoint_intensity(T, hip, h, w, size, base):
    case, runs = a0_case(h, w, size), []
    for fill in FILLS:
        b = Bufs(T)
        th, tv = _tables(b, hip, h, w, size, True)
        out = b.o("out", (A0_FRAMES, A0_K))
        hip.keypoint_intensity(_image(b, case["imgs"], base, fill), size, th, tv, b.i("kp_pixel", case["kp"]), out=out)
        b.check(f"keypoint_intensity {h}x{w}->{size} base {base} bands {fill:#04x}")
        assert_bits(T, out, case["inten"], "keypoint_intensity")
        runs.append((out,))
    same_runs(T, runs, "keypoint_intensity")


# ======================================================================================================= A2 (bn_tokens.hip)
# bn_tokens_launch: train, group 1, SSLAM_BN_FORM != 1 -> the register kernel in three forms by cell count (<= 784, <= 1 600,
# <= 3 600); everything else - more cells, the knob, a group, eval mode - the three-sweep kernel.  Grids: one cell count on each
# side of every boundary, and 3 x 3.  At G = 61 the "register" case is the three-sweep kernel too (3 721 cells).
BN_GRIDS = [3, 28, 29, 40, 41, 60, 61]
BN_FORMS = {"register": (2, 1, True, None), "sweeps_knob": (2, 1, True, 1), "sweeps_group2": (4, 2, True, None),
            "sweeps_eval": (2, 1, False, None)}          # frames, group, train, SSLAM_BN_FORM
_bn = {}


def bn_case(grid, frames, group, train, n_prefix):
    key = (grid, frames, group, train, n_prefix)
    if key not in _bn:
        if len(_bn) > 4:
            _bn.clear()
        tok = np.ascontiguousarray(synth.tokens(10 + grid, grid, frames)[:, 5 - n_prefix:])
        r = _rng(grid)
        par = dict(gamma=(1 + 0.1 * r.standard_normal(384)).astype(np.float32), beta=(0.1 * r.standard_normal(384)).astype(np.float32),
                   run_mean=(0.2 * r.standard_normal(384)).astype(np.float32), run_var=(1 + 0.3 * r.random(384)).astype(np.float32))
        y, mean, var = ora.bn_tokens(tok, n_prefix, group, par["gamma"], par["beta"], par["run_mean"], par["run_var"], train, 1e-5)
        _bn[key] = (tok, par, y, mean, var)
    return _bn[key]


@pytest.mark.parametrize("bf16copy", [False, True], ids=["fp32", "bf16copy"])
@pytest.mark.parametrize("n_prefix", [5, 0])
@pytest.mark.parametrize("form", list(BN_FORMS))
@pytest.mark.parametrize("grid", BN_GRIDS)
def test_bn_tokens(T, hip, knob, grid, form, n_prefix, bf16copy):
    """The C entries directly, as lib.bn_tokens calls them, so that out_mean / out_var are guarded too (train mode; eval mode
    writes neither and gets NULL, as from the wrapper)."""
    frames, group, train, bn_form = BN_FORMS[form]
    if bn_form is not None:
        knob("SSLAM_BN_FORM", bn_form)
    tok, par, y, mean, var = bn_case(grid, frames, group, train, n_prefix)
    cells = grid * grid
    b = Bufs(T)
    d_tok = b.i("tokens", tok)
    d_par = [b.i(k, par[k]) for k in ("gamma", "beta", "run_mean", "run_var")]
    out = b.o("out_feat", (frames, cells, 384))
    out_bf = b.o("out_feat_bf16", (frames, cells, 384), T.bfloat16) if bf16copy else None
    o_mean = b.o("out_mean", (frames // group, 384)) if train else None
    o_var = b.o("out_var", (frames // group, 384)) if train else None
    dp = hip._dp
    head = (dp(d_tok), frames, cells + n_prefix, n_prefix, group, *(dp(t) for t in d_par), int(train), C.c_float(1e-5), dp(out))
    if bf16copy:
        hip._run("bn_tokens_bf16copy", hip.lib().sslam_bn_tokens_bf16copy, (d_tok, out), *head, dp(out_bf), dp(o_mean), dp(o_var))
    else:
        hip._run("bn_tokens", hip.lib().sslam_bn_tokens, (d_tok, out), *head, dp(o_mean), dp(o_var))
    b.check(f"bn_tokens G {grid} {form} prefix {n_prefix}")
    assert_bits(T, out, y, "out_feat")
    if bf16copy:
        assert_bits(T, out_bf, _bf16_bits(y), "out_feat_bf16")
    if train:
        assert_bits(T, o_mean, mean, "out_mean")
        assert_bits(T, o_var, var, "out_var")


# ========================================================================================================= A3 (selector.hip)
# sslam_selector_saliency_ws: latency form 2 (rows <= SSLAM_CONV_LAT2_ROWS and <= SSLAM_CONV_LATENCY_ROWS, hs 256, a workspace of
# 16 bytes per cell; two launches) - the 8-wave latency form (rows <= SSLAM_CONV_LATENCY_ROWS) - with SSLAM_CONV_LATENCY_ROWS = 0
# the throughput forms: the halo kernel (G = 5, 28: tiles cross frames) or its per-frame tiling (G = 44, 60), SSLAM_CONV_TAIL = 4
# cutting the rest after rounds of 4 big tiles into 32-cell tiles / quarters, the stage form under SSLAM_CONV_NO_HALO or a
# SSLAM_CONV_VARIANT other than 2 (0, 1, 3: three wave tilings).  hs = 128 has the stage kernel only, in two instantiations
# (variant < 2, >= 2), whatever the other knobs say.  A form without a workspace need (every one but latency2) gets NULL.
BIG = 1 << 30
SEL_FORMS = {"latency2": dict(SSLAM_CONV_LATENCY_ROWS=BIG, SSLAM_CONV_LAT2_ROWS=BIG),
             "latency": dict(SSLAM_CONV_LATENCY_ROWS=BIG, SSLAM_CONV_LAT2_ROWS=0),
             "throughput": dict(SSLAM_CONV_LATENCY_ROWS=0, SSLAM_CONV_LAT2_ROWS=0),
             "throughput_tail": dict(SSLAM_CONV_LATENCY_ROWS=0, SSLAM_CONV_LAT2_ROWS=0, SSLAM_CONV_TAIL=4),
             "throughput_stage": dict(SSLAM_CONV_LATENCY_ROWS=0, SSLAM_CONV_LAT2_ROWS=0, SSLAM_CONV_NO_HALO=1),
             "stage_v0": dict(SSLAM_CONV_LATENCY_ROWS=0, SSLAM_CONV_LAT2_ROWS=0, SSLAM_CONV_VARIANT=0),
             "stage_v1": dict(SSLAM_CONV_LATENCY_ROWS=0, SSLAM_CONV_LAT2_ROWS=0, SSLAM_CONV_VARIANT=1),
             "stage_v3": dict(SSLAM_CONV_LATENCY_ROWS=0, SSLAM_CONV_LAT2_ROWS=0, SSLAM_CONV_VARIANT=3)}
SEL_SHAPES = [(5, 2, 256), (28, 3, 256), (44, 3, 256), (60, 2, 256), (28, 2, 128)]
_sel = {}


def sel_case(grid, frames, hidden):
    key = (grid, frames, hidden)
    if key not in _sel:
        _sel.clear()
        sd = synth.selector_state(0 if hidden == 256 else 1, hidden=hidden)
        feat = ora.bn_tokens(synth.tokens(20 + grid, grid, frames))[0].reshape(frames, grid, grid, 384)
        _sel[key] = (feat, sd, ora.selector_saliency(feat, sd))
    return _sel[key]


def _selector_inputs(b, feat, sd, w1p):
    return (b.i("feat", feat), b.i("w1_packed", w1p), b.i("b1", sd["conv.0.bias"]), b.i("w2", sd["conv.2.weight"].reshape(-1)),
            b.i("b2", sd["conv.2.bias"]))


@pytest.mark.parametrize("form", list(SEL_FORMS))
@pytest.mark.parametrize("grid,frames,hidden", SEL_SHAPES)
def test_selector_saliency(T, hip, knob, grid, frames, hidden, form):
    """With a workspace of exactly sslam_selector_saliency_workspace_bytes (0x00, then 0xFF) and, through the entry that takes
    none, without."""
    for k, v in SEL_FORMS[form].items():
        knob(k, v)
    feat, sd, want = sel_case(grid, frames, hidden)
    w1p = hip.pack_conv3x3(sd["conv.0.weight"])
    need = int(hip.lib().sslam_selector_saliency_workspace_bytes(frames, grid))
    assert need == (frames * grid * grid * 16 if form == "latency2" else 0)
    runs = []
    for fill in FILLS if need else FILLS[:1]:
        b = Bufs(T)
        ins = _selector_inputs(b, feat, sd, w1p)
        out = b.o("sal", (frames, grid, grid))
        ws = gd.dirty(T, need, fill)
        hip.selector_saliency(*ins, hidden, out=out, workspace=ws if need else None)
        b.check(f"selector_saliency G {grid} x {frames} hs {hidden} {form} workspace {fill:#04x}")
        assert_bits(T, out, want, f"saliency, {form}")
        runs.append((out,))
    same_runs(T, runs, f"selector_saliency {form}")
    b = Bufs(T)
    d_feat, d_w1, d_b1, d_w2, d_b2 = _selector_inputs(b, feat, sd, w1p)
    out = b.o("sal", (frames, grid, grid))
    dp = hip._dp
    hip._run("selector_saliency", hip.lib().sslam_selector_saliency, (d_feat, out), dp(d_feat), frames, grid, dp(d_w1), dp(d_b1), dp(d_w2),
             dp(d_b2), hidden, dp(out))
    b.check(f"selector_saliency G {grid} x {frames} hs {hidden} {form}, the entry without a workspace")
    assert_bits(T, out, want, f"saliency, {form}, no workspace")


# ============================================================================================= A3, bf16 (selector_bf16.hip)
# The forms and the order-free inputs (tests/orderfree.py: any accumulation order gives the exact oracle's bits) of
# test_gpu_bf16_exact.py; the form that runs is checked against the library's own dispatch (sslam_selector_bf16_halo_groups).
BF_FORMS = {"halo": {}, "halo_tail2": {"SSLAM_CONVBF_TAIL": 2},
            "stage_v0": {"SSLAM_CONVBF_NO_HALO": 1, "SSLAM_CONVBF_VARIANT": 0},
            "stage_v1": {"SSLAM_CONVBF_NO_HALO": 1, "SSLAM_CONVBF_VARIANT": 1},
            "stage_v2": {"SSLAM_CONVBF_NO_HALO": 1, "SSLAM_CONVBF_VARIANT": 2}}
BF_SHAPES = {(28, 3): 6, (44, 3): 7, (5, 2): 5}          # (G, frames) -> 64-row image groups of the halo form
_selbf = {}


def selbf_case(grid, frames):
    if (grid, frames) not in _selbf:
        _selbf.clear()
        feat, sd, _, _ = orderfree.selector_case(grid, grid, frames, 256)
        _selbf[grid, frames] = (feat, sd, ora.selector_saliency(feat, sd))
    return _selbf[grid, frames]


@pytest.mark.parametrize("form", list(BF_FORMS))
@pytest.mark.parametrize("grid,frames", list(BF_SHAPES))
def test_selector_saliency_bf16(T, hip, knob, grid, frames, form):
    for k, v in BF_FORMS[form].items():
        knob(k, v)
    feat, sd, want = selbf_case(grid, frames)
    assert hip.selector_bf16_halo_groups(frames, grid, 256) == (BF_SHAPES[grid, frames] if form.startswith("halo") else 0)
    b = Bufs(T)
    fb = b.i("feat_bf16", hip.to_bf16(T.from_numpy(feat).cuda()))
    w1p = b.i("w1_packed_bf16", T.from_numpy(hip.pack_conv3x3_bf16(sd["conv.0.weight"]).view(np.int16)).view(T.bfloat16))
    out = b.o("sal", (frames, grid, grid))
    hip.selector_saliency_bf16(fb, w1p, b.i("b1", sd["conv.0.bias"]), b.i("w2", sd["conv.2.weight"].reshape(-1)), b.i("b2", sd["conv.2.bias"]),
                               256, out=out)
    b.check(f"selector_saliency_bf16 G {grid} x {frames} {form}")
    assert_bits(T, out, want, f"bf16 saliency, {form}")


# ====================================================================================================== A4 / A5 (select.hip)
# One workgroup per frame, every branch decided on the device: the fixture's tags name the branches; K above the cell count gives
# status 1 and padded slots (the oracle's rule, bit for bit); a constant map; idx and kp_pixel are optional outputs.
SELECT_TAGS = bytes(np.load(os.path.join(GOLD, "select_cases.npz"))["tags"]).decode().split(",")
SELECT_SYNTH = {"g7_k20": (7, 20), "g7_k60": (7, 60), "g64_k4096": (64, 4096)}          # K = 60 > 49 cells: status 1
OPTIONAL = {"idx_px": (True, True), "idx": (True, False), "px": (False, True), "neither": (False, False)}
_select = {}


def select_case(name):
    if name not in _select:
        if name in SELECT_SYNTH:
            grid, K = SELECT_SYNTH[name]
            sal = _rng(grid * 7 + K).random((2, grid, grid)).astype(np.float32)
            sal[0].ravel()[::5] = sal[0].ravel()[3]          # exact ties
            sal[1] = np.float32(0.5)                          # a constant map
            radius, pct, gold_idx = 2, 0.5, None
        else:
            g = np.load(os.path.join(GOLD, "select_cases.npz"))
            sal, K, radius, pct = g[name + "_map"][None], int(g[name + "_K"]), int(g[name + "_radius"]), float(g[name + "_pct"])
            gold_idx = g[name + "_idx"]
        kp, sc, idx, st = ora.select_keypoints(sal, K, radius, pct)
        if gold_idx is not None:
            assert st[0] == 0 and np.array_equal(idx[0], gold_idx), "the oracle on the fixture"
        _select[name] = (sal, K, radius, pct, kp, sc, idx, st, ora.patch_to_pixel(kp))
    return _select[name]


@pytest.mark.parametrize("optional", list(OPTIONAL))
@pytest.mark.parametrize("name", SELECT_TAGS + list(SELECT_SYNTH))
def test_select_keypoints(T, hip, name, optional):
    sal, K, radius, pct, kp, sc, idx, st, px = select_case(name)
    if name == "g7_k60":
        assert st.tolist() == [1, 1]
    n = sal.shape[0]
    want_idx, want_px = OPTIONAL[optional]
    b = Bufs(T)
    out = (b.o("kp_xy", (n, K, 2)), b.o("scores", (n, K)), b.o("idx", (n, K), T.int32) if want_idx else None,
           b.o("kp_pixel", (n, K, 2)) if want_px else None, b.o("status", (n,), T.int32))
    hip.select_keypoints(b.i("sal", sal), K, radius, pct, out=out)
    b.check(f"select_keypoints {name} {optional}")
    for got, want, what in zip(out, (kp, sc, idx, px, st), ("kp_xy", "scores", "idx", "kp_pixel", "status")):
        if got is not None:
            assert_bits(T, got, want, what)


# ================================================================================== A6 / A7 (refine.hip, refine_bf16.hip)
# 32-row MLP tiles (64 in the bf16 kernel): 1, 74 and 387 rows all end in a ragged tile, the last two in more than one workgroup.
# sslam_gather_refine_ws: SSLAM_REFINE_DISTINCT 0 = the direct launch (no workspace need: NULL), 1 = the distinct-row work list
# (four launches; workspace of exactly sslam_gather_refine_workspace_bytes, 0x00 and 0xFF).  Keypoints as in test_gpu_fuzz.py -
# fractional, integer, outside the grid - with the second half of every frame repeating the first bit for bit.
REF_SHAPES = [(8, 1, 1), (28, 37, 2), (28, 129, 3)]          # (G, K, frames)
_ref = {}


def _refiner_sd(width, depth):
    return synth.refiner_state(0, n_blocks=depth) if width == 128 else d256_cases.refiner_state(depth)


def ref_case(grid, K, frames, width=None, depth=None):
    base = (grid, K, frames)
    if base not in _ref:
        r = _rng(31 + grid + K)
        feat = r.standard_normal((frames, grid, grid, 384)).astype(np.float32)
        kp = (r.random((frames, K, 2)) * (grid + 3) - 2).astype(np.float32)
        kp[:, ::7] = np.floor(kp[:, ::7])
        if K > 1:
            kp[:, K - K // 2:] = kp[:, :K // 2]
        _ref[base] = dict(feat=feat, kp=kp, x=ora.gather(feat, kp))
    c = _ref[base]
    if width is not None and (width, depth) not in c:
        sd = _refiner_sd(width, depth)
        c[width, depth] = (sd, ora.refine(c["x"], sd, n_blocks=depth))
    return c


def _guard(width):
    return gd.GUARD_WIDE if width == 256 else gd.GUARD


@pytest.mark.parametrize("grid,K,frames", REF_SHAPES)
def test_gather(T, hip, grid, K, frames):
    c = ref_case(grid, K, frames)
    b = Bufs(T)
    out = b.o("out", (frames, K, 384))
    hip.gather(b.i("feat", c["feat"]), b.i("kp_xy", c["kp"]), out=out)
    b.check(f"gather G {grid} K {K} x {frames}")
    assert_bits(T, out, c["x"], "gather")


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("grid,K,frames", REF_SHAPES)
def test_refine(T, hip, grid, K, frames, width, depth):
    c = ref_case(grid, K, frames, width, depth)
    sd, want = c[width, depth]
    b = Bufs(T)
    out = b.o("desc", (frames, K, width), guard=_guard(width))
    hip.refine(b.i("x", c["x"]), b.i("packed", hip.pack_refiner(ora.refiner_weight_list(sd, depth), depth)), depth, out=out)
    b.check(f"refine {frames * K} rows width {width} depth {depth}")
    assert_bits(T, out, want, "refine")


@pytest.mark.parametrize("distinct", [0, 1])
@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("grid,K,frames", REF_SHAPES)
def test_gather_refine(T, hip, knob, grid, K, frames, width, depth, distinct):
    knob("SSLAM_REFINE_DISTINCT", distinct)
    c = ref_case(grid, K, frames, width, depth)
    sd, want = c[width, depth]
    packed = hip.pack_refiner(ora.refiner_weight_list(sd, depth), depth)
    need = int(hip.lib().sslam_gather_refine_workspace_bytes(frames, K))
    assert (need > 0) == bool(distinct)
    runs = []
    for fill in FILLS if need else FILLS[:1]:
        b = Bufs(T)
        out = b.o("desc", (frames, K, width), guard=_guard(width))
        ws = gd.dirty(T, need, fill)
        n0 = hip.launch_count()
        hip.gather_refine(b.i("feat", c["feat"]), b.i("kp_xy", c["kp"]), b.i("packed", packed), depth, out=out, workspace=ws if need else None)
        assert hip.launch_count() - n0 == (4 if distinct else 1), "the form the knob names"
        b.check(f"gather_refine G {grid} K {K} x {frames} width {width} depth {depth} distinct {distinct} workspace {fill:#04x}")
        assert_bits(T, out, want, "gather_refine")
        runs.append((out,))
    same_runs(T, runs, "gather_refine")


_refbf = {}


def refbf_case(grid, K, frames, depth):
    """depth 0: the order-free case of test_gpu_bf16_exact.py (keypoints on the half-integer lattice from -0.5 to G - 0.5, drawn
    with repetition) - the exact oracle's bits.  depth 2 has no bit-exact reference: the inputs of ref_case, held to the bars
    test_gpu_bf16_mode.py::test_gather_refine_bf16 sets that do not depend on the row count."""
    key = (grid, K, frames, depth)
    if key not in _refbf:
        if depth == 0:
            feat, kp, sd, x, _, desc, _ = orderfree.refiner_case(1000 * grid + frames * K, grid, frames, K)
            want = ora.refine(ora.gather(feat, kp).reshape(-1, 384), sd, n_blocks=0)
            assert np.array_equal(_bytes(want), _bytes(desc)), "the oracle sits on the builder's exact value"
            _refbf[key] = dict(feat=feat, kp=kp, x=x, sd=sd, want=want.reshape(frames, K, 128))
        else:
            c, sd = ref_case(grid, K, frames), synth.refiner_state(0)
            x = c["x"].reshape(-1, 384)
            _refbf[key] = dict(feat=c["feat"], kp=c["kp"], x=x, sd=sd, ref64=refine_bf16_ref(x, sd).reshape(frames, K, 128),
                               exact=ora.refine(c["x"], sd))
    return _refbf[key]


def _check_bf16_descriptors(T, c, out, what):
    if "want" in c:
        assert_bits(T, out, c["want"], what)
        return
    desc = _host(T, out)
    assert np.isfinite(desc).all(), what
    assert np.abs(desc - c["ref64"]).max() < 5e-3 and (desc * c["exact"]).sum(-1).min() > 0.999, what
    assert np.abs(np.sqrt((desc * desc).sum(-1)) - 1).max() < 1e-5, what


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("grid,K,frames", REF_SHAPES)
def test_refine_bf16_and_gather_refine_bf16(T, hip, grid, K, frames, depth):
    """Both bf16 entries, one guarded call each; at depth 2 also: the fused entry and the x_in entry give the same bits."""
    c = refbf_case(grid, K, frames, depth)
    packed = hip.pack_refiner_bf16(ora.refiner_weight_list(c["sd"], depth), depth)
    b = Bufs(T)
    rows = b.o("desc", (frames * K, 128))
    hip.refine_bf16(b.i("x", c["x"]), b.i("packed_bf16", packed), depth, out=rows)
    b.check(f"refine_bf16 {frames * K} rows depth {depth}")
    _check_bf16_descriptors(T, c, rows.view(frames, K, 128), "refine_bf16")
    b = Bufs(T)
    fused = b.o("desc", (frames, K, 128))
    hip.gather_refine_bf16(b.i("feat", c["feat"]), b.i("kp_xy", c["kp"]), b.i("packed_bf16", packed), depth, out=fused)
    b.check(f"gather_refine_bf16 G {grid} K {K} x {frames} depth {depth}")
    _check_bf16_descriptors(T, c, fused, "gather_refine_bf16")
    assert np.array_equal(_bytes(_host(T, fused)), _bytes(_host(T, rows))), "the fused entry and the x_in entry differ"


# =========================================================================================================== M1 (match.hip)
# launch_sim_argmax: the one-pass form (S once, 64-bit keys in the workspace, which the entry clears itself) under
# SSLAM_M1_VARIANT = 2 or by default from 16 pairs; the two-pass form under SSLAM_M1_VARIANT = 1 or below 16 pairs, no workspace.
# 128-row query blocks: (33, 70) one ragged block a side, (1, 300) and (128, 1) a single row / column, (129, 65) a second block of
# one row.  Pairs ride on the grid in rounds of eight: 3 and 17 are no multiples.  sim_argmax / sim_argmax_pairs have no out=:
# their C entries are called as the wrappers call them.
SIM_SHAPES = [(33, 70), (1, 300), (128, 1), (129, 65)]
SIM_FORMS = {"two_pass_3": (1, 3), "one_pass_3": (2, 3), "default_17": (None, 17)}          # SSLAM_M1_VARIANT, pairs
WANTS = {"s21_second": (True, True), "s21": (True, False), "second": (False, True), "neither": (False, False)}
_sim = {}


def _pair_arrays(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nn12, s12, nn21, s21 = ora.sim_argmax(a, b)
    S = ora.sim_matrix(a, b)
    S[np.arange(a.shape[0]), nn12] = -np.inf
    return nn12, s12, nn21, s21, S.max(1)


def sim_case(n1, n2, width, n_pairs):
    """n_pairs pairs of (n1, width) against (n2, width) - rotations of one descriptor pair with duplicated rows (exact ties) -
    with scores and intensities, and the oracle's five arrays stacked over the pairs."""
    key = (n1, n2, width, n_pairs)
    if key not in _sim:
        if len(_sim) > 6:
            _sim.clear()
        dup = 4 if min(n1, n2) >= 8 else 0
        d1, d2, s1, s2, i1, i2 = d256_cases.pair(900 + n1 + n2, n1, n2, dup, d=width)
        roll = lambda a, k: np.roll(a, k, axis=0)
        c = dict(d1=np.stack([roll(d1, p) for p in range(n_pairs)]), d2=np.stack([roll(d2, -2 * p) for p in range(n_pairs)]),
                 s1=np.stack([roll(s1, p) for p in range(n_pairs)]), s2=np.stack([roll(s2, -2 * p) for p in range(n_pairs)]),
                 i1=np.stack([roll(i1, p) for p in range(n_pairs)]), i2=np.stack([roll(i2, -2 * p) for p in range(n_pairs)]))
        per = [_pair_arrays(c["d1"][p], c["d2"][p]) for p in range(n_pairs)]
        for k, name in enumerate(("nn12", "s12", "nn21", "s21", "second12")):
            c[name] = np.stack([r[k] for r in per])
        _sim[key] = c
    return _sim[key]


def _sim_outputs(b, T, n_pairs, n1, n2, want_s21, want_second):
    return (b.o("nn12", (n_pairs, n1), T.int32), b.o("s12", (n_pairs, n1)), b.o("nn21", (n_pairs, n2), T.int32),
            b.o("s21", (n_pairs, n2)) if want_s21 else None, b.o("second12", (n_pairs, n1)) if want_second else None)


def _check_sim(T, out, c, names=("nn12", "s12", "nn21", "s21", "second12")):
    for got, name in zip(out, names):
        if got is not None:
            assert_bits(T, got, c[name], name)


@pytest.mark.parametrize("wants", list(WANTS))
@pytest.mark.parametrize("form", list(SIM_FORMS))
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("n1,n2", SIM_SHAPES)
def test_sim_argmax_strided(T, hip, knob, n1, n2, width, form, wants):
    variant, n_pairs = SIM_FORMS[form]
    if variant is not None:
        knob("SSLAM_M1_VARIANT", variant)
    c = sim_case(n1, n2, width, n_pairs)
    need = int(hip.lib().sslam_sim_argmax_workspace_bytes(n2, n_pairs))
    assert need == (0 if form == "two_pass_3" else n_pairs * n2 * 8)
    dp, runs = hip._dp, []
    for fill in FILLS if need else FILLS[:1]:
        b = Bufs(T)
        d1, d2 = b.i("desc1", c["d1"], guard=_guard(width)), b.i("desc2", c["d2"], guard=_guard(width))
        out = _sim_outputs(b, T, n_pairs, n1, n2, *WANTS[wants])
        ws = gd.dirty(T, need, fill) if need else None
        hip._run("sim_argmax", hip.lib().sslam_sim_argmax_ws_d, (d1, d2, out[0]), dp(d1), n1 * width, n1, dp(d2), n2 * width, n2, n_pairs,
                 *(dp(t) for t in out), dp(ws), need, width)
        b.check(f"sim_argmax ({n1}, {n2}) width {width} {form} {wants} workspace {fill:#04x}")
        _check_sim(T, out, c)
        runs.append(out)
    same_runs(T, runs, "sim_argmax")


# listed pairs over a bank of 4 frames (n1 = n2 = K): an absent pair (-1: zero rows), a repeated pair, a self pair
LISTS = {3: ([0, -1, 0], [1, 2, 1]),
         17: ([0, 1, 2, 3, 0, -1, 2, 3, 3, 1, 0, 2, 1, 3, 0, 1, 2], [1, 2, 3, 0, 2, 1, 2, 1, 0, 3, 1, 4, 0, 2, 1, 1, 0])}
LIST_K = [1, 33, 129]
_bank = {}


def bank_case(K, width, n_pairs):
    key = (K, width, n_pairs)
    if key not in _bank:
        if len(_bank) > 6:
            _bank.clear()
        dup = 4 if K >= 8 else 0
        base = d256_cases.pair(700 + K, K, K, dup, d=width)
        bank = np.stack([base[0], base[1], np.roll(base[0], 3, axis=0), np.roll(base[1], -5, axis=0)])
        r = _rng(K)
        c = dict(bank=bank, scores=(0.2 + 0.8 * r.random((4, K))).astype(np.float32), intensity=r.random((4, K)).astype(np.float32),
                 first=np.array(LISTS[n_pairs][0], np.int32), second=np.array(LISTS[n_pairs][1], np.int32))
        c["present"] = [(0 <= a < 4 and 0 <= s < 4) for a, s in zip(c["first"], c["second"])]
        assert not all(c["present"]) and len(set(zip(c["first"], c["second"]))) < n_pairs, "an absent and a repeated pair"
        zero = (np.zeros(K, np.int32), np.zeros(K, np.float32), np.zeros(K, np.int32), np.zeros(K, np.float32), np.zeros(K, np.float32))
        per = [_pair_arrays(bank[a], bank[s]) if ok else zero for a, s, ok in zip(c["first"], c["second"], c["present"])]
        for k, name in enumerate(("nn12", "s12", "nn21", "s21", "second12")):
            c[name] = np.stack([p[k] for p in per])
        _bank[key] = c
    return _bank[key]


@pytest.mark.parametrize("wants", ["s21_second", "neither"])
@pytest.mark.parametrize("form", list(SIM_FORMS))
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("K", LIST_K)
def test_sim_argmax_listed(T, hip, knob, K, width, form, wants):
    variant, n_pairs = SIM_FORMS[form]
    if variant is not None:
        knob("SSLAM_M1_VARIANT", variant)
    c = bank_case(K, width, n_pairs)
    need = int(hip.lib().sslam_sim_argmax_workspace_bytes(K, n_pairs))
    dp, runs = hip._dp, []
    for fill in FILLS if need else FILLS[:1]:
        b = Bufs(T)
        bank, first, second = b.i("bank", c["bank"], guard=_guard(width)), b.i("pair_first", c["first"]), b.i("pair_second", c["second"])
        out = _sim_outputs(b, T, n_pairs, K, K, *WANTS[wants])
        ws = gd.dirty(T, need, fill) if need else None
        hip._run("sim_argmax_pairs", hip.lib().sslam_sim_argmax_pairs_d, (bank, first, second, out[0]), dp(bank), K * width, 4, K, dp(first),
                 dp(second), n_pairs, *(dp(t) for t in out), dp(ws), need, width)
        b.check(f"sim_argmax_pairs K {K} width {width} {form} {wants} workspace {fill:#04x}")
        _check_sim(T, out, c)
        runs.append(out)
    same_runs(T, runs, "sim_argmax_pairs")


@pytest.mark.parametrize("want_second", [True, False], ids=["second", "no_second"])
@pytest.mark.parametrize("n_pairs", [3, 17])
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("n1,n2", SIM_SHAPES)
def test_sim_argmax_rows(T, hip, n1, n2, width, n_pairs, want_second):
    """One launch form, no workspace; s12 is optional in the C entry but the wrapper always asks for it."""
    c = sim_case(n1, n2, width, n_pairs)
    b = Bufs(T)
    d1, d2 = b.i("desc1", c["d1"], guard=_guard(width)), b.i("desc2", c["d2"], guard=_guard(width))
    out = (b.o("nn12", (n_pairs, n1), T.int32), b.o("s12", (n_pairs, n1)), b.o("second12", (n_pairs, n1)) if want_second else None)
    hip.sim_argmax_rows(d1, n1 * width, n1, d2, n2 * width, n2, n_pairs, out=out)
    b.check(f"sim_argmax_rows ({n1}, {n2}) width {width} x {n_pairs}")
    _check_sim(T, out, c, ("nn12", "s12", "second12"))


@pytest.mark.parametrize("want_second", [True, False], ids=["second", "no_second"])
@pytest.mark.parametrize("n_pairs", [3, 17])
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("K", LIST_K)
def test_sim_argmax_rows_pairs(T, hip, K, width, n_pairs, want_second):
    c = bank_case(K, width, n_pairs)
    b = Bufs(T)
    out = (b.o("nn12", (n_pairs, K), T.int32), b.o("s12", (n_pairs, K)), b.o("second12", (n_pairs, K)) if want_second else None)
    hip.sim_argmax_rows_pairs(b.i("bank", c["bank"], guard=_guard(width)), b.i("pair_first", c["first"]), b.i("pair_second", c["second"]), out=out)
    b.check(f"sim_argmax_rows_pairs K {K} width {width} x {n_pairs}")
    _check_sim(T, out, c, ("nn12", "s12", "second12"))


# ---- the four finalize kernels, on the oracle's arg-max arrays of the cases above (they read no descriptors: width 128) ------
from test_oracle_golden import RUNS          # noqa: E402  the M1 thresholds of test_match_with_quality

RULES = {mc.RATIO: 1, mc.MNN_RATIO: 2, mc.TRACKED: 3}          # lib.RULE_RATIO_BEST, RULE_RATIO_SECOND, RULE_TRACKED


def _full(n1, rows, values):
    """A finalize entry's fixed-capacity output of one pair: the kept rows, then zeros (include/sslam_hip.h)."""
    m, v = np.zeros((n1, 2), np.int64), np.zeros((n1,), np.float32)
    m[:len(rows)], v[:len(rows)] = rows, values
    return m, v, np.int32(len(rows))


def _stack(per):
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.array([p[2] for p in per], np.int32)


def _finalize_out(b, T, n_pairs, n1, value="quality"):
    return b.o("matches", (n_pairs, n1, 2), T.int64), b.o(value, (n_pairs, n1)), b.o("count", (n_pairs,), T.int32)


def _check_finalize(T, out, want, what):
    for got, w, name in zip(out, want, ("matches", "value", "count")):
        assert_bits(T, got, w, f"{what}: {name}")


def _m1_kw(run, i1, i2):
    kw = RUNS[run](i1, i2)
    sw = kw.get("saliency_weight", 0.3)
    return kw, (1.0 - sw, sw, kw.get("min_saliency", 0.2), kw.get("min_descriptor_sim", 0.7), kw.get("min_intensity", 0.1))


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("n_pairs", [3, 17])
@pytest.mark.parametrize("n1,n2", SIM_SHAPES)
def test_match_finalize(T, hip, n1, n2, n_pairs, run):
    c = sim_case(n1, n2, 128, n_pairs)
    per = []
    for p in range(n_pairs):
        kw, thr = _m1_kw(run, c["i1"][p], c["i2"][p])
        per.append(_full(n1, *ora.match_with_quality(c["d1"][p], c["d2"][p], c["s1"][p], c["s2"][p], **kw)))
    with_int = "intensity1" in kw
    b = Bufs(T)
    out = _finalize_out(b, T, n_pairs, n1)
    hip.match_finalize(b.i("nn12", c["nn12"]), b.i("s12", c["s12"]), b.i("nn21", c["nn21"]), n1, n2, n_pairs, b.i("scores1", c["s1"]), n1,
                       b.i("scores2", c["s2"]), n2, b.i("intensity1", c["i1"]) if with_int else None,
                       b.i("intensity2", c["i2"]) if with_int else None, *thr, out=out)
    b.check(f"match_finalize ({n1}, {n2}) x {n_pairs} {run}")
    _check_finalize(T, out, _stack(per), f"match_finalize {run}")


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("n_pairs", [3, 17])
@pytest.mark.parametrize("K", LIST_K)
def test_match_finalize_pairs(T, hip, K, n_pairs, run):
    c = bank_case(K, 128, n_pairs)
    per = []
    for a, s, ok in zip(c["first"], c["second"], c["present"]):
        kw, thr = _m1_kw(run, c["intensity"][a % 4], c["intensity"][s % 4])
        per.append(_full(K, *ora.match_with_quality(c["bank"][a], c["bank"][s], c["scores"][a], c["scores"][s], **kw)) if ok
                   else _full(K, np.zeros((0, 2), np.int64), np.zeros(0, np.float32)))
    b = Bufs(T)
    out = _finalize_out(b, T, n_pairs, K)
    hip.match_finalize_pairs(b.i("nn12", c["nn12"]), b.i("s12", c["s12"]), b.i("nn21", c["nn21"]), b.i("pair_first", c["first"]),
                             b.i("pair_second", c["second"]), b.i("scores_bank", c["scores"]),
                             b.i("intensity_bank", c["intensity"]) if "intensity1" in kw else None, *thr, out=out)
    b.check(f"match_finalize_pairs K {K} x {n_pairs} {run}")
    _check_finalize(T, out, _stack(per), f"match_finalize_pairs {run}")


def _rule_inputs(b, c, rule):
    tracked = rule == mc.TRACKED          # reads neither second12 nor nn21: NULL
    return (b.i("nn12", c["nn12"]), b.i("s12", c["s12"]), None if tracked else b.i("second12", c["second12"]),
            None if tracked else b.i("nn21", c["nn21"]))


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("n_pairs", [3, 17])
@pytest.mark.parametrize("n1,n2", SIM_SHAPES)
def test_match_finalize_rule(T, hip, n1, n2, n_pairs, rule):
    """Each rule at the middle threshold of tests/match_rules_cases.py.  M4 on one candidate (n2 = 1) is refused before anything
    is launched, as the original's np.sort(...)[:, 1] raises: the outputs stay untouched."""
    c = sim_case(n1, n2, 128, n_pairs)
    param = float(np.float32(mc.MIDDLE[rule]))
    b = Bufs(T)
    out = _finalize_out(b, T, n_pairs, n1, "value")
    args = (*_rule_inputs(b, c, rule), n1, n2, n_pairs, RULES[rule], param)
    if rule == mc.MNN_RATIO and n2 < 2:
        with pytest.raises(ValueError):
            hip.match_finalize_rule(*args, out=out)
        b.check(f"match_finalize_rule ({n1}, {n2}) {rule}, refused", unwritten=("matches", "value", "count"))
        return
    hip.match_finalize_rule(*args, out=out)
    b.check(f"match_finalize_rule ({n1}, {n2}) x {n_pairs} {rule}")
    want = _stack([_full(n1, *mc.oracle_rule(rule, c["d1"][p], c["d2"][p], param)) for p in range(n_pairs)])
    _check_finalize(T, out, want, f"match_finalize_rule {rule}")


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("n_pairs", [3, 17])
@pytest.mark.parametrize("K", LIST_K)
def test_match_finalize_rule_pairs(T, hip, K, n_pairs, rule):
    c = bank_case(K, 128, n_pairs)
    param = float(np.float32(mc.MIDDLE[rule]))
    b = Bufs(T)
    out = _finalize_out(b, T, n_pairs, K, "value")
    args = (*_rule_inputs(b, c, rule), b.i("pair_first", c["first"]), b.i("pair_second", c["second"]), 4, RULES[rule], param)
    if rule == mc.MNN_RATIO and K < 2:
        with pytest.raises(ValueError):
            hip.match_finalize_rule_pairs(*args, out=out)
        b.check(f"match_finalize_rule_pairs K {K} {rule}, refused", unwritten=("matches", "value", "count"))
        return
    hip.match_finalize_rule_pairs(*args, out=out)
    b.check(f"match_finalize_rule_pairs K {K} x {n_pairs} {rule}")
    want = _stack([_full(K, *mc.oracle_rule(rule, c["bank"][a], c["bank"][s], param)) if ok
                   else _full(K, np.zeros((0, 2), np.int64), np.zeros(0, np.float32))
                   for a, s, ok in zip(c["first"], c["second"], c["present"])])
    _check_finalize(T, out, want, f"match_finalize_rule_pairs {rule}")


# =============================================================================================================== f32_to_bf16
def _bf16_inputs(n):
    """Ties to even in both directions, +-0, subnormals, +-Inf, a NaN, the largest finite value (n = 8: one of each but -Inf and
    the negative subnormal), then seeded values over twelve decades."""
    special = np.array([1.00390625, 1.01171875, 0.0, -0.0, 1e-40, np.inf, np.nan, 3.4028235e38, -np.inf, -1e-40, -1.00390625,
                        -1.01171875, 65280.0, 1e-30], np.float32)
    special.view(np.uint32)[6] = 0x7FC00000
    r = _rng(n)
    a = (r.standard_normal(n) * 10.0 ** r.integers(-6, 6, n)).astype(np.float32)
    k = min(n, special.size)
    a[:k] = special[:k]
    return a


@pytest.mark.parametrize("n", [8, 8 * 257])
def test_f32_to_bf16(T, hip, n):
    a = _bf16_inputs(n)
    b = Bufs(T)
    out = b.o("out_bf16", (n,), T.bfloat16)
    hip.to_bf16(b.i("in", a), out=out)
    b.check(f"f32_to_bf16 n {n}")
    assert_bits(T, out, _bf16_bits(a), "f32_to_bf16")
    got = _host(T, out)
    assert (got[6] & 0x7F80) == 0x7F80 and (got[6] & 0x007F) != 0, "the NaN stays a NaN"
    assert got[2] == 0x0000 and got[3] == 0x8000 and got[5] == 0x7F80 and got[7] == 0x7F80, "+0, -0, +Inf; the largest finite rounds to +Inf"


# ============================================================================================== A1 (vit.hip, vit_f32.hip)
# No bit-exact oracle: the token output is guarded and fully written, a workspace of NaN bits (0xFF) and one of zeros give the
# same bits, and the tokens meet the bars of tests/test_gpu_vit_reference.py against oracle/ora_vit.py (its BARS, its check).
# Size 64 x 2 frames: T = 21 tokens, 42 rows (one ragged 128-row tile, one 64-key tile); size 144 x 1: T = 86 (two key tiles, the
# second ragged; the few-frame form cuts them into two ranges).  Both bf16 forms are named (sslam_vit_forward[_patches]_form),
# both fp32 attention forms (sslam_vit_forward_f32_form); the workspace has exactly the form's advertised size.
VIT_SHAPES = [(64, 2), (144, 1)]
_vit = {}


def vit_case(T, size, frames):
    import foreign_vit
    from oracle import ora_vit
    if "model" not in _vit:
        _vit["model"] = foreign_vit.random_vit(1).cuda()
    if (size, frames) not in _vit:
        x = T.randn(frames, 3, size, size, generator=T.Generator().manual_seed(size)).cuda()
        _vit[size, frames] = dict(x=x, bf16=ora_vit.forward(_vit["model"], x, "bf16"), exact=ora_vit.forward(_vit["model"], x, "exact"))
    return _vit["model"], _vit[size, frames]


def _hip_vit(T, cls, size):
    """The packed weights of the model (built once per class) with the RoPE tables of this grid, as forward_features sets them."""
    if cls.__name__ not in _vit:
        _vit[cls.__name__] = cls(_vit["model"])
    hv, g = _vit[cls.__name__], size // 16
    if g not in hv._rope:
        cos, sin = hv.vit.rope_tables(g, g, hv.device)
        hv._rope[g] = (cos.float().contiguous(), sin.float().contiguous())
    hv.w.rope_cos, hv.w.rope_sin = hv._rope[g][0].data_ptr(), hv._rope[g][1].data_ptr()
    return hv


@pytest.mark.parametrize("entry", ["images", "patches"])
@pytest.mark.parametrize("form", ["throughput", "few_frame"])
@pytest.mark.parametrize("size,frames", VIT_SHAPES)
def test_vit_forward_bf16(T, hip, size, frames, form, entry):
    import test_gpu_vit_reference as ref
    from sslam_amd.vit_hip import HipViT
    assert ref.BARS["bf16"] == (1.3e-2, 5e-5, 1.6e-2)
    model, c = vit_case(T, size, frames)
    hv, g = _hip_vit(T, HipViT, size), size // 16
    named = {"throughput": hip.VIT_FORM_THROUGHPUT, "few_frame": hip.VIT_FORM_FEW_FRAME}[form]
    need = hip.vit_workspace_bytes(frames, size, named)
    x = c["x"].cpu().numpy()
    if entry == "patches":          # the image rounded to bf16 once, as the patch rows of sslam_preprocess_u8_patches
        x = c["x"].reshape(frames, 3, g, 16, g, 16).permute(0, 2, 4, 1, 3, 5).reshape(frames, g * g, 768).bfloat16()
    runs = []
    for fill in FILLS:
        b = Bufs(T)
        d_x = b.i({"images": "images_chw", "patches": "patches_bf16"}[entry], x, guard=gd.GUARD_WIDE)
        out = b.o("tokens_out", (frames, 5 + g * g, 384), guard=gd.GUARD_WIDE)
        ws = gd.dirty(T, need, fill)
        if entry == "patches":
            hip.vit_forward_patches(d_x, size, hv.w, ws, out=out, form=named)
        else:
            hip.vit_forward(d_x, hv.w, ws, out=out, form=named)
        b.check(f"vit_forward {entry} {size} x {frames} {form} workspace {fill:#04x}")
        runs.append((out,))
    same_runs(T, runs, f"vit_forward {entry} {form}")
    ref._check(f"guarded bf16 {entry} {size}x{frames} {form}", runs[0][0], c["bf16"], "bf16")


@pytest.mark.parametrize("attention", ["one_pass", "key_split"])
@pytest.mark.parametrize("size,frames", VIT_SHAPES)
def test_vit_forward_f32(T, hip, size, frames, attention):
    import test_gpu_vit_reference as ref
    from sslam_amd.vit_hip import HipViTF32
    model, c = vit_case(T, size, frames)
    hv, g = _hip_vit(T, HipViTF32, size), size // 16
    need = hip.vit_f32_workspace_bytes(frames, size)
    runs = []
    for fill in FILLS:
        b = Bufs(T)
        out = b.o("tokens_out", (frames, 5 + g * g, 384), guard=gd.GUARD_WIDE)
        hip.vit_forward_f32(b.i("images_chw", c["x"].cpu().numpy(), guard=gd.GUARD_WIDE), hv.w, gd.dirty(T, need, fill), out=out,
                            attention_form={"one_pass": hip.ATTN_ONE_PASS, "key_split": hip.ATTN_KEY_SPLIT}[attention])
        b.check(f"vit_forward_f32 {size} x {frames} {attention} workspace {fill:#04x}")
        runs.append((out,))
    same_runs(T, runs, f"vit_forward_f32 {attention}")
    ref._check(f"guarded fp32 {size}x{frames} {attention}", runs[0][0], c["exact"], "f32")
