"""ctypes binding of the native libraries (include/*.h) for torch tensors.

Each library has a section below: its export list, its constants, its prototypes function and its wrappers.  How the libraries are
built and loaded is stated once, in the class Library and the table LIBRARIES at the end of this file: one row per library with
its symbol prefix, source directory, header, export list, the prerequisites outside its directory and its prototypes function.
lib(), ext(), ... , build(), ext_build(), ... and launch_count(), ext_launch_count(), ... are one-line definitions over that table.

PyTorch is used for device memory and streams only: every wrapper passes raw device pointers and the current
HIP stream to the C ABI.  There is NO fallback: if a library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(_PKG, "csrc")

OK, E_INVALID, E_UNSUPPORTED, E_LAUNCH = 0, -1, -2, -3
_ERR = {E_INVALID: "invalid argument", E_UNSUPPORTED: "unsupported shape", E_LAUNCH: "kernel launch failed"}

C_FEAT, HID, D_OUT = 384, 384, 128
WIDTHS = (128, 256)     # descriptor widths the kernels are built for; D_OUT is the default (include/sslam_hip.h, the _d entries)
MAX_TAPS = 32


class SslamHipError(RuntimeError):
    pass


class VitLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_g", "ln2_b", "wup", "bup",
                                          "wdown", "bdown", "wmlp")]


class VitWeights(C.Structure):
    _fields_ = [("patch_w", C.c_void_p), ("patch_b", C.c_void_p), ("prefix", C.c_void_p), ("layer", VitLayer * 12),
                ("norm_g", C.c_void_p), ("norm_b", C.c_void_p), ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p)]


class VitLayerF32(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ls1", "ln2_g", "ln2_b", "wup", "bup",
                                          "wdown", "bdown", "ls2")]


class VitWeightsF32(C.Structure):
    _fields_ = [("patch_w", C.c_void_p), ("patch_b", C.c_void_p), ("prefix", C.c_void_p), ("layer", VitLayerF32 * 12),
                ("norm_g", C.c_void_p), ("norm_b", C.c_void_p), ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p)]


class RefinerLayout(C.Structure):
    _fields_ = [("n_blocks", C.c_int), ("total", C.c_longlong), ("in_w", C.c_longlong), ("in_b", C.c_longlong),
                ("blk", (C.c_longlong * 8) * 8), ("out_w", C.c_longlong), ("out_b", C.c_longlong)]


_INCLUDE = os.path.join(os.path.dirname(_PKG), "include")
_MK = [os.path.join(CSRC, "flags.mk"), os.path.join(CSRC, "rules.mk")]      # every Makefile's rule depends on both


def _make_if_stale(csrc, so_path, others, force):
    """make -C csrc if so_path is missing or older than a .hip or .h of csrc, one of `others`, flags.mk or rules.mk, or if forced;
    -> so_path."""
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))] + others + _MK
    stale = (not os.path.exists(so_path)) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", csrc, "-s", "-j4"])
    return so_path


def _load(so_path, csrc, prefix, prototypes):
    """CDLL so_path with <prefix>_arch, <prefix>_launch_count and `prototypes` (a function of the library) set; raises if it has not
    been built (no silent fallback)."""
    if not os.path.exists(so_path):
        raise SslamHipError(f"{so_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            f"(or `make -C {csrc}`); this package has no non-HIP execution path")
    L = C.CDLL(so_path)
    getattr(L, prefix + "_arch").restype = C.c_char_p
    getattr(L, prefix + "_launch_count").restype = C.c_longlong
    prototypes(L)
    return L


@dataclasses.dataclass
class Library:
    """A row of LIBRARIES (at the end of this file): one native library, its source directory and how it is built and loaded."""
    name: str               # "lib", "ext", ...: the loader is the module function of that name
    prefix: str             # of every exported symbol, without the underscore
    directory: str          # the source directory, beside this package; its Makefile names the library OUT
    so: str                 # the file name of the shared object, built into the source directory
    header: str             # the public header, a file name under include/
    exports: list
    deps: tuple             # the prerequisites outside the directory, relative to it: the DEPS of its Makefile, the header among them
    prototypes: object      # a function of the loaded library that sets restype and argtypes
    handle: object = None   # the loaded library, once load() has run

    def __post_init__(self):
        self.csrc = os.path.join(_PKG, self.directory)
        self.so_path = os.path.join(self.csrc, self.so)
        self.header_path = os.path.join(_INCLUDE, self.header)
        self.prerequisites = [os.path.normpath(os.path.join(self.csrc, d)) for d in self.deps]

    def build(self, force: bool = False) -> str:
        """Compile the library for gfx950 in-tree if it is stale or forced (hipcc cross-compiles without a GPU); -> so_path."""
        return _make_if_stale(self.csrc, self.so_path, self.prerequisites, force)

    def load(self):
        """The loaded library, with its prototypes set; raises if it has not been built (no silent fallback)."""
        if self.handle is None:
            self.handle = _load(self.so_path, self.csrc, self.prefix, self.prototypes)
        return self.handle

    def launch_count(self) -> int:
        return int(getattr(self.load(), self.prefix + "_launch_count")())


EXPORTS = [
    "sslam_version", "sslam_arch", "sslam_launch_count", "sslam_pack_conv3x3_host", "sslam_pack_linear_host",
    "sslam_resample_table_host", "sslam_preprocess_u8", "sslam_bn_tokens", "sslam_selector_saliency",
    "sslam_select_keypoints", "sslam_gather", "sslam_refiner_layout", "sslam_refiner_pack_host", "sslam_refine",
    "sslam_gather_refine", "sslam_keypoint_intensity", "sslam_sim_argmax", "sslam_match_finalize",
    "sslam_vit_pack_linear_host", "sslam_vit_pack_mlp_host", "sslam_vit_workspace_bytes", "sslam_vit_forward",
    "sslam_f32_to_bf16", "sslam_pack_conv3x3_bf16_host", "sslam_selector_saliency_bf16",
    "sslam_bn_tokens_bf16copy", "sslam_refiner_bf16_bytes", "sslam_refiner_pack_bf16_host", "sslam_refine_bf16", "sslam_gather_refine_bf16",
    "sslam_workspace_bytes", "sslam_selector_saliency_workspace_bytes", "sslam_sim_argmax_workspace_bytes",
    "sslam_selector_saliency_ws", "sslam_sim_argmax_ws", "sslam_test_set_knob",
    "sslam_gather_refine_ws", "sslam_gather_refine_workspace_bytes",
    "sslam_preprocess_u8_patches", "sslam_vit_forward_patches", "sslam_vit_f32_workspace_bytes", "sslam_vit_forward_f32",
    "sslam_vit_f32_pack_linear_host", "sslam_vit_forward_f32_form",
    "sslam_vit_workspace_bytes_form", "sslam_vit_forward_form", "sslam_vit_forward_patches_form",
    "sslam_sim_argmax_pairs", "sslam_match_finalize_pairs", "sslam_selector_bf16_halo_groups",
    "sslam_match_finalize_rule", "sslam_match_finalize_rule_pairs", "sslam_sim_argmax_rows", "sslam_sim_argmax_rows_pairs",
    "sslam_row_lse", "sslam_row_lse_pairs", "sslam_edge_pool", "sslam_val_frame_stats", "sslam_val_pair_stats",
    "sslam_val_pair_stats_pairs",
    "sslam_refiner_layout_d", "sslam_refiner_pack_host_d", "sslam_refine_d", "sslam_gather_refine_d", "sslam_gather_refine_ws_d",
    "sslam_sim_argmax_d", "sslam_sim_argmax_ws_d", "sslam_sim_argmax_pairs_d", "sslam_sim_argmax_rows_d",
    "sslam_sim_argmax_rows_pairs_d", "sslam_row_lse_d", "sslam_row_lse_pairs_d", "sslam_val_frame_stats_d",
    "sslam_match_rank", "sslam_pose_nn_pairs", "sslam_match_score_pairs",
    "sslam_keypoint_depth", "sslam_pose_depth_nn_pairs", "sslam_match_score_known_pairs",
    "sslam_pose_ransac_pairs", "sslam_pose_refine_pairs",
]


def _prototypes(L):
    p, i, ll, f, d = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_double
    L.sslam_pack_conv3x3_host.argtypes = [p, i, p]
    L.sslam_pack_linear_host.argtypes = [p, i, i, p]
    L.sslam_resample_table_host.argtypes = [i, i, i, p, p, i]
    L.sslam_preprocess_u8.argtypes = [p, i, i, i, i, p, p, i, p, p, i, p, p]
    L.sslam_preprocess_u8_patches.argtypes = [p, i, i, i, i, p, p, i, p, p, i, p, p]
    L.sslam_bn_tokens.argtypes = [p, i, i, i, i, p, p, p, p, i, f, p, p, p, p]
    L.sslam_selector_saliency.argtypes = [p, i, i, p, p, p, p, i, p, p]
    L.sslam_selector_saliency_ws.argtypes = [p, i, i, p, p, p, p, i, p, p, ll, p]
    for fn, at in ((L.sslam_workspace_bytes, [i, i, i, i]), (L.sslam_selector_saliency_workspace_bytes, [i, i]),
                   (L.sslam_sim_argmax_workspace_bytes, [i, i]), (L.sslam_gather_refine_workspace_bytes, [i, i])):
        fn.restype, fn.argtypes = ll, at
    L.sslam_test_set_knob.argtypes = [C.c_char_p, ll, i]
    L.sslami_selector_border_plan.argtypes = [i, i, p, p]
    L.sslami_selector_border_owners.argtypes = [i, i, i, ll, i, p]
    L.sslami_selector_border_check.restype, L.sslami_selector_border_check.argtypes = ll, [i, i]
    L.sslam_select_keypoints.argtypes = [p, i, i, i, i, d, p, p, p, p, p, p]
    L.sslam_gather.argtypes = [p, i, i, p, i, p, p]
    L.sslam_refiner_layout.argtypes = [i, C.POINTER(RefinerLayout)]
    L.sslam_refiner_pack_host.argtypes = [p, i, p]
    L.sslam_refine.argtypes = [p, ll, p, i, p, p]
    L.sslam_gather_refine.argtypes = [p, i, i, p, i, p, i, p, p]
    L.sslam_gather_refine_ws.argtypes = [p, i, i, p, i, p, i, p, p, ll, p]
    L.sslam_keypoint_intensity.argtypes = [p, i, i, i, i, p, p, i, p, p, i, p, i, p, p]
    L.sslam_sim_argmax.argtypes = [p, ll, i, p, ll, i, i, p, p, p, p, p, p]
    L.sslam_sim_argmax_ws.argtypes = [p, ll, i, p, ll, i, i, p, p, p, p, p, p, ll, p]
    L.sslam_match_finalize.argtypes = [p, p, p, i, i, i, p, ll, p, ll, p, p, f, f, f, f, f, p, p, p, p]
    L.sslam_sim_argmax_pairs.argtypes = [p, ll, i, i, p, p, i, p, p, p, p, p, p, ll, p]
    L.sslam_match_finalize_pairs.argtypes = [p, p, p, i, i, p, p, i, p, ll, p, f, f, f, f, f, p, p, p, p]
    L.sslam_match_finalize_rule.argtypes = [p, p, p, p, i, i, i, i, f, p, p, p, p]
    L.sslam_match_finalize_rule_pairs.argtypes = [p, p, p, p, i, i, p, p, i, i, f, p, p, p, p]
    L.sslam_match_rank.argtypes = [p, p, p, i, i, i, i, p, p, p, p, p]
    L.sslam_pose_nn_pairs.argtypes = [p, i, i, i, i, p, p, i, p, d, p, p, p, p, p, p]
    L.sslam_match_score_pairs.argtypes = [p, p, p, p, p, i, i, p, p, p, p, p]
    L.sslam_keypoint_depth.argtypes = [p, i, i, i, p, i, d, d, p, p]
    L.sslam_pose_depth_nn_pairs.argtypes = [p, p, i, i, i, i, p, p, i, p] + [d] * 10 + [p, p, p, p, p, p, p]
    L.sslam_match_score_known_pairs.argtypes = [p, p, p, p, p, i, i, p, p, p, p, p, p]
    L.sslam_pose_ransac_pairs.argtypes = [p, p, i, i, p, p, i, p, p, i] + [d] * 10 + [i, C.c_uint64] + [p] * 7 + [p]
    L.sslam_pose_refine_pairs.argtypes = [p, p, i, i, p, p, i, p, p, i] + [d] * 10 + [p, d, i] + [p] * 12 + [p]
    L.sslam_sim_argmax_rows.argtypes = [p, ll, i, p, ll, i, i, p, p, p, p]
    L.sslam_sim_argmax_rows_pairs.argtypes = [p, ll, i, i, p, p, i, p, p, p, p]
    L.sslam_row_lse.argtypes = [p, ll, i, p, ll, i, i, p, f, p, p, p, p]
    L.sslam_row_lse_pairs.argtypes = [p, ll, i, i, p, p, i, p, f, p, p, p, p]
    L.sslam_edge_pool.argtypes = [p, i, i, p, p, p]
    L.sslam_val_frame_stats.argtypes = [p, p, p, p, i, i, i, p, p, p, p]
    L.sslam_val_pair_stats.argtypes = [p, p, i, p, p, p, p, p, i, i, i, f, p, p, p]
    L.sslam_val_pair_stats_pairs.argtypes = [p, i, i, p, p, p, p, p, p, p, i, i, f, p, p, p]
    # the width-taking forms: `int d` in front of the stream (of the output pointer in the host-side packers)
    L.sslam_refiner_layout_d.argtypes = [i, i, C.POINTER(RefinerLayout)]
    L.sslam_refiner_pack_host_d.argtypes = [p, i, i, p]
    for name in ("refine", "gather_refine", "gather_refine_ws", "sim_argmax", "sim_argmax_ws", "sim_argmax_pairs", "sim_argmax_rows",
                 "sim_argmax_rows_pairs", "row_lse", "row_lse_pairs", "val_frame_stats"):
        at = getattr(L, "sslam_" + name).argtypes
        getattr(L, f"sslam_{name}_d").argtypes = at[:-1] + [i, at[-1]]
    L.sslam_f32_to_bf16.argtypes = [p, p, ll, p]
    L.sslam_pack_conv3x3_bf16_host.argtypes = [p, i, p]
    L.sslam_selector_saliency_bf16.argtypes = [p, i, i, p, p, p, p, i, p, p]
    L.sslam_selector_bf16_halo_groups.argtypes = [i, i, i]
    L.sslam_bn_tokens_bf16copy.argtypes = [p, i, i, i, i, p, p, p, p, i, f, p, p, p, p, p]
    L.sslam_refiner_bf16_bytes.restype = C.c_longlong
    L.sslam_refiner_bf16_bytes.argtypes = [i]
    L.sslam_refiner_pack_bf16_host.argtypes = [p, i, p]
    L.sslam_refine_bf16.argtypes = [p, ll, p, i, p, p]
    L.sslam_gather_refine_bf16.argtypes = [p, i, i, p, i, p, i, p, p]
    L.sslam_vit_pack_linear_host.argtypes = [p, i, i, p]
    L.sslam_vit_pack_mlp_host.argtypes = [p, p, p, p]
    L.sslam_vit_workspace_bytes.restype = C.c_longlong
    L.sslam_vit_workspace_bytes.argtypes = [i, i]
    L.sslam_vit_forward.argtypes = [p, i, i, C.POINTER(VitWeights), p, ll, p, p]
    L.sslam_vit_forward_patches.argtypes = [p, i, i, C.POINTER(VitWeights), p, ll, p, p]
    L.sslam_vit_workspace_bytes_form.restype = C.c_longlong
    L.sslam_vit_workspace_bytes_form.argtypes = [i, i, i]
    L.sslam_vit_forward_form.argtypes = [p, i, i, C.POINTER(VitWeights), p, ll, p, i, p]
    L.sslam_vit_forward_patches_form.argtypes = [p, i, i, C.POINTER(VitWeights), p, ll, p, i, p]
    L.sslam_vit_f32_workspace_bytes.restype = C.c_longlong
    L.sslam_vit_f32_workspace_bytes.argtypes = [i, i]
    L.sslam_vit_forward_f32.argtypes = [p, i, i, C.POINTER(VitWeightsF32), p, ll, p, p]
    L.sslam_vit_forward_f32_form.argtypes = [p, i, i, C.POINTER(VitWeightsF32), p, ll, p, i, p]
    L.sslam_vit_f32_pack_linear_host.argtypes = [p, i, i, p]


def _check(rc: int, what: str):
    if rc != OK:
        if rc == E_INVALID:
            raise ValueError(f"{what}: {_ERR[rc]}")
        raise SslamHipError(f"{what}: {_ERR.get(rc, rc)}")


def common_device(*tensors):
    """The ONE CUDA device every tensor argument of a call lives on.  Raises ValueError for a CPU tensor or for tensors
    on different GPUs (the reference's torch ops raise a device-mismatch error there; handing a device-1 pointer to a
    device-0 stream would be a GPU memory fault instead)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"libsslam_hip takes CUDA tensors only, got a tensor on {t.device}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"tensor arguments on different devices: {dev} and {t.device}")
    if dev is None:
        raise ValueError("no device tensor among the arguments")
    return dev


def _run(what: str, fn, tensors, *args):
    """Call one C-ABI entry: all `tensors` must share a device; that device is made current for the call and the
    launch goes to ITS current stream (not the process-wide current device's)."""
    dev = common_device(*tensors)
    with torch.cuda.device(dev):
        _check(fn(*args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), what)


def _dp(t):
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous()):
        raise ValueError("device-resident contiguous tensor required")
    return C.c_void_p(t.data_ptr())


def check_width(d, what: str = "descriptor width") -> int:
    """d if the kernels are built for it (WIDTHS), else ValueError naming them."""
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or int(d) not in WIDTHS:
        raise ValueError(f"{what} must be one of {WIDTHS}, got {d!r}")
    return int(d)


def _operand_width(*named) -> int:
    """The one width of a call's descriptor operands ((name, tensor) pairs): the last dimension of each; a 1-D buffer stands for
    rows of the default width.  Unequal or unsupported widths: ValueError."""
    d = None
    for name, t in named:
        w = check_width(int(t.shape[-1]) if t.dim() >= 2 else D_OUT, f"the width of {name}")
        if d is not None and w != d:
            raise ValueError(f"descriptor operands of unequal width: {d} and {w}")
        d = w
    return d


_PACKED_WIDTH = {}      # (floats, n_blocks) -> width: refine / gather_refine ask on every call


def packed_refiner_width(packed, n_blocks: int) -> int:
    """The output width a packed refiner buffer was laid out for, from its length (refiner_layout(n_blocks, d).total)."""
    n = int(packed.numel())
    key = (n, int(n_blocks))
    if key not in _PACKED_WIDTH:
        _PACKED_WIDTH[key] = next((d for d in WIDTHS if n == int(refiner_layout(n_blocks, d).total)), None)
    if _PACKED_WIDTH[key] is not None:
        return _PACKED_WIDTH[key]
    raise ValueError(f"a packed refiner buffer of {n} floats fits no supported output width {WIDTHS} at {n_blocks} blocks")


def workspace_bytes(n_frames: int, G: int, K: int, n_pairs: int) -> int:
    """Bytes of caller-owned scratch that serve every *_ws entry of one pipeline step on one stream (include/sslam_hip.h)."""
    b = int(lib().sslam_workspace_bytes(n_frames, G, K, n_pairs))
    if b < 0:
        _check(b, "workspace_bytes")
    return b


def _scratch(workspace, need: int, device):
    """The caller's workspace tensor if it is large enough, else a fresh torch allocation (the library itself never allocates)."""
    if need <= 0:
        return None, 0
    if workspace is not None and workspace.numel() * workspace.element_size() >= need:
        return workspace, workspace.numel() * workspace.element_size()
    ws = torch.empty((need,), dtype=torch.uint8, device=device)
    return ws, need


class knobs:
    """TEST-ONLY: `with lib.knobs(SSLAM_CONV_TAIL=4): ...` overrides load-time knobs of the library for the block
    (sslam_test_set_knob) and restores their load-time values (environment at load, else the built-in defaults) afterwards.  Product code never uses it."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            _check(lib().sslam_test_set_knob(k.encode(), int(v), 0), f"set_knob({k})")
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            lib().sslam_test_set_knob(k.encode(), 0, 1)
        return False


# ------------------------------------------------------------------------------------------ host-side packing
def pack_conv3x3(w: np.ndarray) -> np.ndarray:
    w = np.ascontiguousarray(w, np.float32)
    hs = w.shape[0]
    assert w.shape == (hs, C_FEAT, 3, 3)
    out = np.empty(9 * C_FEAT * hs, np.float32)
    _check(lib().sslam_pack_conv3x3_host(w.ctypes.data, hs, out.ctypes.data), "pack_conv3x3")
    return out


def refiner_layout(n_blocks: int, d: int = D_OUT) -> RefinerLayout:
    """Offsets (floats) of the packed refiner buffer for output width d (128 or 256)."""
    lay = RefinerLayout()
    _check(lib().sslam_refiner_layout_d(n_blocks, check_width(d, "refiner output width"), C.byref(lay)), "refiner_layout")
    return lay


def pack_refiner(weights: list, n_blocks: int) -> np.ndarray:
    """weights: 4 + 8*n_blocks fp32 arrays in state_dict order (input_proj, blocks, output_proj); the output width is the
    row count of output_proj.weight (128 or 256)."""
    ws = [np.ascontiguousarray(w, np.float32) for w in weights]
    assert len(ws) == 4 + 8 * n_blocks
    d = check_width(int(ws[-2].shape[0]), "refiner output width")
    if ws[-2].shape != (d, HID) or ws[-1].shape != (d,):
        raise ValueError(f"output_proj of shapes {ws[-2].shape}, {ws[-1].shape}: ({d}, {HID}) and ({d},) expected")
    lay = refiner_layout(n_blocks, d)
    out = np.empty(lay.total, np.float32)
    arr = (C.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
    _check(lib().sslam_refiner_pack_host_d(arr, n_blocks, d, out.ctypes.data), "refiner_pack")
    return out


def pack_refiner_bf16(weights: list, n_blocks: int) -> np.ndarray:
    """bf16-mode image of the same weight list (LayerNorm folded into fc1 / fc2): uint8 buffer."""
    ws = [np.ascontiguousarray(w, np.float32) for w in weights]
    assert len(ws) == 4 + 8 * n_blocks
    out = np.empty(int(lib().sslam_refiner_bf16_bytes(n_blocks)), np.uint8)
    arr = (C.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
    _check(lib().sslam_refiner_pack_bf16_host(arr, n_blocks, out.ctypes.data), "refiner_pack_bf16")
    return out


def resample_table(in_size: int, out_size: int, bicubic: bool):
    bounds = np.empty(out_size * 2, np.int32)
    coefs = np.empty(out_size * MAX_TAPS, np.int32)
    ks = lib().sslam_resample_table_host(in_size, out_size, int(bicubic), bounds.ctypes.data, coefs.ctypes.data, coefs.size)
    if ks < 0:
        _check(ks, "resample_table")
    return bounds, coefs[: out_size * ks].copy(), ks


# ------------------------------------------------------------------------------------------------ device calls
def preprocess_u8(img, size, tab_h, tab_v, out=None):
    n, h, w, _ = img.shape
    assert img.dtype == torch.uint8
    if out is None:
        out = torch.empty((n, 3, size, size), dtype=torch.float32, device=img.device)
    (bh, ch, kh), (bv, cv, kv) = tab_h, tab_v
    _run("preprocess_u8", lib().sslam_preprocess_u8, (img, bh, ch, bv, cv, out,),
         _dp(img), n, h, w, size, _dp(bh), _dp(ch), kh, _dp(bv), _dp(cv), kv, _dp(out))
    return out


def preprocess_u8_patches(img, size, tab_h, tab_v, out=None):
    """A0 written as the ViT's patch-embedding operand: (n, (size/16)^2, 768) bf16 (include/sslam_hip.h).  Returns None where the
    tiled kernel does not cover the resampling ratio (callers then take preprocess_u8 + vit_forward)."""
    n, h, w, _ = img.shape
    assert img.dtype == torch.uint8 and size % 16 == 0
    if out is None:
        out = torch.empty((n, (size // 16) ** 2, 768), dtype=torch.bfloat16, device=img.device)
    (bh, ch, kh), (bv, cv, kv) = tab_h, tab_v
    dev = common_device(img, bh, ch, bv, cv, out)
    with torch.cuda.device(dev):
        rc = lib().sslam_preprocess_u8_patches(_dp(img), n, h, w, size, _dp(bh), _dp(ch), kh, _dp(bv), _dp(cv), kv, _dp(out),
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == E_UNSUPPORTED:
        return None
    _check(rc, "preprocess_u8_patches")
    return out


def bn_tokens(tokens, n_prefix, group, gamma, beta, run_mean, run_var, train, eps, out=None, want_stats=True, bf16_copy=False,
              out_bf16=None):
    """bf16_copy=True: returns (out, mean, var, out_bf16) - the bf16 copy is written by the same kernel pass (into out_bf16 if given)."""
    n, t, c = tokens.shape
    assert c == C_FEAT and tokens.dtype == torch.float32
    cells = t - n_prefix
    if out is None:
        out = torch.empty((n, cells, c), dtype=torch.float32, device=tokens.device)
    assert out.dtype == torch.float32 and out.numel() == n * cells * c and out.is_contiguous()
    mean = var = None
    if train and want_stats:
        mean = torch.empty((n // group, c), dtype=torch.float32, device=tokens.device)
        var = torch.empty_like(mean)
    if bf16_copy:
        out_bf = out_bf16 if out_bf16 is not None else torch.empty((n, cells, c), dtype=torch.bfloat16, device=tokens.device)
        assert out_bf.dtype == torch.bfloat16 and out_bf.numel() == n * cells * c and out_bf.is_contiguous()
        _run("bn_tokens_bf16copy", lib().sslam_bn_tokens_bf16copy, (tokens, gamma, beta, run_mean, run_var, out, out_bf, mean, var,),
         _dp(tokens), n, t, n_prefix, group, _dp(gamma), _dp(beta), _dp(run_mean),
                                              _dp(run_var), int(bool(train)), C.c_float(eps), _dp(out), _dp(out_bf), _dp(mean),
                                              _dp(var))
        return out, mean, var, out_bf
    _run("bn_tokens", lib().sslam_bn_tokens, (tokens, gamma, beta, run_mean, run_var, out, mean, var,),
         _dp(tokens), n, t, n_prefix, group, _dp(gamma), _dp(beta), _dp(run_mean), _dp(run_var),
                                 int(bool(train)), C.c_float(eps), _dp(out), _dp(mean), _dp(var))
    return out, mean, var


def selector_saliency(feat, w1p, b1, w2, b2, hs, out=None, workspace=None):
    """workspace: optional caller-owned scratch tensor (sslam_workspace_bytes); allocated here through torch if absent and
    the launch form needs one (few-frame calls only)."""
    n, g = feat.shape[0], feat.shape[1]
    if out is None:
        out = torch.empty((n, g, g), dtype=torch.float32, device=feat.device)
    ws, wsb = _scratch(workspace, int(lib().sslam_selector_saliency_workspace_bytes(n, g)), feat.device)
    _run("selector_saliency", lib().sslam_selector_saliency_ws, (feat, w1p, b1, w2, b2, out, ws),
         _dp(feat), n, g, _dp(w1p), _dp(b1), _dp(w2), _dp(b2), hs, _dp(out), _dp(ws), wsb)
    return out


def pack_conv3x3_bf16(w: np.ndarray) -> np.ndarray:
    """-> uint16 array holding the bf16 bit patterns (view it as torch.bfloat16 on the device)."""
    w = np.ascontiguousarray(w, np.float32)
    hs = w.shape[0]
    assert w.shape == (hs, C_FEAT, 3, 3)
    out = np.empty(9 * C_FEAT * hs, np.uint16)
    _check(lib().sslam_pack_conv3x3_bf16_host(w.ctypes.data, hs, out.ctypes.data), "pack_conv3x3_bf16")
    return out


def to_bf16(x, out=None):
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _run("f32_to_bf16", lib().sslam_f32_to_bf16, (x, out,),
         _dp(x), _dp(out), x.numel())
    return out


def selector_saliency_bf16(feat_bf16, w1p_bf16, b1, w2, b2, hs, out=None):
    n, g = feat_bf16.shape[0], feat_bf16.shape[1]
    if out is None:
        out = torch.empty((n, g, g), dtype=torch.float32, device=feat_bf16.device)
    _run("selector_saliency_bf16", lib().sslam_selector_saliency_bf16, (feat_bf16, w1p_bf16, b1, w2, b2, out,),
         _dp(feat_bf16), n, g, _dp(w1p_bf16), _dp(b1), _dp(w2), _dp(b2), hs, _dp(out))
    return out


def selector_bf16_halo_groups(n_frames: int, G: int, hs: int = 256) -> int:
    """The kernel selector_saliency_bf16 launches for this shape under the present knobs: 5..8 = halo form with that many
    64-row image groups, 0 = stage form (include/sslam_hip.h)."""
    np_ = int(lib().sslam_selector_bf16_halo_groups(n_frames, G, hs))
    if np_ < 0:
        _check(np_, "selector_bf16_halo_groups")
    return np_


BORDER_KINDS = ("big", "top", "bottom", "left", "right", "rest")


def selector_border_plan(n_frames: int, G: int):
    """The border-class tiling of the fp32 conv (csrc/selector.hip) for a launch: (applies, {kind: tiles}, {kind: most image rows a
    tile needs}).  `applies` False: the planner refuses the grid (the figures say why); host only."""
    tiles, rows = (C.c_longlong * 6)(), (C.c_int * 6)()
    rc = lib().sslami_selector_border_plan(n_frames, G, tiles, rows)
    if rc not in (OK, E_UNSUPPORTED):
        _check(rc, "selector_border_plan")
    return rc == OK, dict(zip(BORDER_KINDS, tiles)), dict(zip(BORDER_KINDS, rows))


def selector_border_check(n_frames: int, G: int) -> int:
    """Walks every tile of the plan as the kernel does: the (slot, tap) pairs whose image row is not the neighbour cell's, 0 if the
    geometry is right."""
    bad = int(lib().sslami_selector_border_check(n_frames, G))
    if bad < 0:
        _check(bad, "selector_border_check")
    return bad


def selector_border_owners(n_frames: int, G: int, kind: str) -> np.ndarray:
    """(tiles, slots, 3) int32: the (frame, y, x) every slot of every tile of `kind` computes, -1 for an empty slot."""
    ok, tiles, _ = selector_border_plan(n_frames, G)
    if not ok:
        raise SslamHipError(f"selector_border_owners: the border-class tiling does not apply to G = {G}")
    out = np.empty((tiles[kind], 128 if kind == "big" else 32, 3), np.int32)
    _check(lib().sslami_selector_border_owners(n_frames, G, BORDER_KINDS.index(kind), 0, tiles[kind], out.ctypes.data), "selector_border_owners")
    return out


def select_keypoints(sal, K, radius=2, pct=0.5, want_idx=True, want_pixel=True, out=None):
    """out: optional (kp, sc, idx, px, st) tensors to write into (a launch group's slice of the caller's buffers)."""
    n, g = sal.shape[0], sal.shape[1]
    dev = sal.device
    if out is not None:
        kp, sc, idx, px, st = out
    else:
        kp = torch.empty((n, K, 2), dtype=torch.float32, device=dev)
        sc = torch.empty((n, K), dtype=torch.float32, device=dev)
        idx = torch.empty((n, K), dtype=torch.int32, device=dev) if want_idx else None
        px = torch.empty((n, K, 2), dtype=torch.float32, device=dev) if want_pixel else None
        st = torch.empty((n,), dtype=torch.int32, device=dev)
    _run("select_keypoints", lib().sslam_select_keypoints, (sal, kp, sc, idx, px, st,),
         _dp(sal), n, g, K, radius, C.c_double(pct), _dp(kp), _dp(sc), _dp(idx), _dp(px),
                                        _dp(st))
    return kp, sc, idx, px, st


def gather(feat, kp, out=None):
    n, g = feat.shape[0], feat.shape[1]
    K = kp.shape[1]
    if out is None:
        out = torch.empty((n, K, C_FEAT), dtype=torch.float32, device=feat.device)
    _run("gather", lib().sslam_gather, (feat, kp, out,),
         _dp(feat), n, g, _dp(kp), K, _dp(out))
    return out


def refine(x, packed, n_blocks, out=None):
    """x (..., 384) -> descriptors (..., d), d the output width `packed` was laid out for (pack_refiner)."""
    rows = x.numel() // C_FEAT
    d = packed_refiner_width(packed, n_blocks)
    if out is None:
        out = torch.empty(x.shape[:-1] + (d,), dtype=torch.float32, device=x.device)
    elif out.numel() != rows * d:
        raise ValueError(f"out holds {out.numel()} floats, {rows} rows of width {d} expected")
    _run("refine", lib().sslam_refine_d, (x, packed, out,),
         _dp(x), rows, _dp(packed), n_blocks, _dp(out), d)
    return out


def gather_refine(feat, kp, packed, n_blocks, out=None, workspace=None):
    """workspace: optional caller-owned scratch tensor (sslam_workspace_bytes); allocated here through torch if absent and the
    launch form needs one (the distinct-row work list of launches beyond one round of MLP workgroups).  After such a launch
    the scratch starts with the int32 distinct-keypoint counts of the n frames and their sum (gather_refine_counts)."""
    n, g = feat.shape[0], feat.shape[1]
    K = kp.shape[1]
    d = packed_refiner_width(packed, n_blocks)
    if out is None:
        out = torch.empty((n, K, d), dtype=torch.float32, device=feat.device)
    elif out.numel() != n * K * d:
        raise ValueError(f"out holds {out.numel()} floats, ({n}, {K}, {d}) expected")
    ws, wsb = _scratch(workspace, int(lib().sslam_gather_refine_workspace_bytes(n, K)), feat.device)
    _run("gather_refine", lib().sslam_gather_refine_ws_d, (feat, kp, packed, out, ws),
         _dp(feat), n, g, _dp(kp), K, _dp(packed), n_blocks, _dp(out), _dp(ws), wsb, d)
    return out


def gather_refine_counts(workspace, n_frames: int):
    """(per-frame distinct-keypoint counts, their sum) that the last work-list gather_refine over n_frames left in `workspace`."""
    c = workspace[: 4 * (n_frames + 1)].view(torch.int32)
    return c[:n_frames], c[n_frames]


def gather_refine_bf16(feat, kp, packed_bf16, n_blocks, out=None):
    n, g = feat.shape[0], feat.shape[1]
    K = kp.shape[1]
    if out is None:
        out = torch.empty((n, K, D_OUT), dtype=torch.float32, device=feat.device)
    _run("gather_refine_bf16", lib().sslam_gather_refine_bf16, (feat, kp, packed_bf16, out,),
         _dp(feat), n, g, _dp(kp), K, _dp(packed_bf16), n_blocks, _dp(out))
    return out


def refine_bf16(x, packed_bf16, n_blocks, out=None):
    rows = x.shape[0]
    if out is None:
        out = torch.empty((rows, D_OUT), dtype=torch.float32, device=x.device)
    _run("refine_bf16", lib().sslam_refine_bf16, (x, packed_bf16, out,),
         _dp(x), rows, _dp(packed_bf16), n_blocks, _dp(out))
    return out


def keypoint_intensity(img, size, tab_h, tab_v, kp_pixel, out=None):
    n, h, w, _ = img.shape
    K = kp_pixel.shape[1]
    if out is None:
        out = torch.empty((n, K), dtype=torch.float32, device=img.device)
    (bh, ch, kh), (bv, cv, kv) = tab_h, tab_v
    _run("keypoint_intensity", lib().sslam_keypoint_intensity, (img, bh, ch, bv, cv, kp_pixel, out,),
         _dp(img), n, h, w, size, _dp(bh), _dp(ch), kh, _dp(bv), _dp(cv), kv, _dp(kp_pixel), K,
                                          _dp(out))
    return out


def sim_argmax(d1, stride1, n1, d2, stride2, n2, n_pairs, want_s21=False, want_second=False, workspace=None):
    """workspace: optional caller-owned scratch tensor (sslam_workspace_bytes); batched calls without one get a torch
    allocation of n_pairs * n2 * 8 bytes here - the library itself never allocates."""
    dev = d1.device
    d = _operand_width(("d1", d1), ("d2", d2))
    nn12 = torch.empty((n_pairs, n1), dtype=torch.int32, device=dev)
    s12 = torch.empty((n_pairs, n1), dtype=torch.float32, device=dev)
    nn21 = torch.empty((n_pairs, n2), dtype=torch.int32, device=dev)
    s21 = torch.empty((n_pairs, n2), dtype=torch.float32, device=dev) if want_s21 else None
    sec = torch.empty((n_pairs, n1), dtype=torch.float32, device=dev) if want_second else None
    ws, wsb = _scratch(workspace, int(lib().sslam_sim_argmax_workspace_bytes(n2, n_pairs)), dev)
    _run("sim_argmax", lib().sslam_sim_argmax_ws_d, (nn12, s12, nn21, s21, sec, d1, d2, ws),
         C.c_void_p(d1.data_ptr()), stride1, n1, C.c_void_p(d2.data_ptr()), stride2, n2, n_pairs,
                                  _dp(nn12), _dp(s12), _dp(nn21), _dp(s21), _dp(sec), _dp(ws), wsb, d)
    return nn12, s12, nn21, s21, sec


def match_finalize(nn12, s12, nn21, n1, n2, n_pairs, sc1, ss1, sc2, ss2, in1, in2, w_desc, w_sal, t_sal, t_sim, t_int, out=None):
    """out: optional (matches, quality, count) tensors to write into."""
    dev = nn12.device
    if out is not None:
        matches, quality, count = out
    else:
        matches = torch.empty((n_pairs, n1, 2), dtype=torch.int64, device=dev)
        quality = torch.empty((n_pairs, n1), dtype=torch.float32, device=dev)
        count = torch.empty((n_pairs,), dtype=torch.int32, device=dev)
    f = C.c_float
    _run("match_finalize", lib().sslam_match_finalize, (nn12, s12, nn21, matches, quality, count, sc1, sc2, in1, in2,),
         _dp(nn12), _dp(s12), _dp(nn21), n1, n2, n_pairs, C.c_void_p(sc1.data_ptr()), ss1,
                                      C.c_void_p(sc2.data_ptr()), ss2,
                                      None if in1 is None else C.c_void_p(in1.data_ptr()),
                                      None if in2 is None else C.c_void_p(in2.data_ptr()),
                                      f(w_desc), f(w_sal), f(t_sal), f(t_sim), f(t_int), _dp(matches), _dp(quality),
                                      _dp(count))
    return matches, quality, count


def check_pair_lists(first, second, device=None) -> int:
    """The two index lists of a pair-list call: 1-D int32 tensors of one length, contiguous, on `device` when it is given.
    Raises ValueError, touching no device; returns the number of pairs.  The VALUES are the kernels' business (an index outside
    the bank makes an absent pair): the host never reads them."""
    for name, t in (("first", first), ("second", second)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"pair list `{name}` must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise ValueError(f"pair list `{name}` must be int32, got {t.dtype}")
        if t.dim() != 1:
            raise ValueError(f"pair list `{name}` must be 1-D, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"pair list `{name}` must be contiguous")
    if first.shape[0] != second.shape[0]:
        raise ValueError(f"pair lists of unequal length: {first.shape[0]} and {second.shape[0]}")
    if first.shape[0] == 0:
        raise ValueError("empty pair list")
    if device is not None:
        for name, t in (("first", first), ("second", second)):
            if t.device != device:
                raise ValueError(f"pair list `{name}` is on {t.device}, the bank on {device}")
    return int(first.shape[0])


def _check_bank(name, t, tail):
    """t: a contiguous fp32 tensor (n_bank >= 1, *tail); a tail entry given as a string stands for any size >= 1, one given as a
    tuple for any of its sizes (the descriptor widths)."""
    fits = lambda d, w: isinstance(w, str) or (d in w if isinstance(w, tuple) else d == w)
    ok = isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 1 + len(tail) and t.is_contiguous()
    ok = ok and all(d >= 1 for d in t.shape) and all(fits(d, w) for d, w in zip(t.shape[1:], tail))
    if not ok:
        shape = ", ".join(" | ".join(str(x) for x in w) if isinstance(w, tuple) else str(w) for w in tail)
        raise ValueError(f"{name} must be a contiguous fp32 tensor of shape (n_bank, {shape})")


def sim_argmax_pairs(bank, first, second, want_s21=False, want_second=False, workspace=None):
    """sslam_sim_argmax_pairs: bank (n_bank, K, 128 | 256) fp32; first / second: 1-D int32 DEVICE tensors naming, pair by pair, the
    two frames of the bank to match (an index outside [0, n_bank), -1 by convention, makes the pair ABSENT: zero rows).
    Returns (nn12, s12, nn21, s21, second12) with one row per listed pair, as sim_argmax does.  workspace: as there."""
    _check_bank("bank", bank, ("K", WIDTHS))
    n_bank, k = int(bank.shape[0]), int(bank.shape[1])
    n_pairs = check_pair_lists(first, second, bank.device)
    dev = common_device(bank, first, second, workspace)
    nn12 = torch.empty((n_pairs, k), dtype=torch.int32, device=dev)
    s12 = torch.empty((n_pairs, k), dtype=torch.float32, device=dev)
    nn21 = torch.empty((n_pairs, k), dtype=torch.int32, device=dev)
    s21 = torch.empty((n_pairs, k), dtype=torch.float32, device=dev) if want_s21 else None
    sec = torch.empty((n_pairs, k), dtype=torch.float32, device=dev) if want_second else None
    ws, wsb = _scratch(workspace, int(lib().sslam_sim_argmax_workspace_bytes(k, n_pairs)), dev)
    d = int(bank.shape[2])
    _run("sim_argmax_pairs", lib().sslam_sim_argmax_pairs_d, (bank, first, second, nn12, s12, nn21, s21, sec, ws),
         _dp(bank), k * d, n_bank, k, _dp(first), _dp(second), n_pairs, _dp(nn12), _dp(s12), _dp(nn21), _dp(s21), _dp(sec),
         _dp(ws), wsb, d)
    return nn12, s12, nn21, s21, sec


def match_finalize_pairs(nn12, s12, nn21, first, second, scores, intensity, w_desc, w_sal, t_sal, t_sim, t_int, out=None):
    """sslam_match_finalize_pairs: the arg-max arrays of sim_argmax_pairs over the same two lists; scores (n_bank, K) and
    intensity (n_bank, K) or None are the banks those lists index.  out: optional (matches, quality, count) to write into."""
    _check_bank("scores", scores, ("K",))
    n_bank, k = int(scores.shape[0]), int(scores.shape[1])
    if intensity is not None:
        _check_bank("intensity", intensity, (k,))
        if intensity.shape[0] != n_bank:
            raise ValueError(f"intensity holds {intensity.shape[0]} frames, scores {n_bank}")
    n_pairs = check_pair_lists(first, second, scores.device)
    for name, t, dt in (("nn12", nn12, torch.int32), ("s12", s12, torch.float32), ("nn21", nn21, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (n_pairs, k) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {(n_pairs, k)}")
    dev = scores.device
    if out is not None:
        matches, quality, count = out
        for name, t, dt, sh in (("matches", matches, torch.int64, (n_pairs, k, 2)), ("quality", quality, torch.float32, (n_pairs, k)),
                                ("count", count, torch.int32, (n_pairs,))):
            if t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous():
                raise ValueError(f"out `{name}` must be a contiguous {dt} tensor of shape {sh}")
    else:
        matches = torch.empty((n_pairs, k, 2), dtype=torch.int64, device=dev)
        quality = torch.empty((n_pairs, k), dtype=torch.float32, device=dev)
        count = torch.empty((n_pairs,), dtype=torch.int32, device=dev)
    f = C.c_float
    _run("match_finalize_pairs", lib().sslam_match_finalize_pairs, (nn12, s12, nn21, first, second, scores, intensity, matches, quality, count),
         _dp(nn12), _dp(s12), _dp(nn21), k, n_bank, _dp(first), _dp(second), n_pairs, _dp(scores), k, _dp(intensity),
         f(w_desc), f(w_sal), f(t_sal), f(t_sim), f(t_int), _dp(matches), _dp(quality), _dp(count))
    return matches, quality, count


# rules of the sibling matchers the finalize stage can apply in place of M1's (include/sslam_hip.h)
RULE_RATIO_BEST, RULE_RATIO_SECOND, RULE_TRACKED = 1, 2, 3


def _check_arrays(shape, *named):
    """named: (name, tensor or None, dtype); every tensor given must be contiguous, of that dtype and of `shape`."""
    for name, t, dt in named:
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape}")


def _rows_out(out, n_pairs, n1, want_second, dev):
    if out is None:
        return (torch.empty((n_pairs, n1), dtype=torch.int32, device=dev), torch.empty((n_pairs, n1), dtype=torch.float32, device=dev),
                torch.empty((n_pairs, n1), dtype=torch.float32, device=dev) if want_second else None)
    nn12, s12, sec = out
    if nn12 is None:
        raise ValueError("out `nn12` is required")
    _check_arrays((n_pairs, n1), ("out `nn12`", nn12, torch.int32), ("out `s12`", s12, torch.float32), ("out `second12`", sec, torch.float32))
    return nn12, s12, sec


def sim_argmax_rows(d1, stride1, n1, d2, stride2, n2, n_pairs, want_second=False, out=None):
    """sslam_sim_argmax_rows: the row direction of sim_argmax alone - one launch, no workspace, the same bits.
    Returns (nn12, s12, second12 or None).  out: optional (nn12, s12, second12 or None) tensors to write into."""
    nn12, s12, sec = _rows_out(out, n_pairs, n1, want_second, d1.device)
    d = _operand_width(("d1", d1), ("d2", d2))
    _run("sim_argmax_rows", lib().sslam_sim_argmax_rows_d, (nn12, s12, sec, d1, d2),
         C.c_void_p(d1.data_ptr()), stride1, n1, C.c_void_p(d2.data_ptr()), stride2, n2, n_pairs, _dp(nn12), _dp(s12), _dp(sec), d)
    return nn12, s12, sec


def sim_argmax_rows_pairs(bank, first, second, want_second=False, out=None):
    """sslam_sim_argmax_rows_pairs: the row direction of sim_argmax_pairs alone (bank and lists as there).
    Returns (nn12, s12, second12 or None), one row per listed pair.  out: optional tensors to write into, as sim_argmax_rows."""
    _check_bank("bank", bank, ("K", WIDTHS))
    n_bank, k = int(bank.shape[0]), int(bank.shape[1])
    n_pairs = check_pair_lists(first, second, bank.device)
    dev = common_device(bank, first, second)
    nn12, s12, sec = _rows_out(out, n_pairs, k, want_second, dev)
    d = int(bank.shape[2])
    _run("sim_argmax_rows_pairs", lib().sslam_sim_argmax_rows_pairs_d, (bank, first, second, nn12, s12, sec),
         _dp(bank), k * d, n_bank, k, _dp(first), _dp(second), n_pairs, _dp(nn12), _dp(s12), _dp(sec), d)
    return nn12, s12, sec


def _check_rule_arrays(rule, n_pairs, n1, n2, nn12, s12, second12, nn21):
    """The arg-max arrays a rule's finalize kernel reads, row for row: a short or mistyped one would be read past its end."""
    for name, t in (("nn12", nn12), ("s12", s12)) + ((("second12", second12), ("nn21", nn21)) if int(rule) != RULE_TRACKED else ()):
        if t is None:
            raise ValueError(f"{name} is required by this rule")
    _check_arrays((n_pairs, n1), ("nn12", nn12, torch.int32), ("s12", s12, torch.float32), ("second12", second12, torch.float32))
    _check_arrays((n_pairs, n2), ("nn21", nn21, torch.int32))


def _rule_out(out, n_pairs, n1, dev):
    if out is not None:
        matches, value, count = out
        for name, t, dt, sh in (("matches", matches, torch.int64, (n_pairs, n1, 2)), ("value", value, torch.float32, (n_pairs, n1)),
                                ("count", count, torch.int32, (n_pairs,))):
            if t is None:
                raise ValueError(f"out `{name}` is required")
            _check_arrays(sh, (f"out `{name}`", t, dt))
        return matches, value, count
    return (torch.empty((n_pairs, n1, 2), dtype=torch.int64, device=dev), torch.empty((n_pairs, n1), dtype=torch.float32, device=dev),
            torch.empty((n_pairs,), dtype=torch.int32, device=dev))


def match_finalize_rule(nn12, s12, second12, nn21, n1, n2, n_pairs, rule, param, out=None):
    """sslam_match_finalize_rule: rule RULE_RATIO_BEST (M2) / RULE_RATIO_SECOND (M4) / RULE_TRACKED (M5) with its fp32 parameter
    on the arg-max arrays of sim_argmax (want_second=True) - or of sim_argmax_rows for RULE_TRACKED, which reads neither second12
    nor nn21 (pass None).  Returns (matches, value, count); out: optional tensors of those shapes to write into."""
    _check_rule_arrays(rule, n_pairs, n1, n2, nn12, s12, second12, nn21)
    matches, value, count = _rule_out(out, n_pairs, n1, nn12.device)
    _run("match_finalize_rule", lib().sslam_match_finalize_rule, (nn12, s12, second12, nn21, matches, value, count),
         _dp(nn12), _dp(s12), _dp(second12), _dp(nn21), n1, n2, n_pairs, int(rule), C.c_float(param), _dp(matches), _dp(value),
         _dp(count))
    return matches, value, count


def match_finalize_rule_pairs(nn12, s12, second12, nn21, first, second, n_bank, rule, param, out=None):
    """sslam_match_finalize_rule_pairs: match_finalize_rule on the arrays of sim_argmax_pairs / sim_argmax_rows_pairs over the
    same two lists into a bank of n_bank frames (the lists only tell which pairs are absent: count 0, zero rows)."""
    n_pairs = check_pair_lists(first, second, nn12.device if isinstance(nn12, torch.Tensor) else None)
    if not isinstance(nn12, torch.Tensor) or nn12.dim() != 2 or nn12.shape[0] != n_pairs:
        raise ValueError(f"nn12 must be a tensor of shape ({n_pairs}, K)")
    k = int(nn12.shape[1])
    _check_rule_arrays(rule, n_pairs, k, k, nn12, s12, second12, nn21)
    matches, value, count = _rule_out(out, n_pairs, k, nn12.device)
    _run("match_finalize_rule_pairs", lib().sslam_match_finalize_rule_pairs, (nn12, s12, second12, nn21, first, second, matches, value, count),
         _dp(nn12), _dp(s12), _dp(second12), _dp(nn21), k, int(n_bank), _dp(first), _dp(second), n_pairs, int(rule), C.c_float(param),
         _dp(matches), _dp(value), _dp(count))
    return matches, value, count


RANK_MAX_N1 = 4096      # SSLAM_RANK_MAX_N1: the longest list sslam_match_rank ranks (a pair's keys live in LDS)


def check_best(best, n1: int) -> int:
    """`best` of a rank call as an int in [1, n1] (None: all n1 rows), else ValueError - before any device work."""
    if best is None:
        return int(n1)
    if isinstance(best, bool) or not isinstance(best, (int, np.integer)) or not 1 <= int(best) <= int(n1):
        raise ValueError(f"best must be None or an int in [1, {int(n1)}], got {best!r}")
    return int(best)


def match_rank(matches, value, count, best=None, ascending=False, out=None, want_slot=True):
    """sslam_match_rank: the `best` best rows of every pair's match list, better value first (larger; smaller with ascending=True:
    a cosine distance), equal values in ascending input slot, NaN rows last (include/sslam_hip.h states the order).
    matches (P, n1, 2) int64, value (P, n1) fp32, count (P,) int32: what a finalize entry wrote.  best=None ranks all n1 rows.
    Returns (matches (P, best, 2), value (P, best), count (P,) = min(count, best), slot (P, best) int32 or None): rows past the
    count are zero; slot names the input row each kept row came from.  out: optional tensors of those shapes to write into (slot
    None, or want_slot=False, for no slot array).  One launch, no host read."""
    if not isinstance(matches, torch.Tensor) or matches.dim() != 3 or matches.shape[2] != 2 or matches.shape[0] < 1 or matches.shape[1] < 1:
        raise ValueError("matches must be a tensor of shape (n_pairs >= 1, n1 >= 1, 2)")
    n_pairs, n1 = int(matches.shape[0]), int(matches.shape[1])
    _check_arrays((n_pairs, n1, 2), ("matches", matches, torch.int64))
    for name, t in (("value", value), ("count", count)):
        if t is None:
            raise ValueError(f"{name} is required")
    _check_arrays((n_pairs, n1), ("value", value, torch.float32))
    _check_arrays((n_pairs,), ("count", count, torch.int32))
    best = check_best(best, n1)
    if not isinstance(ascending, (bool, np.bool_)):
        raise ValueError(f"ascending must be a bool, got {ascending!r}")
    if n1 > RANK_MAX_N1:
        raise SslamHipError(f"match_rank: lists of {n1} rows; at most {RANK_MAX_N1} are ranked on the device")
    dev = matches.device
    if out is not None:
        o_m, o_v, o_c, o_s = out
        for name, t in (("matches", o_m), ("value", o_v), ("count", o_c)):
            if t is None:
                raise ValueError(f"out `{name}` is required")
        _check_arrays((n_pairs, best, 2), ("out `matches`", o_m, torch.int64))
        _check_arrays((n_pairs, best), ("out `value`", o_v, torch.float32), ("out `slot`", o_s, torch.int32))
        _check_arrays((n_pairs,), ("out `count`", o_c, torch.int32))
    else:
        o_m = torch.empty((n_pairs, best, 2), dtype=torch.int64, device=dev)
        o_v = torch.empty((n_pairs, best), dtype=torch.float32, device=dev)
        o_c = torch.empty((n_pairs,), dtype=torch.int32, device=dev)
        o_s = torch.empty((n_pairs, best), dtype=torch.int32, device=dev) if want_slot else None
    _run("match_rank", lib().sslam_match_rank, (matches, value, count, o_m, o_v, o_c, o_s),
         _dp(matches), _dp(value), _dp(count), n1, n_pairs, best, int(ascending), _dp(o_m), _dp(o_v), _dp(o_c), _dp(o_s))
    return o_m, o_v, o_c, o_s


# ------------------------------------------------------------------------------------------------ pose-based scoring
EVAL_MAX_K = 4096       # SSLAM_EVAL_MAX_K: the most keypoints per frame sslam_pose_nn_pairs searches (a pair's distances live in LDS)
POSE_SCORE_KEYS = ("gt_matches", "gt_count", "gt_of_row", "dist_sum", "dist_median")
MATCH_SCORE_KEYS = ("tp", "fp", "fn", "value_sum")


def check_threshold(threshold) -> float:
    """The pixel threshold of pose_nn_pairs as a float: finite and >= 0, else ValueError - before any device work."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.floating, np.integer)):
        raise ValueError(f"threshold must be a number, got {threshold!r}")
    t = float(threshold)
    if not (np.isfinite(t) and t >= 0.0):
        raise ValueError(f"threshold must be finite and >= 0, got {threshold!r}")
    return t


def pose_score_shapes(n_pairs: int, n1: int) -> dict:
    """name -> (shape, dtype) of the outputs of pose_nn_pairs and match_score_pairs for n_pairs pairs of n1 query rows."""
    return {"gt_matches": ((n_pairs, n1, 2), torch.int64), "gt_count": ((n_pairs,), torch.int32),
            "gt_of_row": ((n_pairs, n1), torch.int32), "dist_sum": ((n_pairs,), torch.float64),
            "dist_median": ((n_pairs,), torch.float64), "tp": ((n_pairs,), torch.int32), "fp": ((n_pairs,), torch.int32),
            "fn": ((n_pairs,), torch.int32), "value_sum": ((n_pairs,), torch.float64)}


def _outputs(shapes, keys, out, dev=None):
    """The output tensors of a call, in the order of `keys`: `out` checked against `shapes` (name -> (shape, dtype); no device
    needed), or fresh ones on dev."""
    if out is None:
        return [torch.empty(shapes[key][0], dtype=shapes[key][1], device=dev) for key in keys]
    if len(out) != len(keys):
        raise ValueError(f"out must hold {len(keys)} tensors: {', '.join(keys)}")
    for key, t in zip(keys, out):
        if t is None:
            raise ValueError(f"out `{key}` is required")
        _check_arrays(shapes[key][0], (f"out `{key}`", t, shapes[key][1]))
    return list(out)


def _pose_operands(what, kp_bank, first, second, threshold, depth=None, rows=None, listed=None):
    """The operands the bank-and-pairs wrappers share, checked before any device work: the bank kp_bank (n_bank, K, 2), the pair
    lists and the threshold; depth: (kp_depth_bank, camera, scale_x, scale_y) of a wrapper that takes them; rows: (n1, n2) of a
    search, None standing for K - or listed: (matches, count), a match list of n1 slots per pair; K against EVAL_MAX_K.
    Returns (n_bank, k, n_pairs, n1, n2 - None for a list -, the C doubles every such entry takes in this order: with depth fx, fy,
    cx, cy, depth_scale, scale_x, scale_y, view_w, view_h, then the threshold)."""
    _check_bank("kp_bank", kp_bank, ("K", 2))
    n_bank, k = int(kp_bank.shape[0]), int(kp_bank.shape[1])
    if depth is not None:
        if depth[0] is None:
            raise ValueError("kp_depth_bank is required")
        _check_arrays((n_bank, k), ("kp_depth_bank", depth[0], torch.int32))
    n_pairs = check_pair_lists(first, second, kp_bank.device)
    if listed is None:
        n1, n2 = (k if v is None else v for v in rows)
        for name, v in (("n1", n1), ("n2", n2)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= k:
                raise ValueError(f"{name} must be an int in [1, {k}], got {v!r}")
        n1, n2 = int(n1), int(n2)
    else:
        matches, count = listed
        if not isinstance(matches, torch.Tensor) or matches.dim() != 3 or matches.shape[2] != 2 or int(matches.shape[0]) != n_pairs or \
                not 1 <= int(matches.shape[1]) <= k:
            raise ValueError(f"matches must be a tensor of shape ({n_pairs}, n1 in [1, {k}], 2)")
        n1, n2 = int(matches.shape[1]), None
        if count is None:
            raise ValueError("count is required")
        _check_arrays((n_pairs, n1, 2), ("matches", matches, torch.int64))
        _check_arrays((n_pairs,), ("count", count, torch.int32))
    doubles = (check_threshold(threshold),)
    if depth is not None:
        fx, fy, cx, cy, ds, vw, vh = check_camera(depth[1])
        doubles = (fx, fy, cx, cy, ds, check_positive("scale_x", depth[2]), check_positive("scale_y", depth[3]), vw, vh) + doubles
    if k > EVAL_MAX_K:
        raise SslamHipError(f"{what}: {k} keypoints per frame; at most {EVAL_MAX_K} are handled on the device")
    return n_bank, k, n_pairs, n1, n2, tuple(C.c_double(v) for v in doubles)


def _check_pose_rows(name, t, n_pairs, cols):
    """t: a pair's homography or [R | t] per row - a contiguous float64 tensor (n_pairs, cols) or (n_pairs, 3, cols / 3)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous() or \
            tuple(t.shape) not in ((n_pairs, cols), (n_pairs, 3, cols // 3)):
        raise ValueError(f"{name} must be a contiguous float64 tensor of shape ({n_pairs}, {cols}) or ({n_pairs}, 3, {cols // 3})")


def pose_nn_pairs(kp_bank, first, second, H=None, threshold=3.0, n1=None, n2=None, out=None):
    """sslam_pose_nn_pairs: kp_bank (n_bank, K, 2) fp32 pixel keypoints; first / second: 1-D int32 DEVICE lists naming each pair's
    two frames (-1 = absent pair); H (n_pairs, 9) or (n_pairs, 3, 3) float64 device tensor of homographies first -> second, or None
    for the raw coordinates.  n1 / n2: the rows of the first / second frame that count (K by default).
    Returns (gt_matches (P, n1, 2) int64, gt_count (P,) int32, gt_of_row (P, n1) int32, dist_sum (P,) float64, dist_median (P,)
    float64) - include/sslam_hip.h states them; out: optional tensors of those shapes to write into.  One launch, no host read."""
    n_bank, k, n_pairs, n1, n2, (t,) = _pose_operands("pose_nn_pairs", kp_bank, first, second, threshold, rows=(n1, n2))
    if H is not None:
        _check_pose_rows("H", H, n_pairs, 9)
    shapes = pose_score_shapes(n_pairs, n1)
    o = None if out is None else _outputs(shapes, POSE_SCORE_KEYS, out)
    dev = common_device(kp_bank, first, second, H)
    o = _outputs(shapes, POSE_SCORE_KEYS, None, dev) if o is None else o
    _run("pose_nn_pairs", lib().sslam_pose_nn_pairs, (kp_bank, first, second, H, *o),
         _dp(kp_bank), n_bank, k, n1, n2, _dp(first), _dp(second), n_pairs, _dp(H), t, *(_dp(x) for x in o))
    return tuple(o)


def _match_score(what, entry, keys, matches, value, count, gt_of_row, gt_count, out):
    """match_score_pairs and match_score_known_pairs: the entry and its output keys apart, one call."""
    if not isinstance(matches, torch.Tensor) or matches.dim() != 3 or matches.shape[2] != 2 or matches.shape[0] < 1 or matches.shape[1] < 1:
        raise ValueError("matches must be a tensor of shape (n_pairs >= 1, n1 >= 1, 2)")
    n_pairs, n1 = int(matches.shape[0]), int(matches.shape[1])
    for name, t in (("value", value), ("count", count), ("gt_of_row", gt_of_row), ("gt_count", gt_count)):
        if t is None:
            raise ValueError(f"{name} is required")
    _check_arrays((n_pairs, n1, 2), ("matches", matches, torch.int64))
    _check_arrays((n_pairs, n1), ("value", value, torch.float32), ("gt_of_row", gt_of_row, torch.int32))
    _check_arrays((n_pairs,), ("count", count, torch.int32), ("gt_count", gt_count, torch.int32))
    if n1 > EVAL_MAX_K:
        raise SslamHipError(f"{what}: lists of {n1} rows; at most {EVAL_MAX_K} are scored on the device")
    shapes = pose_depth_score_shapes(n_pairs, n1)
    o = None if out is None else _outputs(shapes, keys, out)
    dev = common_device(matches, value, count, gt_of_row, gt_count)
    o = _outputs(shapes, keys, None, dev) if o is None else o
    _run(what, getattr(lib(), entry), (matches, value, count, gt_of_row, gt_count, *o),
         _dp(matches), _dp(value), _dp(count), _dp(gt_of_row), _dp(gt_count), n1, n_pairs, *(_dp(x) for x in o))
    return tuple(o)


def match_score_pairs(matches, value, count, gt_of_row, gt_count, out=None):
    """sslam_match_score_pairs: a match list (matches (P, n1, 2) int64, value (P, n1) fp32, count (P,) int32, as a finalize entry
    wrote it; idx1 unique within a pair) against gt_of_row (P, n1) / gt_count (P,) of pose_nn_pairs over the same pairs.
    Returns (tp, fp, fn (P,) int32, value_sum (P,) float64); out: optional tensors of those shapes.  One launch, no host read."""
    return _match_score("match_score_pairs", "sslam_match_score_pairs", MATCH_SCORE_KEYS, matches, value, count, gt_of_row, gt_count, out)


# ------------------------------------------------------------------------------- pose-based scoring with depth (evaluate.hip)
POSE_DEPTH_SCORE_KEYS = ("gt_matches", "gt_count", "gt_of_row", "valid_count", "dist_sum", "dist_median")
MATCH_KNOWN_SCORE_KEYS = ("tp", "fp", "fn", "unknown", "value_sum")
CAMERA_FIELDS = ("fx", "fy", "cx", "cy", "depth_scale", "width", "height")


def pose_depth_score_shapes(n_pairs: int, n1: int) -> dict:
    """pose_score_shapes plus the two outputs the depth entries add: valid_count and unknown, (n_pairs,) int32."""
    return dict(pose_score_shapes(n_pairs, n1), valid_count=((n_pairs,), torch.int32), unknown=((n_pairs,), torch.int32))


def check_positive(name: str, v) -> float:
    """v as a float: a finite number > 0, else ValueError - before any device work."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not (np.isfinite(float(v)) and float(v) > 0.0):
        raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    return float(v)


def check_camera(camera) -> tuple:
    """(fx, fy, cx, cy, depth_scale, width, height) as floats from an object with those attributes (evaluation.Camera): cx and cy
    finite, the others finite and positive, else ValueError."""
    if any(not hasattr(camera, f) for f in CAMERA_FIELDS):
        raise ValueError(f"camera must have the attributes {', '.join(CAMERA_FIELDS)} (evaluation.Camera), got {camera!r}")
    out = []
    for f in CAMERA_FIELDS:
        v = getattr(camera, f)
        if f in ("cx", "cy"):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(float(v)):
                raise ValueError(f"camera {f} must be a finite number, got {v!r}")
            out.append(float(v))
        else:
            out.append(check_positive(f"camera {f}", v))
    return tuple(out)


def keypoint_depth(depth, kp_pixel, scale_x=1.0, scale_y=1.0, out=None):
    """sslam_keypoint_depth: depth (n, h, w) uint16 raw depth images, kp_pixel (n, K, 2) fp32; scale_x / scale_y take keypoint
    units to depth pixels.  Returns kp_depth (n, K) int32: the raw value under each keypoint (nearest pixel), -1 outside the image
    or for a NaN coordinate; a raw 0 (no measurement) stays 0.  out: an optional tensor of that shape.  One launch, no host read."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.uint16 or depth.dim() != 3 or not depth.is_contiguous() or \
            min(depth.shape) < 1:
        raise ValueError("depth must be a contiguous uint16 tensor of shape (n, h, w)")
    n, h, w = (int(v) for v in depth.shape)
    if not isinstance(kp_pixel, torch.Tensor) or kp_pixel.dim() != 3 or int(kp_pixel.shape[1]) < 1:
        raise ValueError(f"kp_pixel must be a contiguous fp32 tensor of shape ({n}, K, 2)")
    k = int(kp_pixel.shape[1])
    _check_arrays((n, k, 2), ("kp_pixel", kp_pixel, torch.float32))
    sx, sy = check_positive("scale_x", scale_x), check_positive("scale_y", scale_y)
    _check_arrays((n, k), ("out `kp_depth`", out, torch.int32))
    dev = common_device(depth, kp_pixel, out)
    if out is None:
        out = torch.empty((n, k), dtype=torch.int32, device=dev)
    _run("keypoint_depth", lib().sslam_keypoint_depth, (depth, kp_pixel, out), _dp(depth), n, h, w, _dp(kp_pixel), k, C.c_double(sx),
         C.c_double(sy), _dp(out))
    return out


def pose_depth_nn_pairs(kp_bank, kp_depth_bank, first, second, T, camera, scale_x=1.0, scale_y=1.0, threshold=3.0, n1=None, n2=None,
                        out=None):
    """sslam_pose_depth_nn_pairs: kp_bank (n_bank, K, 2) fp32 and kp_depth_bank (n_bank, K) int32 (keypoint_depth's output for the
    same bank); first / second as pose_nn_pairs takes them; T (n_pairs, 12) or (n_pairs, 3, 4) float64 device tensor, [R | t] from
    camera first to camera second in metres; camera: an evaluation.Camera (fx, fy, cx, cy, depth_scale and the view width x height
    in depth pixels); scale_x / scale_y: keypoint units to depth pixels.
    Returns (gt_matches, gt_count, gt_of_row, valid_count, dist_sum, dist_median) - POSE_DEPTH_SCORE_KEYS; gt_of_row is -2 in a row
    without ground truth (include/sslam_hip.h).  out: optional tensors of those shapes.  One launch, no host read."""
    n_bank, k, n_pairs, n1, n2, doubles = _pose_operands("pose_depth_nn_pairs", kp_bank, first, second, threshold,
                                                         depth=(kp_depth_bank, camera, scale_x, scale_y), rows=(n1, n2))
    _check_pose_rows("T", T, n_pairs, 12)
    shapes = pose_depth_score_shapes(n_pairs, n1)
    o = None if out is None else _outputs(shapes, POSE_DEPTH_SCORE_KEYS, out)
    dev = common_device(kp_bank, kp_depth_bank, first, second, T)
    o = _outputs(shapes, POSE_DEPTH_SCORE_KEYS, None, dev) if o is None else o
    _run("pose_depth_nn_pairs", lib().sslam_pose_depth_nn_pairs, (kp_bank, kp_depth_bank, first, second, T, *o),
         _dp(kp_bank), _dp(kp_depth_bank), n_bank, k, n1, n2, _dp(first), _dp(second), n_pairs, _dp(T), *doubles, *(_dp(x) for x in o))
    return tuple(o)


def match_score_known_pairs(matches, value, count, gt_of_row, gt_count, out=None):
    """sslam_match_score_known_pairs: match_score_pairs against a gt_of_row that may hold -2 (pose_depth_nn_pairs).
    Returns (tp, fp, fn, unknown (P,) int32, value_sum (P,) float64) - MATCH_KNOWN_SCORE_KEYS: unknown counts the listed rows whose
    query has no ground truth, fp = count - tp - unknown.  out: optional tensors of those shapes.  One launch, no host read."""
    return _match_score("match_score_known_pairs", "sslam_match_score_known_pairs", MATCH_KNOWN_SCORE_KEYS, matches, value, count,
                        gt_of_row, gt_count, out)


# ------------------------------------------------------------------------------- relative pose from matches and depth (pose_estimate.hip)
POSE_MAX_HYP = 1024     # SSLAM_POSE_MAX_HYP
POSE_RANSAC_KEYS = ("T", "inlier_count", "usable_count", "best_hypothesis", "refit_kept", "inlier_of_slot", "rms")


def pose_ransac_shapes(n_pairs: int, n1: int) -> dict:
    """name -> (shape, dtype) of the outputs of pose_ransac_pairs for n_pairs pairs with lists of n1 slots."""
    one = ((n_pairs,), torch.int32)
    return {"T": ((n_pairs, 12), torch.float64), "inlier_count": one, "usable_count": one, "best_hypothesis": one, "refit_kept": one,
            "inlier_of_slot": ((n_pairs, n1), torch.int32), "rms": ((n_pairs,), torch.float64)}


def check_hypotheses(hypotheses) -> int:
    """The number of RANSAC hypotheses: an int in 1 .. POSE_MAX_HYP, else ValueError - before any device work."""
    if isinstance(hypotheses, bool) or not isinstance(hypotheses, (int, np.integer)) or not 1 <= int(hypotheses) <= POSE_MAX_HYP:
        raise ValueError(f"hypotheses must be an int in [1, {POSE_MAX_HYP}], got {hypotheses!r}")
    return int(hypotheses)


def check_seed(seed) -> int:
    """The sampler's seed: an int in [0, 2^64), else ValueError."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
    return int(seed)


def pose_ransac_pairs(kp_bank, kp_depth_bank, first, second, matches, count, camera, scale_x=1.0, scale_y=1.0, threshold=3.0,
                      hypotheses=256, seed=0, out=None):
    """sslam_pose_ransac_pairs: kp_bank (n_bank, K, 2) fp32 and kp_depth_bank (n_bank, K) int32 (keypoint_depth's output for the same
    bank); first / second as pose_nn_pairs takes them; matches (P, n1, 2) int64 and count (P,) int32: the lists a matcher or
    match_rank wrote for the same pairs; camera: an evaluation.Camera; scale_x / scale_y: keypoint units to depth pixels;
    threshold in keypoint units; hypotheses in 1 .. POSE_MAX_HYP; seed: the sampler's 64-bit seed.
    Returns (T (P, 12) float64 [R | t] camera first -> camera second, inlier_count, usable_count, best_hypothesis, refit_kept (P,)
    int32, inlier_of_slot (P, n1) int32, rms (P,) float64) - POSE_RANSAC_KEYS, include/sslam_hip.h states them.  out: optional
    tensors of those shapes.  One launch, no host read."""
    n_bank, k, n_pairs, n1, _, doubles = _pose_operands("pose_ransac_pairs", kp_bank, first, second, threshold,
                                                        depth=(kp_depth_bank, camera, scale_x, scale_y), listed=(matches, count))
    n_hyp, seed = check_hypotheses(hypotheses), check_seed(seed)
    shapes = pose_ransac_shapes(n_pairs, n1)
    o = None if out is None else _outputs(shapes, POSE_RANSAC_KEYS, out)
    dev = common_device(kp_bank, kp_depth_bank, first, second, matches, count)
    o = _outputs(shapes, POSE_RANSAC_KEYS, None, dev) if o is None else o
    _run("pose_ransac_pairs", lib().sslam_pose_ransac_pairs, (kp_bank, kp_depth_bank, first, second, matches, count, *o),
         _dp(kp_bank), _dp(kp_depth_bank), n_bank, k, _dp(first), _dp(second), n_pairs, _dp(matches), _dp(count), n1, *doubles, n_hyp,
         C.c_uint64(seed), *(_dp(x) for x in o))
    return tuple(o)


# ------------------------------------------------------------------------------- pose refinement on the reprojection error (pose_refine.hip)
REFINE_MAX_ITER = 16    # SSLAM_REFINE_MAX_ITER
POSE_REFINE_KEYS = ("T", "status", "iterations", "selected_count", "usable_count", "inlier_count_in", "inlier_count", "inlier_of_slot",
                    "cost_in", "cost", "rms", "info")
# status: refined and returned / no step accepted / steps accepted but fewer inliers, not kept / not attempted
REFINE_OK, REFINE_NO_STEP, REFINE_NOT_KEPT, REFINE_NOT_ATTEMPTED = 0, 1, 2, 3


def pose_refine_shapes(n_pairs: int, n1: int) -> dict:
    """name -> (shape, dtype) of the outputs of pose_refine_pairs for n_pairs pairs with lists of n1 slots."""
    one, real = ((n_pairs,), torch.int32), ((n_pairs,), torch.float64)
    return {"T": ((n_pairs, 12), torch.float64), "status": one, "iterations": one, "selected_count": one, "usable_count": one,
            "inlier_count_in": one, "inlier_count": one, "inlier_of_slot": ((n_pairs, n1), torch.int32), "cost_in": real, "cost": real,
            "rms": real, "info": ((n_pairs, 21), torch.float64)}


def check_huber(huber) -> float:
    """The Huber delta of the refinement, in keypoint units: a finite number > 0, else ValueError - before any device work."""
    return check_positive("huber", huber)


def check_iterations(iterations) -> int:
    """The most Gauss-Newton steps: an int in 0 .. REFINE_MAX_ITER, else ValueError - before any device work."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= REFINE_MAX_ITER:
        raise ValueError(f"iterations must be an int in [0, {REFINE_MAX_ITER}], got {iterations!r}")
    return int(iterations)


def pose_refine_pairs(kp_bank, kp_depth_bank, first, second, matches, count, camera, T_in, scale_x=1.0, scale_y=1.0, threshold=3.0,
                      huber=1.0, iterations=5, out=None):
    """sslam_pose_refine_pairs: kp_bank .. camera, scale_x / scale_y and threshold as pose_ransac_pairs takes them; T_in (P, 12) or
    (P, 3, 4) float64 device tensor, the initial [R | t] of every pair (camera first -> camera second); huber: the Huber delta in
    keypoint units; iterations: the most Gauss-Newton steps, 0 .. REFINE_MAX_ITER.
    Returns (T (P, 12) float64, status, iterations, selected_count, usable_count, inlier_count_in, inlier_count (P,) int32,
    inlier_of_slot (P, n1) int32, cost_in, cost, rms (P,) float64, info (P, 21) float64: the upper triangle of the 6 x 6
    information matrix, row-major) - POSE_REFINE_KEYS, include/sslam_hip.h states them.  out: optional tensors of those shapes
    (T must not be T_in).  One launch, no host read."""
    n_bank, k, n_pairs, n1, _, doubles = _pose_operands("pose_refine_pairs", kp_bank, first, second, threshold,
                                                        depth=(kp_depth_bank, camera, scale_x, scale_y), listed=(matches, count))
    hub, n_iter = check_huber(huber), check_iterations(iterations)
    _check_pose_rows("T_in", T_in, n_pairs, 12)
    shapes = pose_refine_shapes(n_pairs, n1)
    o = None if out is None else _outputs(shapes, POSE_REFINE_KEYS, out)
    if o is not None and o[0].data_ptr() == T_in.data_ptr():
        raise ValueError("out `T` must not be T_in")
    dev = common_device(kp_bank, kp_depth_bank, first, second, matches, count, T_in)
    o = _outputs(shapes, POSE_REFINE_KEYS, None, dev) if o is None else o
    _run("pose_refine_pairs", lib().sslam_pose_refine_pairs, (kp_bank, kp_depth_bank, first, second, matches, count, T_in, *o),
         _dp(kp_bank), _dp(kp_depth_bank), n_bank, k, _dp(first), _dp(second), n_pairs, _dp(matches), _dp(count), n1, *doubles,
         _dp(T_in), C.c_double(hub), n_iter, *(_dp(x) for x in o))
    return tuple(o)


# ------------------------------------------------------------------------------------------------ validation stage
# slots of a sslam_val_frame_stats / sslam_val_pair_stats row (include/sslam_hip.h)
VAL_FRAME_STATS, VAL_PAIR_STATS = 12, 4
VAL_FRAME_SLOTS = dict(sal_mean=0, sal_var=1, sal_max=2, sal_dx=3, sal_dy=4, sal_high=5, sal_ss=6, edge_a=7, edge_e=8, edge_mean=9,
                       edge_max=10)
VAL_PAIR_SLOTS = dict(repeat=0, ce_sum=1, pad_ce=2, matches=3)


def check_temperature(temperature) -> float:
    """The InfoNCE temperature as the fp32 value the kernels divide by: a finite number above zero, else ValueError."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.floating, np.integer)):
        raise ValueError(f"temperature must be a number, got {temperature!r}")
    t = float(np.float32(temperature))
    if not (t > 0.0 and np.isfinite(t)):
        raise ValueError(f"temperature must be finite and positive, got {temperature!r}")
    return t


def _lse_out(n_pairs, n1, dev, out=None):
    f32 = dict(dtype=torch.float32, device=dev)
    if out is None:
        return torch.empty((n_pairs, n1), **f32), torch.empty((n_pairs, n1), **f32), torch.empty((n_pairs,), **f32)
    lse, ce, s00 = out
    _check_arrays((n_pairs, n1), ("out `lse`", lse, torch.float32), ("out `ce`", ce, torch.float32))
    _check_arrays((n_pairs,), ("out `s00`", s00, torch.float32))
    return lse, ce, s00


def row_lse(d1, stride1, n1, d2, stride2, n2, n_pairs, s12, temperature=0.1, out=None):
    """sslam_row_lse: (lse, ce, s00) of the rows of frame p of d1 against frame p of d2; s12 (n_pairs, n1): the row maxima that
    sim_argmax / sim_argmax_rows wrote for the same pairs.  out: optional (lse, ce, s00) to write into; an entry given as None
    is not computed (the entry's NULL; lse and ce not both: ValueError) and comes back as None."""
    t = check_temperature(temperature)
    _check_arrays((n_pairs, n1), ("s12", s12, torch.float32))
    lse, ce, s00 = _lse_out(n_pairs, n1, d1.device, out)
    d = _operand_width(("d1", d1), ("d2", d2))
    _run("row_lse", lib().sslam_row_lse_d, (d1, d2, s12, lse, ce, s00),
         C.c_void_p(d1.data_ptr()), stride1, n1, C.c_void_p(d2.data_ptr()), stride2, n2, n_pairs, _dp(s12), C.c_float(t), _dp(lse),
         _dp(ce), _dp(s00), d)
    return lse, ce, s00


def row_lse_pairs(bank, first, second, s12, temperature=0.1, out=None):
    """sslam_row_lse_pairs: row_lse for the listed pairs of bank (n_bank, K, 128 | 256); lists as sim_argmax_pairs takes them;
    out as row_lse takes it."""
    t = check_temperature(temperature)
    _check_bank("bank", bank, ("K", WIDTHS))
    n_bank, k = int(bank.shape[0]), int(bank.shape[1])
    n_pairs = check_pair_lists(first, second, bank.device)
    _check_arrays((n_pairs, k), ("s12", s12, torch.float32))
    lse, ce, s00 = _lse_out(n_pairs, k, bank.device, out)
    d = int(bank.shape[2])
    _run("row_lse_pairs", lib().sslam_row_lse_pairs_d, (bank, first, second, s12, lse, ce, s00),
         _dp(bank), k * d, n_bank, k, _dp(first), _dp(second), n_pairs, _dp(s12), C.c_float(t), _dp(lse), _dp(ce), _dp(s00), d)
    return lse, ce, s00


def edge_pool(images_chw, out=None):
    """sslam_edge_pool: fp32 (n, 3, S, S) -> (pooled (n, S/16, S/16), edge_max (n,)).  out: optional tensors to write into."""
    if (not isinstance(images_chw, torch.Tensor) or images_chw.dtype != torch.float32 or images_chw.dim() != 4 or images_chw.shape[1] != 3
            or images_chw.shape[2] != images_chw.shape[3] or images_chw.shape[2] % 16 or not images_chw.is_contiguous()):
        raise ValueError("images must be a contiguous fp32 tensor of shape (n, 3, S, S) with S a multiple of 16")
    n, s = int(images_chw.shape[0]), int(images_chw.shape[2])
    g = s // 16
    if out is None:
        out = (torch.empty((n, g, g), dtype=torch.float32, device=images_chw.device),
               torch.empty((n,), dtype=torch.float32, device=images_chw.device))
    pooled, emax = out
    _check_arrays((n, g, g), ("out `pooled`", pooled, torch.float32))
    _check_arrays((n,), ("out `edge_max`", emax, torch.float32))
    _run("edge_pool", lib().sslam_edge_pool, (images_chw, pooled, emax), _dp(images_chw), n, s, _dp(pooled), _dp(emax))
    return pooled, emax


def val_frame_stats(saliency, pooled=None, edge_max=None, descriptors=None):
    """sslam_val_frame_stats: saliency (n, G, G) [+ pooled, edge_max of edge_pool] [+ descriptors (n, K, d), d = 128 | 256] ->
    (stats (n, VAL_FRAME_STATS), desc_mean (n, d) or None, desc_m2 (n, d) or None)."""
    if not isinstance(saliency, torch.Tensor) or saliency.dim() != 3 or saliency.shape[1] != saliency.shape[2]:
        raise ValueError("saliency must be a tensor of shape (n, G, G)")
    n, g = int(saliency.shape[0]), int(saliency.shape[1])
    _check_arrays((n, g, g), ("saliency", saliency, torch.float32), ("pooled", pooled, torch.float32))
    _check_arrays((n,), ("edge_max", edge_max, torch.float32))
    if (pooled is None) != (edge_max is None):
        raise ValueError("pooled and edge_max come together")
    dev, k, dm, d2, width = saliency.device, 0, None, None, D_OUT
    if descriptors is not None:
        _check_bank("descriptors", descriptors, ("K", WIDTHS))
        if descriptors.shape[0] != n:
            raise ValueError(f"descriptors hold {descriptors.shape[0]} frames, saliency {n}")
        k = int(descriptors.shape[1])
        width = int(descriptors.shape[2])
        dm, d2 = (torch.empty((n, width), dtype=torch.float32, device=dev) for _ in range(2))
    stats = torch.empty((n, VAL_FRAME_STATS), dtype=torch.float32, device=dev)
    _run("val_frame_stats", lib().sslam_val_frame_stats_d, (saliency, pooled, edge_max, descriptors, stats),
         _dp(saliency), _dp(pooled), _dp(edge_max), _dp(descriptors), n, g, k, _dp(stats), _dp(dm), _dp(d2), width)
    return stats, dm, d2


def _pair_stats_arrays(n_pairs, n1, n2, nn12, nn21, s12, ce, s00):
    for name, t in (("nn12", nn12), ("nn21", nn21), ("s12", s12), ("ce", ce), ("s00", s00)):
        if t is None:
            raise ValueError(f"{name} is required")
    _check_arrays((n_pairs, n1), ("nn12", nn12, torch.int32), ("s12", s12, torch.float32), ("ce", ce, torch.float32))
    _check_arrays((n_pairs, n2), ("nn21", nn21, torch.int32))
    _check_arrays((n_pairs,), ("s00", s00, torch.float32))


def val_pair_stats(sal1, sal2, nn12, nn21, s12, ce, s00, temperature=0.1):
    """sslam_val_pair_stats: pair p = frame p of sal1 and of sal2 (n_pairs, G, G each; row slices of one saliency tensor do).
    Returns (stats (n_pairs, VAL_PAIR_STATS), n_matches (n_pairs,) int32)."""
    t = check_temperature(temperature)
    if not isinstance(sal1, torch.Tensor) or sal1.dim() != 3 or sal1.shape[1] != sal1.shape[2]:
        raise ValueError("saliency must be a tensor of shape (n_pairs, G, G)")
    n_pairs, g = int(sal1.shape[0]), int(sal1.shape[1])
    _check_arrays((n_pairs, g, g), ("saliency1", sal1, torch.float32), ("saliency2", sal2, torch.float32))
    if not isinstance(nn12, torch.Tensor) or not isinstance(nn21, torch.Tensor) or nn12.dim() != 2 or nn21.dim() != 2:
        raise ValueError("nn12 (n_pairs, n1) and nn21 (n_pairs, n2) tensors expected")
    n1, n2 = int(nn12.shape[1]), int(nn21.shape[1])
    _pair_stats_arrays(n_pairs, n1, n2, nn12, nn21, s12, ce, s00)
    stats = torch.empty((n_pairs, VAL_PAIR_STATS), dtype=torch.float32, device=sal1.device)
    cnt = torch.empty((n_pairs,), dtype=torch.int32, device=sal1.device)
    _run("val_pair_stats", lib().sslam_val_pair_stats, (sal1, sal2, nn12, nn21, s12, ce, s00, stats, cnt),
         _dp(sal1), _dp(sal2), g, _dp(nn12), _dp(nn21), _dp(s12), _dp(ce), _dp(s00), n1, n2, n_pairs, C.c_float(t), _dp(stats), _dp(cnt))
    return stats, cnt


def val_pair_stats_pairs(saliency, first, second, nn12, nn21, s12, ce, s00, temperature=0.1):
    """sslam_val_pair_stats_pairs: the listed pairs of the bank saliency (n_bank, G, G)."""
    t = check_temperature(temperature)
    if not isinstance(saliency, torch.Tensor) or saliency.dim() != 3 or saliency.shape[1] != saliency.shape[2]:
        raise ValueError("saliency must be a tensor of shape (n_bank, G, G)")
    n_bank, g = int(saliency.shape[0]), int(saliency.shape[1])
    _check_arrays((n_bank, g, g), ("saliency", saliency, torch.float32))
    n_pairs = check_pair_lists(first, second, saliency.device)
    if not isinstance(nn12, torch.Tensor) or nn12.dim() != 2:
        raise ValueError("nn12 (n_pairs, K) tensor expected")
    k = int(nn12.shape[1])
    _pair_stats_arrays(n_pairs, k, k, nn12, nn21, s12, ce, s00)
    stats = torch.empty((n_pairs, VAL_PAIR_STATS), dtype=torch.float32, device=saliency.device)
    cnt = torch.empty((n_pairs,), dtype=torch.int32, device=saliency.device)
    _run("val_pair_stats_pairs", lib().sslam_val_pair_stats_pairs, (saliency, first, second, nn12, nn21, s12, ce, s00, stats, cnt),
         _dp(saliency), g, n_bank, _dp(first), _dp(second), _dp(nn12), _dp(nn21), _dp(s12), _dp(ce), _dp(s00), k, n_pairs,
         C.c_float(t), _dp(stats), _dp(cnt))
    return stats, cnt


def pack_vit_linear(w: np.ndarray) -> np.ndarray:
    """(n_out, k_in) fp32 nn.Linear weight -> uint16 array of bf16 bit patterns in the ViT GEMM's streaming order."""
    w = np.ascontiguousarray(w, np.float32)
    out = np.empty(w.size, np.uint16)
    _check(lib().sslam_vit_pack_linear_host(w.ctypes.data, w.shape[0], w.shape[1], out.ctypes.data), "vit_pack_linear")
    return out


def pack_vit_mlp(w_up: np.ndarray, w_down: np.ndarray, row_scale: np.ndarray | None) -> np.ndarray:
    """(1536, 384) up_proj + (384, 1536) down_proj [+ per-row scale of down_proj] -> the fused MLP kernel's weight stream."""
    w_up, w_down = np.ascontiguousarray(w_up, np.float32), np.ascontiguousarray(w_down, np.float32)
    assert w_up.shape == (1536, 384) and w_down.shape == (384, 1536)
    rs = None if row_scale is None else np.ascontiguousarray(row_scale, np.float32)
    out = np.empty(2 * 1536 * 384, np.uint16)
    _check(lib().sslam_vit_pack_mlp_host(w_up.ctypes.data, w_down.ctypes.data, None if rs is None else rs.ctypes.data, out.ctypes.data),
           "vit_pack_mlp")
    return out


# launch forms of the bf16 ViT that a caller can name (include/sslam_hip.h)
VIT_FORM_THROUGHPUT, VIT_FORM_SMALL, VIT_FORM_FEW_FRAME, VIT_FEW_FRAME_MAX_FRAMES = 0, 1, 2, 8


def vit_workspace_bytes(n_frames: int, size: int, form: int | None = None) -> int:
    """Workspace of one bf16 ViT launch.  form None: the unnamed entries' need; VIT_FORM_*: the named form's own (FEW_FRAME adds
    the attention partials).  ValueError for an unknown form and for FEW_FRAME with more than VIT_FEW_FRAME_MAX_FRAMES frames."""
    if form is None:
        b = int(lib().sslam_vit_workspace_bytes(n_frames, size))
    else:
        b = int(lib().sslam_vit_workspace_bytes_form(n_frames, size, int(form)))
    if b < 0:
        _check(b, "vit_workspace_bytes")
    return b


def _with_form(fn, form):
    """The *_form entries take `form` before the trailing stream argument.  The call keeps the entry's name (what a test that
    watches _run sees)."""
    def call(*a):
        return fn(*a[:-1], int(form), a[-1])
    call.__name__ = fn.__name__
    return call


def vit_forward_patches(patches, size: int, weights: VitWeights, workspace, out=None, form: int | None = None):
    """patches (n, (size/16)^2, 768) bf16 from preprocess_u8_patches -> tokens (n, 5 + (size/16)^2, 384) fp32.
    form: None - the library's rule by this launch's token rows; VIT_FORM_* - the caller's (sslam_vit_forward_patches_form)."""
    n = patches.shape[0]
    t = 5 + (size // 16) ** 2
    if out is None:
        out = torch.empty((n, t, C_FEAT), dtype=torch.float32, device=patches.device)
    fn = lib().sslam_vit_forward_patches if form is None else _with_form(lib().sslam_vit_forward_patches_form, form)
    _run("vit_forward_patches", fn, (patches, workspace, out,),
         _dp(patches), n, size, C.byref(weights), _dp(workspace), workspace.numel() * workspace.element_size(), _dp(out))
    return out


def vit_forward(images_chw, weights: VitWeights, workspace, out=None, form: int | None = None):
    """form: None - the library's rule by this launch's token rows; VIT_FORM_* - the caller's (sslam_vit_forward_form)."""
    n, _, size, _ = images_chw.shape
    t = 5 + (size // 16) ** 2
    if out is None:
        out = torch.empty((n, t, C_FEAT), dtype=torch.float32, device=images_chw.device)
    fn = lib().sslam_vit_forward if form is None else _with_form(lib().sslam_vit_forward_form, form)
    _run("vit_forward", fn, (images_chw, workspace, out,),
         _dp(images_chw), n, size, C.byref(weights), _dp(workspace), workspace.numel() * workspace.element_size(),
                                   _dp(out))
    return out


def pack_vit_f32_linear(w: np.ndarray) -> np.ndarray:
    """(n_out, k_in) fp32 nn.Linear weight -> the same values in the fragment order of the fp32 ViT's per-layer GEMM."""
    w = np.ascontiguousarray(w, np.float32)
    out = np.empty(w.size, np.float32)
    _check(lib().sslam_vit_f32_pack_linear_host(w.ctypes.data, w.shape[0], w.shape[1], out.ctypes.data), "vit_f32_pack_linear")
    return out


def vit_f32_workspace_bytes(n_frames: int, size: int) -> int:
    b = int(lib().sslam_vit_f32_workspace_bytes(n_frames, size))
    if b < 0:
        _check(b, "vit_f32_workspace_bytes")
    return b


ATTN_ONE_PASS, ATTN_KEY_SPLIT, ATTN_KEY_SPLIT_MAX_FRAMES = 0, 1, 8          # include/sslam_hip.h


def vit_forward_f32(images_chw, weights: VitWeightsF32, workspace, out=None, attention_form: int | None = None):
    """(n, 3, S, S) fp32 -> tokens (n, 5 + (S/16)^2, 384) fp32 by the fp32-operand HIP ViT (reference numerics for A1).
    attention_form: None - the library's choice by this launch's frame count (key split up to 8 frames); ATTN_ONE_PASS /
    ATTN_KEY_SPLIT - the caller's (a batch cut into several launches passes the form of the whole batch to each)."""
    n, _, size, _ = images_chw.shape
    t = 5 + (size // 16) ** 2
    if out is None:
        out = torch.empty((n, t, C_FEAT), dtype=torch.float32, device=images_chw.device)
    if attention_form is None:
        _run("vit_forward_f32", lib().sslam_vit_forward_f32, (images_chw, workspace, out,),
             _dp(images_chw), n, size, C.byref(weights), _dp(workspace), workspace.numel() * workspace.element_size(), _dp(out))
    else:
        _run("vit_forward_f32_form", _with_form(lib().sslam_vit_forward_f32_form, attention_form), (images_chw, workspace, out,),
             _dp(images_chw), n, size, C.byref(weights), _dp(workspace), workspace.numel() * workspace.element_size(), _dp(out))
    return out


# ------------------------------------------------------------------------------------------ libsslam_ext.so (include/sslam_ext.h)
# Sub-cell keypoint localisation: entries with the prefix sslx_ (row "ext" of LIBRARIES).
EXT_EXPORTS = ["sslx_version", "sslx_arch", "sslx_launch_count", "sslx_subcell_keypoints"]
SUBCELL_MAX_CELLS, SUBCELL_MAX_K = 4096, 4096
FLAG_X, FLAG_Y, FLAG_RANGE = 1, 2, 4           # bits of subcell_keypoints' flags


def _ext_prototypes(L):
    p, i = C.c_void_p, C.c_int
    L.sslx_subcell_keypoints.argtypes = [p, i, i, p, i, p, p, p, p]


def subcell_shapes(n: int, k: int) -> dict:
    """The outputs of subcell_keypoints for n frames of k keypoints: key -> (shape, dtype), in the entry's order."""
    return {"keypoints_subpatch": ((n, k, 2), torch.float32), "keypoints_subpixel": ((n, k, 2), torch.float32),
            "subcell_flags": ((n, k), torch.int32)}


SUBCELL_KEYS = ("keypoints_subpatch", "keypoints_subpixel", "subcell_flags")


def subcell_keypoints(sal, idx, out=None):
    """sslx_subcell_keypoints: sal (n, G, G) fp32 - the saliency the keypoints were selected from - and idx (n, K) int32, the flat
    cells select_keypoints wrote.  Returns (kp_xy_sub (n, K, 2) fp32 in patch units, kp_pixel_sub (n, K, 2) fp32 = kp_xy_sub * 16 + 8,
    flags (n, K) int32: FLAG_X | FLAG_Y where the axis was refined, FLAG_RANGE for an idx outside the grid) - each keypoint at the
    vertex of the per-axis parabola through its cell and the two neighbours (include/sslam_ext.h states every operation).
    out: optional tensors of those shapes to write into.  One launch, no host read; shapes and dtypes are judged first."""
    if not isinstance(sal, torch.Tensor) or sal.dtype != torch.float32 or sal.dim() != 3 or sal.shape[1] != sal.shape[2] or \
            min(sal.shape) < 1 or not sal.is_contiguous():
        raise ValueError("sal must be a contiguous float32 tensor of shape (n, G, G)")
    n, g = int(sal.shape[0]), int(sal.shape[1])
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.dim() != 2 or int(idx.shape[0]) != n or \
            int(idx.shape[1]) < 1 or not idx.is_contiguous():
        raise ValueError(f"idx must be a contiguous int32 tensor of shape ({n}, K)")
    k = int(idx.shape[1])
    if g * g > SUBCELL_MAX_CELLS or k > SUBCELL_MAX_K or n * k > 2 ** 31 - 1:
        raise SslamHipError(f"subcell_keypoints: {_ERR[E_UNSUPPORTED]} (G * G <= {SUBCELL_MAX_CELLS}, K <= {SUBCELL_MAX_K}, "
                            f"n * K < 2^31; got n = {n}, G = {g}, K = {k})")
    shapes = subcell_shapes(n, k)
    if out is not None:
        if len(out) != 3:
            raise ValueError("out must be (kp_xy_sub, kp_pixel_sub, flags)")
        for key, t in zip(SUBCELL_KEYS, out):
            if t is None:
                raise ValueError(f"out `{key}` is required")
            _check_arrays(shapes[key][0], (f"out `{key}`", t, shapes[key][1]))
    dev = common_device(sal, idx, *(out or ()))
    xy, px, fl = out if out is not None else (torch.empty(shapes[key][0], dtype=shapes[key][1], device=dev) for key in SUBCELL_KEYS)
    _run("subcell_keypoints", ext().sslx_subcell_keypoints, (sal, idx, xy, px, fl), _dp(sal), n, g, _dp(idx), k, _dp(xy), _dp(px), _dp(fl))
    return xy, px, fl


# ---------------------------------------------------------------------------------------- libsslam_graph.so (include/sslam_graph.h)
# The banded pose graph: entries with the prefix sslg_ (row "graph" of LIBRARIES).
GRAPH_EXPORTS = ["sslg_version", "sslg_arch", "sslg_launch_count", "sslg_chain_poses", "sslg_pose_graph_workspace_bytes", "sslg_pose_graph"]
GRAPH_MAX_BAND, GRAPH_MAX_NODES, GRAPH_MAX_EDGES, GRAPH_MAX_GRAPHS, GRAPH_MAX_ITER = 32, 4096, 1048576, 65535, 16
GRAPH_MAX_CHAINS = 0x7fffffff // 256      # sslg_chain_poses runs a thread per chain, not a workgroup per graph: its own n_graphs limit
POSE_GRAPH_KEYS = ("C", "status", "iterations", "used_edges", "skipped_edges", "failed_row", "cost_in", "cost", "edge_chi2")
# status: a step was accepted / no step accepted / a failed pivot at the first step / not attempted
GRAPH_OK, GRAPH_NO_STEP, GRAPH_SINGULAR, GRAPH_NOT_ATTEMPTED = 0, 1, 2, 3


def _graph_prototypes(L):
    L.sslg_pose_graph_workspace_bytes.restype = C.c_size_t
    p, i, d = C.c_void_p, C.c_int, C.c_double
    L.sslg_pose_graph_workspace_bytes.argtypes = [i, i, i]
    L.sslg_chain_poses.argtypes = [p, p, i, i, p, p]
    L.sslg_pose_graph.argtypes = [p, p, p, p, i, i, i, p, i, d, d, i] + [p] * 11


def check_band(band) -> int:
    """The most b - a of a used edge: an int >= 1, else ValueError; above GRAPH_MAX_BAND: SslamHipError - before any device work."""
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or int(band) < 1:
        raise ValueError(f"band must be an int >= 1, got {band!r}")
    if int(band) > GRAPH_MAX_BAND:
        raise SslamHipError(f"pose_graph: {_ERR[E_UNSUPPORTED]} (band <= {GRAPH_MAX_BAND}, got {band})")
    return int(band)


def _check_nonnegative(name, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (float(v) >= 0.0) or not np.isfinite(float(v)):
        raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    return float(v)


def check_damping(damping) -> float:
    """What is added to the diagonal of the normal equations: a finite number >= 0, else ValueError - before any device work."""
    return _check_nonnegative("damping", damping)


def check_graph_iterations(iterations) -> int:
    """The most Gauss-Newton steps of the pose graph: an int in 0 .. GRAPH_MAX_ITER, else ValueError - before any device work."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= GRAPH_MAX_ITER:
        raise ValueError(f"iterations must be an int in [0, {GRAPH_MAX_ITER}], got {iterations!r}")
    return int(iterations)


def _graph_rows(name, t, lead, tail, dtype):
    """t: a contiguous tensor of `dtype` shaped lead + tail (a single graph may leave the graph axis out) -> it with the graph axis."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{name} must be a {dtype} tensor")
    if lead is not None and t.dim() == len(lead) + len(tail) - 1 and lead[0] == 1:
        t = t[None]
    want = None if lead is None else tuple(lead) + tuple(tail)
    if (want is not None and tuple(t.shape) != want) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor of shape {want}, got {tuple(t.shape)}")
    return t


def pose_graph_shapes(n_graphs: int, n_nodes: int, n_edges: int) -> dict:
    """name -> (shape, dtype) of the outputs of pose_graph."""
    one, real = ((n_graphs,), torch.int32), ((n_graphs,), torch.float64)
    return {"C": ((n_graphs, n_nodes, 12), torch.float64), "status": one, "iterations": one, "used_edges": one, "skipped_edges": one,
            "failed_row": one, "cost_in": real, "cost": real, "edge_chi2": ((n_graphs, n_edges), torch.float64)}


def pose_graph_workspace_bytes(n_graphs: int, n_nodes: int, band: int) -> int:
    """sslg_pose_graph_workspace_bytes, restated: per graph n * (6 band + 6) + 3 n + 12 n_nodes + 256 * 90 float64 words with
    n = 6 (n_nodes - 1).  Needs no library."""
    n = 6 * (n_nodes - 1)
    return 8 * n_graphs * (n * (6 * band + 6) + 3 * n + 12 * n_nodes + 256 * 90)


def _check_graph_sizes(what, n_graphs, n_nodes, n_edges=1, limits=None):
    """limits: the most (graphs, nodes, edge slots) of the entry; the third library's if not given."""
    max_graphs, max_nodes, max_edges = limits or (GRAPH_MAX_GRAPHS, GRAPH_MAX_NODES, GRAPH_MAX_EDGES)
    if n_graphs < 1 or n_nodes < 1 or n_edges < 1:
        raise ValueError(f"{what}: at least one graph, node and edge slot expected, got {n_graphs}, {n_nodes}, {n_edges}")
    if n_graphs > max_graphs or n_nodes > max_nodes or n_edges > max_edges:
        raise SslamHipError(f"{what}: {_ERR[E_UNSUPPORTED]} (n_graphs <= {max_graphs}, n_nodes <= {max_nodes}, n_edges <= "
                            f"{max_edges}; got {n_graphs}, {n_nodes}, {n_edges})")


def _check_workspace(workspace, need):
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or
                                  workspace.numel() < need or not workspace.is_contiguous()):
        raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {need} bytes")


def _graph_operands(what, first, second, T, info, C_in, limits, shapes_of, keys, out, need_of, workspace):
    """What pose_graph and pose_graph_sparse judge alike, touching no library: the five operands given the graph axis, the sizes
    against `limits`, out against shapes_of(n_graphs, n_nodes, n_edges), the workspace against need_of(the same), one device.
    -> (first, second, T, info, C_in, workspace, *outputs) - outputs and workspace made where not given - and the three sizes."""
    if not isinstance(C_in, torch.Tensor) or C_in.dtype != torch.float64 or C_in.dim() not in (2, 3) or int(C_in.shape[-1]) != 12 or \
            not C_in.is_contiguous():
        raise ValueError("C_in must be a contiguous float64 tensor of shape (n_graphs, n_nodes, 12) or (n_nodes, 12)")
    C3 = C_in[None] if C_in.dim() == 2 else C_in
    n_graphs, n_nodes = int(C3.shape[0]), int(C3.shape[1])
    if not isinstance(first, torch.Tensor) or first.dim() not in (1, 2):
        raise ValueError("first must be an int32 tensor of shape (n_graphs, n_edges) or (n_edges,)")
    n_edges = int(first.shape[-1])
    _check_graph_sizes(what, n_graphs, n_nodes, n_edges, limits)
    lead = (n_graphs, n_edges)
    first = _graph_rows("first", first, lead, (), torch.int32)
    second = _graph_rows("second", second, lead, (), torch.int32)
    T = _graph_rows("T", T, lead, (12,), torch.float64)
    info = _graph_rows("info", info, lead, (21,), torch.float64)
    shapes = shapes_of(n_graphs, n_nodes, n_edges)
    o = None if out is None else _outputs(shapes, keys, out)
    if o is not None and o[0].data_ptr() == C3.data_ptr():
        raise ValueError("out `C` must not be C_in")
    need = need_of(n_graphs, n_nodes, n_edges)
    _check_workspace(workspace, need)
    dev = common_device(first, second, T, info, C3, workspace, *(o or ()))
    o = _outputs(shapes, keys, None, dev) if o is None else o
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    return (first, second, T, info, C3, ws, *o), (n_graphs, n_nodes, n_edges)


def chain_poses(T, n_nodes=None, start=None, out=None):
    """sslg_chain_poses: T (n_graphs, n_nodes - 1, 12) float64 (or (n_nodes - 1, 12) for one chain), the transforms camera i ->
    camera i + 1; start (n_graphs, 12) or None ([I | 0]).  Returns C (n_graphs, n_nodes, 12): C_0 = start, C_{i+1} = T_i o C_i,
    world -> camera.  n_nodes: given to chain only the first n_nodes - 1 rows' worth (T must then be exactly that long).  One launch."""
    if not isinstance(T, torch.Tensor) or T.dtype != torch.float64 or T.dim() not in (2, 3) or int(T.shape[-1]) != 12 or not T.is_contiguous():
        raise ValueError("T must be a contiguous float64 tensor of shape (n_graphs, n_nodes - 1, 12) or (n_nodes - 1, 12)")
    T3 = T[None] if T.dim() == 2 else T
    n_graphs, nn = int(T3.shape[0]), int(T3.shape[1]) + 1
    if n_nodes is not None and int(n_nodes) != nn:
        raise ValueError(f"T holds {nn - 1} transforms, n_nodes = {n_nodes} needs {int(n_nodes) - 1}")
    _check_graph_sizes("chain_poses", n_graphs, nn, limits=(GRAPH_MAX_CHAINS, GRAPH_MAX_NODES, GRAPH_MAX_EDGES))
    if start is not None:
        start = _graph_rows("start", start, (n_graphs,), (12,), torch.float64)
    if out is not None:
        out = _graph_rows("out", out, (n_graphs,), (nn, 12), torch.float64)
    dev = common_device(T3, start, out)
    Cc = torch.empty((n_graphs, nn, 12), dtype=torch.float64, device=dev) if out is None else out
    _run("chain_poses", graph().sslg_chain_poses, (T3, start, Cc), _dp(T3) if nn > 1 else None, _dp(start), n_graphs, nn, _dp(Cc))
    return Cc


def pose_graph(first, second, T, info, C_in, band, huber_chi=4.0, damping=0.0, iterations=8, out=None, workspace=None):
    """sslg_pose_graph: first, second (n_graphs, n_edges) int32 (-1 in first: an absent slot), T (n_graphs, n_edges, 12) and info
    (n_graphs, n_edges, 21) float64 as pose_refine_pairs writes them, C_in (n_graphs, n_nodes, 12) float64 world -> camera (one
    graph may leave the graph axis out of all five).  band: the most b - a of a used edge; huber_chi: finite > 0; damping: finite
    >= 0; iterations 0 .. GRAPH_MAX_ITER.  Returns POSE_GRAPH_KEYS' tensors (include/sslam_graph.h states them), always with the
    graph axis.  out: optional tensors of pose_graph_shapes (C must not be C_in); workspace: optional uint8 tensor of at least
    pose_graph_workspace_bytes.  One launch, no host read; everything is judged before the library is loaded."""
    b, chi, damp, n_iter = check_band(band), check_positive("huber_chi", huber_chi), check_damping(damping), check_graph_iterations(iterations)
    t, (n_graphs, n_nodes, n_edges) = _graph_operands("pose_graph", first, second, T, info, C_in, None, pose_graph_shapes, POSE_GRAPH_KEYS, out,
                                                     lambda g, n, e: pose_graph_workspace_bytes(g, n, b), workspace)
    first, second, T, info, C3, ws, *o = t
    _run("pose_graph", graph().sslg_pose_graph, t, _dp(first), _dp(second), _dp(T), _dp(info),
         n_graphs, n_nodes, n_edges, _dp(C3), b, C.c_double(chi), C.c_double(damp), n_iter, _dp(ws), *(_dp(x) for x in o))
    return tuple(o)


# ------------------------------------------------------------------------------------------ libsslam_loop.so (include/sslam_loop.h)
# Loop closures and the sparse pose graph: entries with the prefix ssll_ (row "loop" of LIBRARIES).
LOOP_EXPORTS = ["ssll_version", "ssll_arch", "ssll_launch_count", "ssll_frame_signatures", "ssll_loop_candidates",
                "ssll_pose_graph_sparse_workspace_bytes", "ssll_pose_graph_sparse"]
LOOP_MAX_FRAMES, LOOP_MAX_K, LOOP_MAX_PER_FRAME = 4096, 4096, 8
SPARSE_MAX_NODES, SPARSE_MAX_EDGES, SPARSE_MAX_GRAPHS, SPARSE_MAX_ITER, SPARSE_MAX_CG = 4096, 65536, 65535, 16, 4096
LOOP_CANDIDATE_KEYS = ("first", "second", "sim", "count")
POSE_GRAPH_SPARSE_KEYS = POSE_GRAPH_KEYS + ("cg_steps",)


def _loop_prototypes(L):
    L.ssll_pose_graph_sparse_workspace_bytes.restype = C.c_size_t
    p, i, d, f = C.c_void_p, C.c_int, C.c_double, C.c_float
    L.ssll_pose_graph_sparse_workspace_bytes.argtypes = [i, i, i]
    L.ssll_frame_signatures.argtypes = [p, p, i, i, i, p, p, p]
    L.ssll_loop_candidates.argtypes = [p, i, i, i, f, i, i, p, p, p, p, p]
    L.ssll_pose_graph_sparse.argtypes = [p, p, p, p, i, i, i, p, d, d, i, i, d] + [p] * 12


def check_int(name, v, lo, hi=None) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(f"{name} must be an int {'>= ' + str(lo) if hi is None else 'in [' + str(lo) + ', ' + str(hi) + ']'}, got {v!r}")
    return int(v)


def check_cg_iterations(cg_iterations) -> int:
    """The most conjugate-gradient iterations of a step: an int >= 1, else ValueError; above SPARSE_MAX_CG: SslamHipError - before any
    device work."""
    n_cg = check_int("cg_iterations", cg_iterations, 1)
    if n_cg > SPARSE_MAX_CG:
        raise SslamHipError(f"pose_graph_sparse: {_ERR[E_UNSUPPORTED]} (cg_iterations <= {SPARSE_MAX_CG}, got {n_cg})")
    return n_cg


def check_cg_tol(cg_tol) -> float:
    """The relative tolerance of the conjugate gradients: a finite number >= 0, else ValueError - before any device work."""
    return _check_nonnegative("cg_tol", cg_tol)


def frame_signatures(descriptors, scores, out=None, workspace=None):
    """ssll_frame_signatures: descriptors (N, K, D) and scores (N, K) float32 as extract() returns them, D in WIDTHS.  Returns sig
    (N, D) float32: the score-weighted descriptor sum of every frame, centred on the sequence's mean and normalised
    (include/sslam_loop.h).  workspace: optional uint8 tensor of at least N * D * 4 bytes.  Two launches, no host read."""
    _check_bank("descriptors", descriptors, ("K", WIDTHS))
    n, k, d = (int(x) for x in descriptors.shape)
    if scores is None:
        raise ValueError("scores is required")
    _check_arrays((n, k), ("scores", scores, torch.float32))
    if n > LOOP_MAX_FRAMES or k > LOOP_MAX_K:
        raise SslamHipError(f"frame_signatures: {_ERR[E_UNSUPPORTED]} (N <= {LOOP_MAX_FRAMES}, K <= {LOOP_MAX_K}; got {n}, {k})")
    if out is not None:
        _check_arrays((n, d), ("out", out, torch.float32))
    need = 4 * n * d
    _check_workspace(workspace, need)
    dev = common_device(descriptors, scores, out, workspace)
    sig = torch.empty((n, d), dtype=torch.float32, device=dev) if out is None else out
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    _run("frame_signatures", loop().ssll_frame_signatures, (descriptors, scores, ws, sig), _dp(descriptors), _dp(scores), n, k, d, _dp(ws),
         _dp(sig))
    return sig


def loop_candidate_shapes(n_frames: int, per_frame: int) -> dict:
    """name -> (shape, dtype) of the outputs of loop_candidates."""
    slots = (n_frames * per_frame,)
    return {"first": (slots, torch.int32), "second": (slots, torch.int32), "sim": (slots, torch.float32), "count": ((n_frames,), torch.int32)}


def check_loop_arguments(min_gap, min_sim, per_frame, suppress) -> tuple:
    """(min_gap >= 1, finite min_sim, per_frame 1 .. LOOP_MAX_PER_FRAME, suppress >= 0), else ValueError - before any device work."""
    gap, per, sup = check_int("min_gap", min_gap, 1), check_int("per_frame", per_frame, 1, LOOP_MAX_PER_FRAME), check_int("suppress", suppress, 0)
    if isinstance(min_sim, bool) or not isinstance(min_sim, (int, float, np.integer, np.floating)) or not np.isfinite(np.float32(min_sim)):
        raise ValueError(f"min_sim must be a finite number, got {min_sim!r}")
    return gap, float(np.float32(min_sim)), per, sup


def loop_candidates(sig, min_gap=30, min_sim=0.3, per_frame=2, suppress=5, out=None):
    """ssll_loop_candidates: sig (N, D) float32 from frame_signatures.  For every frame i up to per_frame older frames j <= i -
    min_gap of similarity >= min_sim (rounded to float32), best first, none within `suppress` frames of a better one.  Returns
    (first, second, sim, count) - LOOP_CANDIDATE_KEYS, loop_candidate_shapes - in match_pairs' pair-list form: first the older
    frame or -1, second = i or -1.  One launch, no host read."""
    gap, sim_min, per, sup = check_loop_arguments(min_gap, min_sim, per_frame, suppress)
    _check_bank("sig", sig, (WIDTHS,))
    n, d = int(sig.shape[0]), int(sig.shape[1])
    if n > LOOP_MAX_FRAMES:
        raise SslamHipError(f"loop_candidates: {_ERR[E_UNSUPPORTED]} (N <= {LOOP_MAX_FRAMES}, got {n})")
    shapes = loop_candidate_shapes(n, per)
    o = None if out is None else _outputs(shapes, LOOP_CANDIDATE_KEYS, out)
    dev = common_device(sig, *(o or ()))
    o = _outputs(shapes, LOOP_CANDIDATE_KEYS, None, dev) if o is None else o
    _run("loop_candidates", loop().ssll_loop_candidates, (sig, *o), _dp(sig), n, d, min(gap, 2 ** 31 - 1), C.c_float(sim_min), per,
         min(sup, 2 ** 31 - 1), *(_dp(x) for x in o))
    return tuple(o)


def pose_graph_sparse_shapes(n_graphs: int, n_nodes: int, n_edges: int) -> dict:
    """name -> (shape, dtype) of the outputs of pose_graph_sparse: pose_graph_shapes and cg_steps."""
    return dict(pose_graph_shapes(n_graphs, n_nodes, n_edges), cg_steps=((n_graphs, SPARSE_MAX_ITER), torch.int32))


def pose_graph_sparse_workspace_bytes(n_graphs: int, n_nodes: int, n_edges: int) -> int:
    """ssll_pose_graph_sparse_workspace_bytes, restated: per graph 90 E + 78 (N - 1) + 12 N + (N + 1 + 2 E + 1) // 2 float64 words.
    Needs no library."""
    return 8 * n_graphs * (90 * n_edges + 78 * (n_nodes - 1) + 12 * n_nodes + (n_nodes + 1 + 2 * n_edges + 1) // 2)


def pose_graph_sparse(first, second, T, info, C_in, huber_chi=4.0, damping=0.0, iterations=8, cg_iterations=512, cg_tol=1e-3, out=None,
                      workspace=None):
    """ssll_pose_graph_sparse: pose_graph's operands without a band - an edge may join any two nodes - and the step solved by
    block-Jacobi preconditioned conjugate gradients: at most cg_iterations (1 .. SPARSE_MAX_CG) per step, stopped at the relative
    tolerance cg_tol (finite >= 0).  Returns POSE_GRAPH_SPARSE_KEYS' tensors (include/sslam_loop.h), always with the graph axis:
    pose_graph's and cg_steps (n_graphs, 16), the CG iterations of every step.  out: optional tensors of pose_graph_sparse_shapes
    (C must not be C_in); workspace: optional uint8 tensor of at least pose_graph_sparse_workspace_bytes.  One launch, no host
    read; everything is judged before the library is loaded."""
    chi, damp, n_iter = check_positive("huber_chi", huber_chi), check_damping(damping), check_graph_iterations(iterations)
    n_cg, tol = check_cg_iterations(cg_iterations), check_cg_tol(cg_tol)
    t, (n_graphs, n_nodes, n_edges) = _graph_operands("pose_graph_sparse", first, second, T, info, C_in,
                                                     (SPARSE_MAX_GRAPHS, SPARSE_MAX_NODES, SPARSE_MAX_EDGES), pose_graph_sparse_shapes,
                                                     POSE_GRAPH_SPARSE_KEYS, out, pose_graph_sparse_workspace_bytes, workspace)
    first, second, T, info, C3, ws, *o = t
    _run("pose_graph_sparse", loop().ssll_pose_graph_sparse, t, _dp(first), _dp(second), _dp(T),
         _dp(info), n_graphs, n_nodes, n_edges, _dp(C3), C.c_double(chi), C.c_double(damp), n_iter, n_cg, C.c_double(tol), _dp(ws),
         *(_dp(x) for x in o))
    return tuple(o)


# -------------------------------------------------------------------------------------- libsslam_window.so (include/sslam_window.h)
# The sliding-window graph of the online stepper: entries with the prefix sslw_ (row "window" of LIBRARIES).
WINDOW_EXPORTS = ["sslw_version", "sslw_arch", "sslw_launch_count", "sslw_window_workspace_bytes", "sslw_window_step"]
WINDOW_MAX_WINDOW, WINDOW_MAX_SPACINGS, WINDOW_MAX_WINDOWS, WINDOW_MAX_FRAME = 32, 8, 65535, 2 ** 31 - 2
WINDOW_STATE_KEYS = ("t", "ring_first", "ring_second", "ring_T", "ring_info", "ring_C", "trajectory")
WINDOW_OUT_KEYS = ("C_window", "base", "n_nodes", "admitted", "predicted_from", "lost", "status", "iterations", "used_edges", "dropped_edges",
                   "failed_row", "cost_in", "cost", "edge_chi2")
WINDOW_COUNTER_OUT_OF_RANGE = 4      # status, beside GRAPH_OK .. GRAPH_NOT_ATTEMPTED


def _window_prototypes(L):
    L.sslw_window_workspace_bytes.restype = C.c_size_t
    p, i, d, ll = C.c_void_p, C.c_int, C.c_double, C.c_longlong
    L.sslw_window_workspace_bytes.argtypes = [i, i, i]
    L.sslw_window_step.argtypes = [p] * 13 + [i, i, i, i, d, d, i, ll] + [p] * 16


def check_window_sizes(window, n_spacings, capacity, n_windows=1) -> tuple:
    """(window 2 .., n_spacings 1 .., capacity 1 .., n_windows 1 ..) as ints, else ValueError; past WINDOW_MAX_*: SslamHipError -
    before any device work."""
    w, s, cap, nw = check_int("window", window, 2), check_int("n_spacings", n_spacings, 1), check_int("capacity", capacity, 1), \
        check_int("n_windows", n_windows, 1)
    if w > WINDOW_MAX_WINDOW or s > WINDOW_MAX_SPACINGS or nw > WINDOW_MAX_WINDOWS or cap > (2 ** 63 - 1) // 96 // nw:
        raise SslamHipError(f"window_step: {_ERR[E_UNSUPPORTED]} (window <= {WINDOW_MAX_WINDOW}, n_spacings <= {WINDOW_MAX_SPACINGS}, "
                            f"n_windows <= {WINDOW_MAX_WINDOWS}, capacity * 96 * n_windows < 2^63; got {w}, {s}, {nw}, {cap})")
    return w, s, cap, nw


def window_state_shapes(n_windows: int, window: int, n_spacings: int, capacity: int) -> dict:
    """name -> (shape, dtype) of the persistent state of window_step (WINDOW_STATE_KEYS)."""
    ws = window * n_spacings
    return {"t": ((n_windows,), torch.int32), "ring_first": ((n_windows, ws), torch.int32), "ring_second": ((n_windows, ws), torch.int32),
            "ring_T": ((n_windows, ws, 12), torch.float64), "ring_info": ((n_windows, ws, 21), torch.float64),
            "ring_C": ((n_windows, window, 12), torch.float64), "trajectory": ((n_windows, capacity, 12), torch.float64)}


def window_out_shapes(n_windows: int, window: int, n_spacings: int) -> dict:
    """name -> (shape, dtype) of the outputs of window_step (WINDOW_OUT_KEYS)."""
    one, real = ((n_windows,), torch.int32), ((n_windows,), torch.float64)
    return {"C_window": ((n_windows, window, 12), torch.float64), "base": one, "n_nodes": one, "admitted": ((n_windows, n_spacings), torch.int32),
            "predicted_from": one, "lost": one, "status": one, "iterations": one, "used_edges": one, "dropped_edges": one, "failed_row": one,
            "cost_in": real, "cost": real, "edge_chi2": ((n_windows, window * n_spacings), torch.float64)}


def window_workspace_bytes(n_windows: int, window: int, n_spacings: int) -> int:
    """sslw_window_workspace_bytes, restated: per window 24 W + 256 * 90 + W S float64 words.  Needs no library."""
    return 8 * n_windows * (24 * window + 256 * 90 + window * n_spacings)


def alloc_window_state(window, n_spacings, capacity, n_windows=1, device="cuda") -> dict:
    """A fresh state of window_step: t = 0, ring_first = -1, everything else zero."""
    w, s, cap, nw = check_window_sizes(window, n_spacings, capacity, n_windows)
    state = {k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in window_state_shapes(nw, w, s, cap).items()}
    state["ring_first"].fill_(-1)
    return state


def alloc_window_out(window, n_spacings, n_windows=1, device="cuda") -> dict:
    """The outputs of window_step as zeroed tensors."""
    w, s, _, nw = check_window_sizes(window, n_spacings, 1, n_windows)
    return {k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in window_out_shapes(nw, w, s).items()}


def window_step(state, spacings, new_T, new_info, new_status, new_inliers, C_start=None, min_inliers=12, huber_chi=4.0, damping=0.0,
                iterations=2, out=None, workspace=None) -> dict:
    """sslw_window_step: one frame of n_windows sliding windows (include/sslam_window.h).  state: alloc_window_state's dict, read and
    written; spacings (S,) int32 device tensor; new_T (n_windows, S, 12), new_info (n_windows, S, 21) float64, new_status and
    new_inliers (n_windows, S) int32 - what pose_refine_pairs wrote for the frame's S pairs (one window may leave the window axis
    out); C_start (n_windows, 12) float64 or None.  min_inliers: int >= 0; huber_chi: finite > 0; damping: finite >= 0; iterations
    0 .. GRAPH_MAX_ITER.  Returns WINDOW_OUT_KEYS' tensors as a dict (out: alloc_window_out's, or made here).  workspace: optional
    uint8 tensor of at least window_workspace_bytes.  One launch, no host read; everything is judged before the library is loaded."""
    mi, chi, damp, n_iter = check_int("min_inliers", min_inliers, 0, 2 ** 31 - 1), check_positive("huber_chi", huber_chi), check_damping(damping), \
        check_graph_iterations(iterations)
    if not isinstance(state, dict) or set(state) != set(WINDOW_STATE_KEYS) or not all(isinstance(v, torch.Tensor) for v in state.values()):
        raise ValueError(f"state must be a dict of the tensors {', '.join(WINDOW_STATE_KEYS)}")
    rc, tr = state["ring_C"], state["trajectory"]
    if rc.dim() != 3 or tr.dim() != 3 or not isinstance(spacings, torch.Tensor) or spacings.dim() != 1:
        raise ValueError("state `ring_C` (n_windows, window, 12), `trajectory` (n_windows, capacity, 12) and spacings (S,) int32 expected")
    w, s, cap, nw = check_window_sizes(int(rc.shape[1]), int(spacings.shape[0]), int(tr.shape[1]), int(rc.shape[0]))
    for key, (shape, dt) in window_state_shapes(nw, w, s, cap).items():
        _check_arrays(shape, (f"state `{key}`", state[key], dt))
    _check_arrays((s,), ("spacings", spacings, torch.int32))
    new_T = _graph_rows("new_T", new_T, (nw, s), (12,), torch.float64)
    new_info = _graph_rows("new_info", new_info, (nw, s), (21,), torch.float64)
    new_status = _graph_rows("new_status", new_status, (nw, s), (), torch.int32)
    new_inliers = _graph_rows("new_inliers", new_inliers, (nw, s), (), torch.int32)
    if C_start is not None:
        C_start = _graph_rows("C_start", C_start, (nw,), (12,), torch.float64)
    shapes = window_out_shapes(nw, w, s)
    if out is not None and (not isinstance(out, dict) or set(out) != set(WINDOW_OUT_KEYS)):
        raise ValueError(f"out must be a dict of the tensors {', '.join(WINDOW_OUT_KEYS)}")
    o = None if out is None else _outputs(shapes, WINDOW_OUT_KEYS, [out[k] for k in WINDOW_OUT_KEYS])
    need = window_workspace_bytes(nw, w, s)
    _check_workspace(workspace, need)
    st = [state[k] for k in WINDOW_STATE_KEYS]
    dev = common_device(*st, spacings, new_T, new_info, new_status, new_inliers, C_start, workspace, *(o or ()))
    o = _outputs(shapes, WINDOW_OUT_KEYS, None, dev) if o is None else o
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    _run("window_step", window().sslw_window_step, (*st, spacings, new_T, new_info, new_status, new_inliers, C_start, ws, *o),
         *(_dp(x) for x in st), _dp(spacings), _dp(new_T), _dp(new_info), _dp(new_status), _dp(new_inliers), _dp(C_start), nw, w, s, mi,
         C.c_double(chi), C.c_double(damp), n_iter, cap, _dp(ws), *(_dp(x) for x in o))
    return dict(zip(WINDOW_OUT_KEYS, o))


# ---------------------------------------------------------------------------------------- libsslam_place.so (include/sslam_place.h)
# The growing place bank and the edge log of online loop closures: entries with the prefix sslp_ (row "place" of LIBRARIES).
PLACE_EXPORTS = ["sslp_version", "sslp_arch", "sslp_launch_count", "sslp_place_workspace_bytes", "sslp_place_step", "sslp_edge_log_step"]
PLACE_MAX_CAPACITY, PLACE_MAX_K, PLACE_MAX_PER_FRAME, PLACE_MAX_SLOTS = 4096, 4096, 8, 16
PLACE_STATE_KEYS = ("t", "raw", "sum")
PLACE_OUT_KEYS = ("first", "second", "sim", "count", "status", "sig")
EDGE_LOG_STATE_KEYS = ("t", "log_first", "log_second", "log_T", "log_info")
EDGE_LOG_OUT_KEYS = ("logged", "status")
PLACE_COUNTER_OUT_OF_RANGE = 4       # status of both steps: the counter was outside 0 .. capacity - 1


def _place_prototypes(L):
    L.sslp_place_workspace_bytes.restype = C.c_size_t
    p, i, f, ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
    L.sslp_place_workspace_bytes.argtypes = [i]
    L.sslp_place_step.argtypes = [p] * 5 + [i, i, i, i, f, i, i] + [p] * 8
    L.sslp_edge_log_step.argtypes = [p] * 10 + [i, i, i, i, ll] + [p] * 3


def check_place_sizes(capacity, k=1, d=D_OUT) -> tuple:
    """(capacity 1 .., k 1 ..) as ints and d in WIDTHS, else ValueError; past PLACE_MAX_*: SslamHipError - before any device work."""
    cap, kk = check_int("capacity", capacity, 1), check_int("k", k, 1)
    width = check_width(d)
    if cap > PLACE_MAX_CAPACITY or kk > PLACE_MAX_K:
        raise SslamHipError(f"place_step: {_ERR[E_UNSUPPORTED]} (capacity <= {PLACE_MAX_CAPACITY}, k <= {PLACE_MAX_K}; got {cap}, {kk})")
    return cap, kk, width


def place_state_shapes(capacity: int, d: int = D_OUT) -> dict:
    """name -> (shape, dtype) of the persistent state of place_step (PLACE_STATE_KEYS)."""
    return {"t": ((1,), torch.int32), "raw": ((capacity, d), torch.float32), "sum": ((d,), torch.float32)}


def place_out_shapes(per_frame: int, d: int = D_OUT) -> dict:
    """name -> (shape, dtype) of the outputs of place_step (PLACE_OUT_KEYS)."""
    slots, one = ((per_frame,), torch.int32), ((1,), torch.int32)
    return {"first": slots, "second": slots, "sim": ((per_frame,), torch.float32), "count": one, "status": one, "sig": ((d,), torch.float32)}


def place_workspace_bytes(capacity: int) -> int:
    """sslp_place_workspace_bytes, restated: capacity float32 words.  Needs no library."""
    return 4 * capacity


def alloc_place_state(capacity, d=D_OUT, device="cuda") -> dict:
    """A fresh state of place_step: t = 0, everything else zero."""
    cap, _, width = check_place_sizes(capacity, 1, d)
    return {k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in place_state_shapes(cap, width).items()}


def alloc_place_out(per_frame=2, d=D_OUT, device="cuda") -> dict:
    """The outputs of place_step: first and second -1 (absent), everything else zero."""
    per, width = check_int("per_frame", per_frame, 1, PLACE_MAX_PER_FRAME), check_width(d)
    out = {k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in place_out_shapes(per, width).items()}
    out["first"].fill_(-1), out["second"].fill_(-1)
    return out


def _state_dict(name, state, keys):
    if not isinstance(state, dict) or set(state) != set(keys) or not all(isinstance(v, torch.Tensor) for v in state.values()):
        raise ValueError(f"{name} must be a dict of the tensors {', '.join(keys)}")


def place_step(state, descriptors, scores, min_gap=30, min_sim=0.3, per_frame=2, suppress=5, out=None, workspace=None) -> dict:
    """sslp_place_step: one frame of a growing place bank (include/sslam_place.h).  state: alloc_place_state's dict, read and
    written; descriptors (K, D) or (1, K, D) and scores (K,) or (1, K) float32 - one frame as extract() returns it, D the state's
    width.  min_gap, min_sim, per_frame, suppress: loop_candidates'.  Returns PLACE_OUT_KEYS' tensors as a dict (out:
    alloc_place_out's, or made here): first / second / sim (per_frame,), count, status (1,), sig (D,) - row t of loop_candidates over
    frame_signatures of the frames so far, bit for bit; status 4 and an absent row once the bank is full.  workspace: optional uint8
    tensor of at least place_workspace_bytes.  Three launches, no host read; everything is judged before the library is loaded."""
    gap, sim_min, per, sup = check_loop_arguments(min_gap, min_sim, per_frame, suppress)
    _state_dict("state", state, PLACE_STATE_KEYS)
    raw = state["raw"]
    if raw.dim() != 2 or not isinstance(descriptors, torch.Tensor) or not isinstance(scores, torch.Tensor):
        raise ValueError("state `raw` (capacity, D), descriptors (K, D) and scores (K,) float32 tensors expected")
    if descriptors.dim() == 3 and descriptors.shape[0] == 1:
        descriptors = descriptors[0]
    if scores.dim() == 2 and scores.shape[0] == 1:
        scores = scores[0]
    if descriptors.dim() != 2:
        raise ValueError(f"descriptors (K, D) of one frame expected, got {tuple(descriptors.shape)}")
    cap, k, d = check_place_sizes(int(raw.shape[0]), int(descriptors.shape[0]), int(raw.shape[1]))
    for key, (shape, dt) in place_state_shapes(cap, d).items():
        _check_arrays(shape, (f"state `{key}`", state[key], dt))
    _check_arrays((k, d), ("descriptors", descriptors, torch.float32))
    _check_arrays((k,), ("scores", scores, torch.float32))
    shapes = place_out_shapes(per, d)
    if out is not None and (not isinstance(out, dict) or set(out) != set(PLACE_OUT_KEYS)):
        raise ValueError(f"out must be a dict of the tensors {', '.join(PLACE_OUT_KEYS)}")
    o = None if out is None else _outputs(shapes, PLACE_OUT_KEYS, [out[key] for key in PLACE_OUT_KEYS])
    need = place_workspace_bytes(cap)
    _check_workspace(workspace, need)
    st = [state[key] for key in PLACE_STATE_KEYS]
    dev = common_device(*st, descriptors, scores, workspace, *(o or ()))
    o = _outputs(shapes, PLACE_OUT_KEYS, None, dev) if o is None else o
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    _run("place_step", place().sslp_place_step, (*st, descriptors, scores, ws, *o), *(_dp(x) for x in st), _dp(descriptors), _dp(scores),
         cap, k, d, min(gap, 2 ** 31 - 1), C.c_float(sim_min), per, min(sup, 2 ** 31 - 1), _dp(ws), *(_dp(x) for x in o))
    return dict(zip(PLACE_OUT_KEYS, o))


def check_edge_log_sizes(capacity, n_slots) -> tuple:
    """(capacity 1 .., n_slots 1 ..) as ints, else ValueError; past the limits: SslamHipError - before any device work."""
    cap, e = check_int("capacity", capacity, 1), check_int("n_slots", n_slots, 1)
    if e > PLACE_MAX_SLOTS or cap > (2 ** 63 - 1) // 168 // e:
        raise SslamHipError(f"edge_log_step: {_ERR[E_UNSUPPORTED]} (n_slots <= {PLACE_MAX_SLOTS}, capacity * 168 * n_slots < 2^63; got {e}, {cap})")
    return cap, e


def edge_log_shapes(capacity: int, n_slots: int) -> dict:
    """name -> (shape, dtype) of the persistent state of edge_log_step (EDGE_LOG_STATE_KEYS)."""
    rows = capacity * n_slots
    return {"t": ((1,), torch.int32), "log_first": ((rows,), torch.int32), "log_second": ((rows,), torch.int32),
            "log_T": ((rows, 12), torch.float64), "log_info": ((rows, 21), torch.float64)}


def edge_log_out_shapes(n_slots: int) -> dict:
    return {"logged": ((n_slots,), torch.int32), "status": ((1,), torch.int32)}


def alloc_edge_log(capacity, n_slots, device="cuda") -> dict:
    """A fresh state of edge_log_step: t = 0, log_first = -1 (absent) everywhere, everything else zero."""
    cap, e = check_edge_log_sizes(capacity, n_slots)
    state = {k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in edge_log_shapes(cap, e).items()}
    state["log_first"].fill_(-1)
    return state


def edge_log_step(state, slot_first, new_T, new_info, new_status, new_inliers, n_odometry, min_inliers=12, loop_min_inliers=12, out=None) -> dict:
    """sslp_edge_log_step: one frame's E verified pairs appended to the edge log (include/sslam_place.h).  state: alloc_edge_log's
    dict, read and written; slot_first (E,) int32: the global index of every slot's older frame, -1 for none; new_T (E, 12),
    new_info (E, 21) float64, new_status, new_inliers (E,) int32 - what pose_refine_pairs wrote for the frame's E pairs.  The slots
    before n_odometry (0 .. E) are held to min_inliers, the others to loop_min_inliers.  Returns EDGE_LOG_OUT_KEYS' tensors as a dict:
    logged (E,), status (1,) - 4 and nothing logged once the log is full.  One launch, no host read; everything is judged before the
    library is loaded."""
    mi, lmi = check_int("min_inliers", min_inliers, 0, 2 ** 31 - 1), check_int("loop_min_inliers", loop_min_inliers, 0, 2 ** 31 - 1)
    _state_dict("state", state, EDGE_LOG_STATE_KEYS)
    if state["log_first"].dim() != 1 or not isinstance(slot_first, torch.Tensor) or slot_first.dim() != 1 or int(slot_first.shape[0]) < 1 or \
            int(state["log_first"].shape[0]) % int(slot_first.shape[0]):
        raise ValueError("state `log_first` (capacity * E,) and slot_first (E,) int32 expected")
    e = int(slot_first.shape[0])
    cap, e = check_edge_log_sizes(int(state["log_first"].shape[0]) // e, e)
    n_odo = check_int("n_odometry", n_odometry, 0, e)
    for key, (shape, dt) in edge_log_shapes(cap, e).items():
        _check_arrays(shape, (f"state `{key}`", state[key], dt))
    _check_arrays((e,), ("slot_first", slot_first, torch.int32), ("new_status", new_status, torch.int32), ("new_inliers", new_inliers, torch.int32))
    _check_arrays((e, 12), ("new_T", new_T, torch.float64))
    _check_arrays((e, 21), ("new_info", new_info, torch.float64))
    shapes = edge_log_out_shapes(e)
    if out is not None and (not isinstance(out, dict) or set(out) != set(EDGE_LOG_OUT_KEYS)):
        raise ValueError(f"out must be a dict of the tensors {', '.join(EDGE_LOG_OUT_KEYS)}")
    o = None if out is None else _outputs(shapes, EDGE_LOG_OUT_KEYS, [out[key] for key in EDGE_LOG_OUT_KEYS])
    st = [state[key] for key in EDGE_LOG_STATE_KEYS]
    dev = common_device(*st, slot_first, new_T, new_info, new_status, new_inliers, *(o or ()))
    o = _outputs(shapes, EDGE_LOG_OUT_KEYS, None, dev) if o is None else o
    _run("edge_log_step", place().sslp_edge_log_step, (*st, slot_first, new_T, new_info, new_status, new_inliers, *o), *(_dp(x) for x in st),
         _dp(slot_first), _dp(new_T), _dp(new_info), _dp(new_status), _dp(new_inliers), e, n_odo, mi, lmi, cap, *(_dp(x) for x in o))
    return dict(zip(EDGE_LOG_OUT_KEYS, o))


# ------------------------------------------------------------------------------------------ libsslam_conf.so (include/sslam_conf.h)
# The keypoint confidence head: entries with the prefix sslc_ (row "conf" of LIBRARIES; csrc/common.h and csrc/gather_taps.h are
# included from where they are).
CONF_EXPORTS = ["sslc_version", "sslc_arch", "sslc_launch_count", "sslc_confidence_layout", "sslc_confidence_pack_host",
                "sslc_confidence_rows", "sslc_gather_confidence", "sslc_confidence_filter", "sslc_take_rows"]
CONF_DINO_DIM, CONF_HIDDEN_DIM, CONF_FILTER_MAX_K = 384, 128, 4096
CONF_STATE_KEYS = ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias")
CONF_FILTER_KEYS = ("slot", "count", "confidence")


class ConfidenceLayout(C.Structure):
    _fields_ = [("d", C.c_int), ("total", C.c_longlong), ("w1", C.c_longlong), ("b1", C.c_longlong), ("w2", C.c_longlong),
                ("b2", C.c_longlong), ("w3", C.c_longlong), ("b3", C.c_longlong)]


def _conf_prototypes(L):
    p, i, ll, f = C.c_void_p, C.c_int, C.c_longlong, C.c_float
    L.sslc_confidence_layout.argtypes = [i, i, i, C.POINTER(ConfidenceLayout)]
    L.sslc_confidence_pack_host.argtypes = [p, i, i, i, p]
    L.sslc_confidence_rows.argtypes = [p, p, ll, i, p, p, p]
    L.sslc_gather_confidence.argtypes = [p, i, i, p, i, p, i, p, p, p]
    L.sslc_confidence_filter.argtypes = [p, i, i, f, p, p, p, p]
    L.sslc_take_rows.argtypes = [p, p, i, i, i, p, p]


def confidence_supported(dino_dim, descriptor_dim, hidden_dim) -> bool:
    """Whether the kernels are built for a head of these widths (include/sslam_conf.h): 384, 128 or 256, 128."""
    return (dino_dim, hidden_dim) == (CONF_DINO_DIM, CONF_HIDDEN_DIM) and descriptor_dim in WIDTHS


def confidence_layout(descriptor_dim: int, dino_dim: int = CONF_DINO_DIM, hidden_dim: int = CONF_HIDDEN_DIM) -> ConfidenceLayout:
    """Offsets (floats) of the packed confidence head; SslamHipError (unsupported shape) for widths the kernels are not built for."""
    lay = ConfidenceLayout()
    _check(conf().sslc_confidence_layout(int(dino_dim), int(descriptor_dim), int(hidden_dim), C.byref(lay)), "confidence_layout")
    return lay


def confidence_pack(weights: list) -> np.ndarray:
    """weights: the six fp32 arrays of the head in state_dict order (CONF_STATE_KEYS): mlp.0.weight (h, 384 + d), mlp.0.bias (h),
    mlp.2.weight (h / 2, h), mlp.2.bias (h / 2), mlp.4.weight (1, h / 2), mlp.4.bias (1).  Returns the packed buffer
    (sslc_confidence_pack_host); SslamHipError (unsupported shape) unless h = 128 and d is 128 or 256."""
    ws = [np.ascontiguousarray(w, np.float32) for w in weights]
    if len(ws) != 6 or ws[0].ndim != 2 or ws[2].ndim != 2:
        raise ValueError("six arrays in state_dict order expected: mlp.0.weight, mlp.0.bias, mlp.2.weight, mlp.2.bias, mlp.4.weight, mlp.4.bias")
    h, k1 = int(ws[0].shape[0]), int(ws[0].shape[1])
    want = [(h, k1), (h,), (h // 2, h), (h // 2,), (1, h // 2), (1,)]
    if h < 2 or k1 <= CONF_DINO_DIM or [tuple(w.shape) for w in ws] != want:
        raise ValueError(f"a confidence head of shapes {[tuple(w.shape) for w in ws]}: {want} expected, with more than {CONF_DINO_DIM} inputs")
    lay = confidence_layout(k1 - CONF_DINO_DIM, CONF_DINO_DIM, h)
    out = np.empty(lay.total, np.float32)
    arr = (C.c_void_p * 6)(*[w.ctypes.data for w in ws])
    _check(conf().sslc_confidence_pack_host(arr, CONF_DINO_DIM, k1 - CONF_DINO_DIM, h, out.ctypes.data), "confidence_pack")
    return out


_CONF_PACKED_WIDTH = {}      # floats -> descriptor width


def packed_confidence_width(packed) -> int:
    """The descriptor width a packed confidence head was laid out for, from its length."""
    n = int(packed.numel())
    if not _CONF_PACKED_WIDTH:
        _CONF_PACKED_WIDTH.update({int(confidence_layout(d).total): d for d in WIDTHS})
    if n not in _CONF_PACKED_WIDTH:
        raise ValueError(f"a packed confidence head of {n} floats fits no supported descriptor width {WIDTHS}")
    return _CONF_PACKED_WIDTH[n]


def _f32_rows(name, t, width):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() < 1 or int(t.shape[-1]) != width or not t.is_contiguous() or \
            t.numel() == 0:
        raise ValueError(f"{name} must be a contiguous float32 tensor of shape (..., {width})")


def confidence_rows(x, desc, packed, out=None):
    """sslc_confidence_rows: x (..., 384) and desc (..., d) fp32, the features at the keypoints and their descriptors; packed: the
    head (confidence_pack) on the device -> confidence (...) fp32 in [0, 1].  d is the width `packed` was laid out for."""
    d = packed_confidence_width(packed)
    _f32_rows("x", x, C_FEAT)
    _f32_rows("desc", desc, d)
    if tuple(x.shape[:-1]) != tuple(desc.shape[:-1]):
        raise ValueError(f"x of shape {tuple(x.shape)} and desc of shape {tuple(desc.shape)} do not hold the same rows")
    lead = tuple(x.shape[:-1])
    _check_arrays(lead, ("out", out, torch.float32))
    if out is None:
        out = torch.empty(lead, dtype=torch.float32, device=x.device)
    _run("confidence_rows", conf().sslc_confidence_rows, (x, desc, packed, out), _dp(x), _dp(desc), x.numel() // C_FEAT, d, _dp(packed), _dp(out))
    return out


def gather_confidence(feat, kp, desc, packed, out=None):
    """sslc_gather_confidence: the confidence of the keypoints kp (n, K, 2) with descriptors desc (n, K, d), the features taken
    from feat (n, G, G, 384) by gather()'s arithmetic inside the kernel -> (n, K) fp32: the bits of
    confidence_rows(gather(feat, kp), desc, packed), nothing of width 384 written."""
    d = packed_confidence_width(packed)
    if not isinstance(feat, torch.Tensor) or feat.dtype != torch.float32 or feat.dim() != 4 or feat.shape[1] != feat.shape[2] or \
            int(feat.shape[3]) != C_FEAT or not feat.is_contiguous() or int(feat.shape[1]) < 2:
        raise ValueError(f"feat must be a contiguous float32 tensor of shape (n, G, G, {C_FEAT}), G >= 2")
    n, g = int(feat.shape[0]), int(feat.shape[1])
    if not isinstance(kp, torch.Tensor) or kp.dim() != 3 or int(kp.shape[0]) != n or int(kp.shape[1]) < 1:
        raise ValueError(f"kp must be a contiguous float32 tensor of shape ({n}, K, 2)")
    k = int(kp.shape[1])
    _check_arrays((n, k, 2), ("kp", kp, torch.float32))
    _check_arrays((n, k, d), ("desc", desc, torch.float32))
    _check_arrays((n, k), ("out", out, torch.float32))
    if out is None:
        out = torch.empty((n, k), dtype=torch.float32, device=feat.device)
    _run("gather_confidence", conf().sslc_gather_confidence, (feat, kp, desc, packed, out), _dp(feat), n, g, _dp(kp), k, _dp(desc), d,
         _dp(packed), _dp(out))
    return out


def confidence_filter_shapes(n: int, k: int) -> dict:
    """The outputs of confidence_filter for n frames of k keypoints: key -> (shape, dtype), in the entry's order."""
    return {"slot": ((n, k), torch.int32), "count": ((n,), torch.int32), "confidence": ((n, k), torch.float32)}


def check_conf_threshold(threshold) -> float:
    """threshold as a float32 value: any number (2.0 keeps each frame's best keypoint alone); not a bool, a string or a tensor."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"threshold must be a number, got {threshold!r}")
    return float(np.float32(threshold))


def confidence_filter(confidence, threshold=0.5, out=None):
    """sslc_confidence_filter: confidence (n, K) fp32 -> (slot (n, K) int32, count (n,) int32, conf_out (n, K) fp32).  Per frame the
    slots with confidence >= float32(threshold) in ascending order, the frame's largest confidence alone where none passes; the
    rest of `slot` repeats the last kept slot and the rest of conf_out is 0 (filter_keypoints_by_confidence's pad).  One launch."""
    thr = check_conf_threshold(threshold)
    if not isinstance(confidence, torch.Tensor) or confidence.dim() != 2 or min(confidence.shape) < 1:
        raise ValueError("confidence must be a contiguous float32 tensor of shape (n, K)")
    n, k = int(confidence.shape[0]), int(confidence.shape[1])
    _check_arrays((n, k), ("confidence", confidence, torch.float32))
    if k > CONF_FILTER_MAX_K:
        raise SslamHipError(f"confidence_filter: {_ERR[E_UNSUPPORTED]} (K <= {CONF_FILTER_MAX_K}; got K = {k})")
    shapes = confidence_filter_shapes(n, k)
    if out is not None:
        if len(out) != 3:
            raise ValueError("out must be (slot, count, conf_out)")
        for key, t in zip(CONF_FILTER_KEYS, out):
            if t is None:
                raise ValueError(f"out `{key}` is required")
            _check_arrays(shapes[key][0], (f"out `{key}`", t, shapes[key][1]))
    dev = common_device(confidence, *(out or ()))
    slot, count, co = out if out is not None else (torch.empty(shapes[key][0], dtype=shapes[key][1], device=dev) for key in CONF_FILTER_KEYS)
    _run("confidence_filter", conf().sslc_confidence_filter, (confidence, slot, count, co), _dp(confidence), n, k, thr, _dp(slot), _dp(count),
         _dp(co))
    return slot, count, co


def take_rows(src, slot, out=None):
    """sslc_take_rows: out[f, j, ...] = src[f, slot[f, j], ...] for src (n, K, ...) of a 4-byte dtype (float32, int32) and slot
    (n, K) int32; out: an optional tensor of src's shape and dtype that is not src.  One launch."""
    if not isinstance(src, torch.Tensor) or src.dim() < 2 or src.element_size() != 4 or not src.is_contiguous() or src.numel() == 0:
        raise ValueError("src must be a contiguous tensor of shape (n, K, ...) and a 4-byte dtype")
    n, k = int(src.shape[0]), int(src.shape[1])
    _check_arrays((n, k), ("slot", slot, torch.int32))
    if slot is None:
        raise ValueError("slot is required")
    _check_arrays(tuple(src.shape), ("out", out, src.dtype))
    if out is None:
        out = torch.empty_like(src)
    if out.data_ptr() == src.data_ptr():
        raise ValueError("out must not be src")
    _run("take_rows", conf().sslc_take_rows, (src, slot, out), _dp(src), _dp(slot), n, k, src.numel() // (n * k), _dp(out))
    return out


# -------------------------------------------------------------------------------------- libsslam_weight.so (include/sslam_weight.h)
# Per-match weights from keypoint confidences and the pose refinement that takes them: entries with the prefix sslu_ (row "weight"
# of LIBRARIES; csrc/pose_refine_common.h is included from where it is: the weighted kernel is pose_refine_pairs' own body).
WEIGHT_EXPORTS = ["sslu_version", "sslu_arch", "sslu_launch_count", "sslu_match_weights", "sslu_pose_refine_weighted_pairs"]
WEIGHT_PRODUCT, WEIGHT_EXPECTED_ERROR = 0, 1      # SSLU_WEIGHT_PRODUCT, SSLU_WEIGHT_EXPECTED_ERROR
POSE_REFINE_WEIGHTED_KEYS = POSE_REFINE_KEYS + ("weight_sum",)


def _weight_prototypes(L):
    p, i, d = C.c_void_p, C.c_int, C.c_double
    L.sslu_match_weights.argtypes = [p, i, i, p, p, i, p, p, i, i, d, p, p]
    L.sslu_pose_refine_weighted_pairs.argtypes = [p, p, i, i, p, p, i, p, p, i] + [d] * 10 + [p, d, i, p] + [p] * 13 + [p]


def check_weights(mode, sigma0=1.0) -> tuple:
    """(mode, sigma0) of match_weights: mode WEIGHT_PRODUCT or WEIGHT_EXPECTED_ERROR; sigma0 a finite number > 0 under the second
    (ignored, and returned as 1.0, under the first) - else ValueError, before any device work."""
    if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)) or int(mode) not in (WEIGHT_PRODUCT, WEIGHT_EXPECTED_ERROR):
        raise ValueError(f"mode must be WEIGHT_PRODUCT ({WEIGHT_PRODUCT}) or WEIGHT_EXPECTED_ERROR ({WEIGHT_EXPECTED_ERROR}), got {mode!r}")
    return int(mode), (check_positive("sigma0", sigma0) if int(mode) == WEIGHT_EXPECTED_ERROR else 1.0)


def pose_refine_weighted_shapes(n_pairs: int, n1: int) -> dict:
    """name -> (shape, dtype) of the outputs of pose_refine_weighted: pose_refine_shapes and weight_sum (P,) float64."""
    return {**pose_refine_shapes(n_pairs, n1), "weight_sum": ((n_pairs,), torch.float64)}


def match_weights(conf_bank, first, second, matches, count, mode=WEIGHT_PRODUCT, sigma0=1.0, out=None):
    """sslu_match_weights: conf_bank (n_bank, K) fp32, the keypoint confidences; first / second, matches (P, n1, 2) int64 and count
    (P,) int32 as pose_refine_pairs takes them; mode and sigma0 as check_weights judges them.
    Returns weight (P, n1) fp32, every element written: c1 * c2 or sigma0^2 / (sigma0^2 + e1^2 + e2^2) with e = 1 / (c + 1e-6) - 1,
    +0.0 for a slot that holds no match (include/sslam_weight.h).  out: an optional tensor of that shape.  One launch, no host read."""
    _check_bank("conf_bank", conf_bank, ("K",))
    n_bank, k = int(conf_bank.shape[0]), int(conf_bank.shape[1])
    n_pairs = check_pair_lists(first, second, conf_bank.device)
    if not isinstance(matches, torch.Tensor) or matches.dim() != 3 or matches.shape[2] != 2 or int(matches.shape[0]) != n_pairs or \
            int(matches.shape[1]) < 1:
        raise ValueError(f"matches must be a tensor of shape ({n_pairs}, n1 >= 1, 2)")
    n1 = int(matches.shape[1])
    if count is None:
        raise ValueError("count is required")
    _check_arrays((n_pairs, n1, 2), ("matches", matches, torch.int64))
    _check_arrays((n_pairs,), ("count", count, torch.int32))
    mode, s0 = check_weights(mode, sigma0)
    _check_arrays((n_pairs, n1), ("out", out, torch.float32))
    if n_pairs * n1 > 0x7fffffff:
        raise SslamHipError(f"match_weights: {_ERR[E_UNSUPPORTED]} (n_pairs * n1 <= 2^31 - 1; got {n_pairs * n1})")
    dev = common_device(conf_bank, first, second, matches, count, out)
    if out is None:
        out = torch.empty((n_pairs, n1), dtype=torch.float32, device=dev)
    _run("match_weights", weight().sslu_match_weights, (conf_bank, first, second, matches, count, out), _dp(conf_bank), n_bank, k,
         _dp(first), _dp(second), n_pairs, _dp(matches), _dp(count), n1, mode, s0, _dp(out))
    return out


def pose_refine_weighted(kp_bank, kp_depth_bank, first, second, matches, count, camera, T_in, weights, scale_x=1.0, scale_y=1.0,
                         threshold=3.0, huber=1.0, iterations=5, out=None):
    """sslu_pose_refine_weighted_pairs: pose_refine_pairs' arguments and weights (P, n1) fp32, the weight of every match slot
    (match_weights' output, or any other).  A row whose weight is not finite and > 0 is not selected; a selected row's weight
    multiplies its Huber terms (include/sslam_weight.h).
    Returns pose_refine_pairs' twelve tensors and weight_sum (P,) float64 - POSE_REFINE_WEIGHTED_KEYS; info is the weighted
    information matrix.  out: optional tensors of those shapes (T must not be T_in).  One launch, no host read."""
    n_bank, k, n_pairs, n1, _, doubles = _pose_operands("pose_refine_weighted", kp_bank, first, second, threshold,
                                                        depth=(kp_depth_bank, camera, scale_x, scale_y), listed=(matches, count))
    hub, n_iter = check_huber(huber), check_iterations(iterations)
    _check_pose_rows("T_in", T_in, n_pairs, 12)
    if weights is None:
        raise ValueError("weights is required: pose_refine_pairs is the unweighted entry")
    _check_arrays((n_pairs, n1), ("weights", weights, torch.float32))
    shapes = pose_refine_weighted_shapes(n_pairs, n1)
    o = None if out is None else _outputs(shapes, POSE_REFINE_WEIGHTED_KEYS, out)
    if o is not None and o[0].data_ptr() == T_in.data_ptr():
        raise ValueError("out `T` must not be T_in")
    dev = common_device(kp_bank, kp_depth_bank, first, second, matches, count, T_in, weights)
    o = _outputs(shapes, POSE_REFINE_WEIGHTED_KEYS, None, dev) if o is None else o
    _run("pose_refine_weighted", weight().sslu_pose_refine_weighted_pairs,
         (kp_bank, kp_depth_bank, first, second, matches, count, T_in, weights, *o), _dp(kp_bank), _dp(kp_depth_bank), n_bank, k, _dp(first),
         _dp(second), n_pairs, _dp(matches), _dp(count), n1, *doubles, _dp(T_in), C.c_double(hub), n_iter, _dp(weights),
         *(_dp(x) for x in o))
    return tuple(o)


# ---------------------------------------------------------------------------------------- libsslam_track.so (include/sslam_track.h)
# Feature tracks and a landmark map: entries with the prefix sslt_ (row "track" of LIBRARIES).
TRACK_EXPORTS = ["sslt_version", "sslt_arch", "sslt_launch_count", "sslt_link_pairs", "sslt_track_workspace_bytes", "sslt_track_ids",
                 "sslt_landmarks", "sslt_track_step"]
TRACK_MAX_K, TRACK_SCAN_TILE, TRACK_MAX_NODES = 4096, 1024, 0x7fffffff      # SSLT_MAX_K, SSLT_SCAN_TILE, n_bank * K
LINK_KEYS = ("prev", "next", "prev_frame", "next_frame")
TRACK_ID_KEYS = ("track_id", "age", "n_tracks", "root_frame", "root_slot", "length")
LANDMARK_KEYS = ("xyz", "n_obs", "n_kept", "status", "weight_sum", "rms", "residual", "kept")
TRACK_STATE_KEYS = ("t", "next_id", "prev", "next", "prev_frame", "next_frame", "track_id", "age")
TRACK_OUT_KEYS = ("track_id", "age", "n_new", "status")
TRACK_COUNTER_OUT_OF_RANGE = 4       # status of track_step: the counter was outside 0 .. capacity - 1


def _track_prototypes(L):
    L.sslt_track_workspace_bytes.restype = C.c_size_t
    p, i, d = C.c_void_p, C.c_int, C.c_double
    L.sslt_track_workspace_bytes.argtypes = [i, i]
    L.sslt_link_pairs.argtypes = [p, p, i, p, p, p, i, i, i, p, p, p, p, p]
    L.sslt_track_ids.argtypes = [p, p, i, i] + [p] * 7 + [p]
    L.sslt_landmarks.argtypes = [p, p, p, i, i] + [d] * 10 + [p] * 6 + [i] + [p] * 8 + [p]
    L.sslt_track_step.argtypes = [p] * 12 + [i, i, i] + [p] * 4 + [p]


def check_track_sizes(what: str, n_bank, k, limit_k: bool = False) -> tuple:
    """(n_bank 1 .., k 1 ..) as ints, else ValueError; n_bank * k past 2^31 - 1, or k past TRACK_MAX_K where the entry keeps a row
    in LDS: SslamHipError - before any device work."""
    nb, kk = check_int("n_bank", n_bank, 1), check_int("k", k, 1)
    if nb * kk > TRACK_MAX_NODES or (limit_k and kk > TRACK_MAX_K):
        raise SslamHipError(f"{what}: {_ERR[E_UNSUPPORTED]} (n_bank * k <= 2^31 - 1" + (f", k <= {TRACK_MAX_K}" if limit_k else "") +
                            f"; got {nb}, {kk})")
    return nb, kk


def link_shapes(n_bank: int, k: int) -> dict:
    """name -> (shape, dtype) of the outputs of link_pairs (LINK_KEYS)."""
    return {"prev": ((n_bank, k), torch.int32), "next": ((n_bank, k), torch.int32), "prev_frame": ((n_bank,), torch.int32),
            "next_frame": ((n_bank,), torch.int32)}


def track_id_shapes(n_bank: int, k: int) -> dict:
    """name -> (shape, dtype) of the outputs of track_ids (TRACK_ID_KEYS)."""
    bank, rows = ((n_bank, k), torch.int32), ((n_bank * k,), torch.int32)
    return {"track_id": bank, "age": bank, "n_tracks": ((1,), torch.int32), "root_frame": rows, "root_slot": rows, "length": rows}


def landmark_shapes(n_bank: int, k: int) -> dict:
    """name -> (shape, dtype) of the outputs of landmarks (LANDMARK_KEYS): per track (n_bank * k rows), then per keypoint."""
    n = n_bank * k
    return {"xyz": ((n, 3), torch.float64), "n_obs": ((n,), torch.int32), "n_kept": ((n,), torch.int32), "status": ((n,), torch.int32),
            "weight_sum": ((n,), torch.float64), "rms": ((n,), torch.float64), "residual": ((n_bank, k), torch.float64),
            "kept": ((n_bank, k), torch.int32)}


def track_state_shapes(capacity: int, k: int) -> dict:
    """name -> (shape, dtype) of the persistent state of track_step (TRACK_STATE_KEYS)."""
    one, bank, frames = ((1,), torch.int32), ((capacity, k), torch.int32), ((capacity,), torch.int32)
    return {"t": one, "next_id": one, "prev": bank, "next": bank, "prev_frame": frames, "next_frame": frames, "track_id": bank, "age": bank}


def track_out_shapes(k: int) -> dict:
    """name -> (shape, dtype) of the outputs of track_step (TRACK_OUT_KEYS)."""
    return {"track_id": ((k,), torch.int32), "age": ((k,), torch.int32), "n_new": ((1,), torch.int32), "status": ((1,), torch.int32)}


def track_workspace_bytes(n_bank: int, k: int) -> int:
    """sslt_track_workspace_bytes, restated: 20 bytes per node and one word per scan tile.  Needs no library."""
    n = n_bank * k
    return 20 * n + 4 * (-(-n // TRACK_SCAN_TILE))


def _dict_out(shapes, keys, out):
    if out is None:
        return None
    if not isinstance(out, dict) or set(out) != set(keys):
        raise ValueError(f"out must be a dict of the tensors {', '.join(keys)}")
    return _outputs(shapes, keys, [out[key] for key in keys])


def _link_row_operands(n_rows, matches, count, mask, k):
    """One or many link rows: matches (n_rows, n1, 2) int64, count (n_rows,) int32, mask (n_rows, n1) int32 or None -> n1."""
    if not isinstance(matches, torch.Tensor) or matches.dim() != 3 or matches.shape[2] != 2 or int(matches.shape[0]) != n_rows or \
            int(matches.shape[1]) < 1:
        raise ValueError(f"matches must be a tensor of shape ({n_rows}, n1 >= 1, 2)")
    n1 = int(matches.shape[1])
    if count is None:
        raise ValueError("count is required")
    _check_arrays((n_rows, n1, 2), ("matches", matches, torch.int64))
    _check_arrays((n_rows,), ("count", count, torch.int32))
    _check_arrays((n_rows, n1), ("mask", mask, torch.int32))
    return n1


def link_pairs(first, second, matches, count, n_bank, k, mask=None, out=None) -> dict:
    """sslt_link_pairs: first / second (P,) int32 device lists, matches (P, n1, 2) int64 and count (P,) int32 as match_pairs or
    match_rank wrote them, mask (P, n1) int32 or None - where given only slots with mask == 1 count (pose_ransac_pairs' or
    pose_refine_pairs' inlier_of_slot) - over a bank of n_bank frames of k slots.  Returns LINK_KEYS' tensors as a dict: prev, next
    (n_bank, k), prev_frame, next_frame (n_bank,) int32, -1 meaning none, every element written (include/sslam_track.h: the
    two-sided lowest-row and lowest-slot rules).  Five launches, no host read."""
    n_pairs = check_pair_lists(first, second)
    nb, kk = check_track_sizes("link_pairs", n_bank, k, limit_k=True)
    n1 = _link_row_operands(n_pairs, matches, count, mask, kk)
    shapes = link_shapes(nb, kk)
    o = _dict_out(shapes, LINK_KEYS, out)
    dev = common_device(first, second, matches, count, mask, *(o or ()))
    o = _outputs(shapes, LINK_KEYS, None, dev) if o is None else o
    _run("link_pairs", track().sslt_link_pairs, (first, second, matches, count, mask, *o), _dp(first), _dp(second), n_pairs, _dp(matches),
         _dp(count), _dp(mask), n1, nb, kk, *(_dp(x) for x in o))
    return dict(zip(LINK_KEYS, o))


def track_ids(prev, prev_frame, out=None, workspace=None) -> dict:
    """sslt_track_ids: prev (n_bank, k) and prev_frame (n_bank,) int32 of link_pairs (or of a track bank's state).  Returns
    TRACK_ID_KEYS' tensors as a dict: track_id, age (n_bank, k), n_tracks (1,), root_frame, root_slot, length (n_bank * k,) int32 -
    roots numbered in ascending (frame, slot) order, rows past n_tracks -1, -1, 0.  workspace: optional uint8 tensor of at least
    track_workspace_bytes, 8-byte aligned.  5 + ceil(log2 n_bank) launches, no host read."""
    if not isinstance(prev, torch.Tensor) or prev.dim() != 2:
        raise ValueError("prev must be an int32 tensor of shape (n_bank, k)")
    nb, kk = check_track_sizes("track_ids", int(prev.shape[0]), int(prev.shape[1]))
    _check_arrays((nb, kk), ("prev", prev, torch.int32))
    if prev_frame is None:
        raise ValueError("prev_frame is required")
    _check_arrays((nb,), ("prev_frame", prev_frame, torch.int32))
    shapes = track_id_shapes(nb, kk)
    o = _dict_out(shapes, TRACK_ID_KEYS, out)
    need = track_workspace_bytes(nb, kk)
    _check_workspace(workspace, need)
    dev = common_device(prev, prev_frame, workspace, *(o or ()))
    o = _outputs(shapes, TRACK_ID_KEYS, None, dev) if o is None else o
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    _run("track_ids", track().sslt_track_ids, (prev, prev_frame, ws, *o), _dp(prev), _dp(prev_frame), nb, kk, _dp(ws), *(_dp(x) for x in o))
    return dict(zip(TRACK_ID_KEYS, o))


def check_min_obs(min_obs) -> int:
    """min_obs of landmarks as an int >= 2, else ValueError."""
    return check_int("min_obs", min_obs, 2, 2 ** 31 - 1)


def landmarks(kp_bank, kp_depth_bank, poses, camera, next_slot, next_frame, root_frame, root_slot, n_tracks, weight=None, scale_x=1.0, scale_y=1.0,
              threshold=3.0, min_obs=2, out=None) -> dict:
    """sslt_landmarks: kp_bank (n_bank, k, 2) fp32 and kp_depth_bank (n_bank, k) int32 as pose_refine_pairs takes them; poses (n_bank, 12)
    or (n_bank, 3, 4) float64, world -> camera [R | t] of every frame (a graph's C); next_slot, next_frame: `next` and `next_frame` of link_pairs; root_frame,
    root_slot, n_tracks of track_ids; weight (n_bank, k) fp32 or None (1 for every keypoint) - extract()'s `confidence` as it is.
    Returns LANDMARK_KEYS' tensors as a dict: per track (n_bank * k rows) xyz (3), n_obs, n_kept, status (0 refit over the kept, 1 the
    first mean, 2 no observation, -1 past n_tracks), weight_sum, rms; per keypoint residual (-1: no observation) and kept
    (include/sslam_track.h).  Two launches, no host read."""
    _check_bank("kp_bank", kp_bank, ("K", 2))
    nb, kk = check_track_sizes("landmarks", int(kp_bank.shape[0]), int(kp_bank.shape[1]))
    for name, t in (("kp_depth_bank", kp_depth_bank), ("poses", poses), ("next_slot", next_slot), ("next_frame", next_frame), ("root_frame", root_frame),
                    ("root_slot", root_slot), ("n_tracks", n_tracks)):
        if t is None:
            raise ValueError(f"{name} is required")
    _check_arrays((nb, kk), ("kp_depth_bank", kp_depth_bank, torch.int32), ("next_slot", next_slot, torch.int32), ("weight", weight, torch.float32))
    _check_arrays((nb,), ("next_frame", next_frame, torch.int32))
    _check_arrays((nb * kk,), ("root_frame", root_frame, torch.int32), ("root_slot", root_slot, torch.int32))
    _check_arrays((1,), ("n_tracks", n_tracks, torch.int32))
    _check_pose_rows("poses", poses, nb, 12)
    fx, fy, cx, cy, ds, vw, vh = check_camera(camera)
    doubles = (fx, fy, cx, cy, ds, check_positive("scale_x", scale_x), check_positive("scale_y", scale_y), vw, vh, check_threshold(threshold))
    mo = check_min_obs(min_obs)
    shapes = landmark_shapes(nb, kk)
    o = _dict_out(shapes, LANDMARK_KEYS, out)
    ins = (kp_bank, kp_depth_bank, poses, next_slot, next_frame, root_frame, root_slot, n_tracks, weight)
    dev = common_device(*ins, *(o or ()))
    o = _outputs(shapes, LANDMARK_KEYS, None, dev) if o is None else o
    _run("landmarks", track().sslt_landmarks, (*ins, *o), _dp(kp_bank), _dp(kp_depth_bank), _dp(poses), nb, kk, *(C.c_double(v) for v in doubles),
         _dp(next_slot), _dp(next_frame), _dp(root_frame), _dp(root_slot), _dp(n_tracks), _dp(weight), mo, *(_dp(x) for x in o))
    return dict(zip(LANDMARK_KEYS, o))


def alloc_track_state(capacity, k, device="cuda") -> dict:
    """A fresh state of track_step: t = 0, next_id = 0, everything else zero (nothing of it is read before it is written)."""
    cap, kk = check_track_sizes("track_step", capacity, k, limit_k=True)
    return {key: torch.zeros(shape, dtype=dt, device=device) for key, (shape, dt) in track_state_shapes(cap, kk).items()}


def alloc_track_out(k, device="cuda") -> dict:
    """The outputs of track_step: track_id and age -1, n_new and status zero."""
    kk = check_int("k", k, 1, TRACK_MAX_K)
    out = {key: torch.zeros(shape, dtype=dt, device=device) for key, (shape, dt) in track_out_shapes(kk).items()}
    out["track_id"].fill_(-1), out["age"].fill_(-1)
    return out


def track_step(state, matches, count, first, mask=None, out=None) -> dict:
    """sslt_track_step: one frame of a growing track bank (include/sslam_track.h).  state: alloc_track_state's dict, read and written;
    matches (n1, 2) or (1, n1, 2) int64, count (1,) int32 and mask (n1,) or (1, n1) int32 or None: this step's link row, one row of
    link_pairs' operands; first (1,) int32 DEVICE: the bank frame the row's first member names, -1 for none.  Returns TRACK_OUT_KEYS'
    tensors as a dict (out: alloc_track_out's, or made here): this frame's track_id, age (k,), n_new, status (1,) - 4, ids and ages
    -1 and the state untouched once the bank is full.  After n steps the state's rows equal link_pairs + track_ids over the rows
    stepped so far, bit for bit.  One launch, no host value, no host read."""
    _state_dict("state", state, TRACK_STATE_KEYS)
    if state["prev"].dim() != 2:
        raise ValueError("state `prev` (capacity, k) expected")
    cap, kk = check_track_sizes("track_step", int(state["prev"].shape[0]), int(state["prev"].shape[1]), limit_k=True)
    for key, (shape, dt) in track_state_shapes(cap, kk).items():
        _check_arrays(shape, (f"state `{key}`", state[key], dt))
    if isinstance(matches, torch.Tensor) and matches.dim() == 2:
        matches = matches[None]
    if isinstance(mask, torch.Tensor) and mask.dim() == 1:
        mask = mask[None]
    n1 = _link_row_operands(1, matches, count, mask, kk)
    if first is None:
        raise ValueError("first is required")
    _check_arrays((1,), ("first", first, torch.int32))
    shapes = track_out_shapes(kk)
    o = _dict_out(shapes, TRACK_OUT_KEYS, out)
    st = [state[key] for key in TRACK_STATE_KEYS]
    dev = common_device(*st, matches, count, mask, first, *(o or ()))
    o = _outputs(shapes, TRACK_OUT_KEYS, None, dev) if o is None else o
    _run("track_step", track().sslt_track_step, (*st, matches, count, mask, first, *o), *(_dp(x) for x in st), _dp(matches), _dp(count),
         _dp(mask), _dp(first), n1, kk, cap, *(_dp(x) for x in o))
    return dict(zip(TRACK_OUT_KEYS, o))


# ------------------------------------------------------------------------------------------------------ the native libraries
# One row per library, in build order: name, prefix, directory, shared object, header, export list, DEPS of its Makefile, prototypes.
_HIP_H, _GRAPH_H = "../../include/sslam_hip.h", "../../include/sslam_graph.h"
LIBRARIES = {row.name: row for row in (
    Library("lib", "sslam", "csrc", "libsslam_hip.so", "sslam_hip.h", EXPORTS, (_HIP_H,), _prototypes),
    Library("ext", "sslx", "csrc_ext", "libsslam_ext.so", "sslam_ext.h", EXT_EXPORTS, ("../../include/sslam_ext.h", _HIP_H), _ext_prototypes),
    Library("graph", "sslg", "csrc_graph", "libsslam_graph.so", "sslam_graph.h", GRAPH_EXPORTS, (_GRAPH_H, _HIP_H), _graph_prototypes),
    Library("loop", "ssll", "csrc_loop", "libsslam_loop.so", "sslam_loop.h", LOOP_EXPORTS,
            ("../csrc_graph/edge_terms.h", "../csrc_graph/gauss_newton.h", "../../include/sslam_loop.h", _GRAPH_H, _HIP_H), _loop_prototypes),
    Library("window", "sslw", "csrc_window", "libsslam_window.so", "sslam_window.h", WINDOW_EXPORTS,
            ("../csrc_graph/edge_terms.h", "../csrc_graph/gauss_newton.h", "../csrc_graph/edge_walk.h", "../../include/sslam_window.h", _GRAPH_H,
             _HIP_H), _window_prototypes),
    Library("place", "sslp", "csrc_place", "libsslam_place.so", "sslam_place.h", PLACE_EXPORTS, ("../../include/sslam_place.h", _HIP_H),
            _place_prototypes),
    Library("conf", "sslc", "csrc_conf", "libsslam_conf.so", "sslam_conf.h", CONF_EXPORTS,
            ("../csrc/common.h", "../csrc/gather_taps.h", "../../include/sslam_conf.h", _HIP_H), _conf_prototypes),
    Library("weight", "sslu", "csrc_weight", "libsslam_weight.so", "sslam_weight.h", WEIGHT_EXPORTS,
            ("../csrc/common.h", "../csrc/pose_common.h", "../csrc/pose_refine_common.h", "../../include/sslam_weight.h", _HIP_H),
            _weight_prototypes),
    Library("track", "sslt", "csrc_track", "libsslam_track.so", "sslam_track.h", TRACK_EXPORTS, ("../../include/sslam_track.h", _HIP_H),
            _track_prototypes),
)}
SO_PATH = LIBRARIES["lib"].so_path      # where the first library is built; to load another file, set LIBRARIES["lib"].so_path


# The names the wrappers above and the rest of the tree call: the loader, the builder and the launch counter of each row.
def lib(): return LIBRARIES["lib"].load()                                                               # noqa: E704
def ext(): return LIBRARIES["ext"].load()                                                               # noqa: E704
def graph(): return LIBRARIES["graph"].load()                                                           # noqa: E704
def loop(): return LIBRARIES["loop"].load()                                                             # noqa: E704
def window(): return LIBRARIES["window"].load()                                                         # noqa: E704
def place(): return LIBRARIES["place"].load()                                                           # noqa: E704
def conf(): return LIBRARIES["conf"].load()                                                             # noqa: E704
def weight(): return LIBRARIES["weight"].load()                                                         # noqa: E704
def track(): return LIBRARIES["track"].load()                                                           # noqa: E704
def build(force: bool = False) -> str: return LIBRARIES["lib"].build(force)                             # noqa: E704
def ext_build(force: bool = False) -> str: return LIBRARIES["ext"].build(force)                         # noqa: E704
def graph_build(force: bool = False) -> str: return LIBRARIES["graph"].build(force)                     # noqa: E704
def loop_build(force: bool = False) -> str: return LIBRARIES["loop"].build(force)                       # noqa: E704
def window_build(force: bool = False) -> str: return LIBRARIES["window"].build(force)                   # noqa: E704
def place_build(force: bool = False) -> str: return LIBRARIES["place"].build(force)                     # noqa: E704
def conf_build(force: bool = False) -> str: return LIBRARIES["conf"].build(force)                       # noqa: E704
def weight_build(force: bool = False) -> str: return LIBRARIES["weight"].build(force)                   # noqa: E704
def track_build(force: bool = False) -> str: return LIBRARIES["track"].build(force)                     # noqa: E704
def launch_count() -> int: return LIBRARIES["lib"].launch_count()                                       # noqa: E704
def ext_launch_count() -> int: return LIBRARIES["ext"].launch_count()                                   # noqa: E704
def graph_launch_count() -> int: return LIBRARIES["graph"].launch_count()                               # noqa: E704
def loop_launch_count() -> int: return LIBRARIES["loop"].launch_count()                                 # noqa: E704
def window_launch_count() -> int: return LIBRARIES["window"].launch_count()                             # noqa: E704
def place_launch_count() -> int: return LIBRARIES["place"].launch_count()                               # noqa: E704
def conf_launch_count() -> int: return LIBRARIES["conf"].launch_count()                                 # noqa: E704
def weight_launch_count() -> int: return LIBRARIES["weight"].launch_count()                             # noqa: E704
def track_launch_count() -> int: return LIBRARIES["track"].launch_count()                               # noqa: E704
