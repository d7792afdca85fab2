"""The size contract of libsslam_hip.so and libsslam_ext.so as a table: for every entry that launches a kernel, the counts or byte
sizes it accepts - as the expression its dispatch code tests -, what it returns above them, where it cuts a call into launch
groups by itself rather than refusing, and the widths in bits of the offset expressions in its kernels (31: a signed int that
must stay non-negative, 32: an unsigned 32-bit byte offset into one buffer descriptor, 64: long long / size_t / pointer
arithmetic).  It is what the block "SIZE LIMITS" of include/sslam_hip.h (and of include/sslam_ext.h) states, line for line;
tests/test_size_limits_cpu.py compares the two, holds the table against sslam_amd.lib.EXPORTS and calls every entry one above
each limit; tests/test_gpu_size_limits.py runs the accepted side with operands past 2^31 bytes.  profiles/size_limits.txt is the
audit the widths come from.  No torch, no GPU: importable anywhere.
"""
import loose_table as lt

E_UNSUPPORTED = -2
U31, U32F, U32 = 0x7fffffff, 0xfffffff0, 0xffffffff
C_FEAT, QB, VIT_MLP, VIT_PREFIX = 384, 128, 1536, 5


# ---- A0: the one entry pair that cuts a call into launch groups by itself
def a0_frame_bytes(h, w):
    return h * w * 3


def a0_per_group(h, w):
    """Frames per launch group of preprocess_launch: grid.z <= 65535 and all byte offsets of a group inside one 32-bit descriptor;
    frame sizes that are no multiple of 4 bytes are cut at multiples of 4 frames, which keeps every group's base dword aligned."""
    fb = a0_frame_bytes(h, w)
    g = min(65535, max(1, U32F // fb))
    if fb & 3 and g >= 4:
        g &= ~3
    return g


def a0_tiles(h, w, size, ksize_v):
    """Tiles per frame of the tiled kernel: 64 columns by 32 rows where the input rows of a 32-row tile fit its LDS buffer, else 16."""
    gx = (size + 63) // 64
    tall = (32 * h + size - 1) // size + ksize_v + 2 <= 64
    return gx * ((size + 31) // 32), gx * ((size + 15) // 16), tall


def a0_workgroups(n, h, w, size, ksize_v):
    """The larger of the two workgroup counts the dispatch code holds against 2^31 - 1, over the groups of an n-frame call."""
    ng = min(n, a0_per_group(h, w))
    tt, ts, _ = a0_tiles(h, w, size, ksize_v)
    return (ng + 7) // 8 * 8 * max(tt, ts)


def a9_fast(n, h, w, K, ksize_h, ksize_v, aligned=True):
    """Whether sslam_keypoint_intensity takes intensity_fast_kernel (32-bit offsets); it falls back to intensity_kernel otherwise."""
    return ksize_h <= 7 and ksize_v <= 7 and aligned and n * h * w * 3 <= U32F and n * K <= 0x7fffff00


def _qblocks(n):
    return (n + QB - 1) // QB


# entry -> row.  limits: (expression the dispatch code tests, return code where it is false).  largest: the call's shape -> the largest
# accepted value of `count`.  cuts: what the entry does instead of refusing.  widths: offset expression -> bits.
_A0 = dict(
    count="h * w * 3",
    limits=[("h * w * 3 <= 0x7fffffff", E_UNSUPPORTED),
            ("(min(n, per_group) + 7) / 8 * 8 * tiles <= 0x7fffffff", E_UNSUPPORTED)],
    largest=lambda **s: U31,
    cuts="n: any; cut into launch groups of per_group = min(65535, max(1, 0xfffffff0 / (h * w * 3))) frames, rounded down to a "
         "multiple of 4 where h * w * 3 is none and per_group >= 4; a group whose base is not dword aligned takes the general kernel",
    widths={"tiled kernel: frame * (h * w * 3) + (row * w + col) * 3 into the group's descriptor": 32,
            "tiled kernel: output frame * 3 * size^2": 64, "general kernel: frame * h * w * 3": 64, "group base n0 * h * w * 3": 64})
_BN = dict(
    count="group * cells", limits=[("group * (tokens_per_frame - n_prefix) <= 0x7fffffff - 112", E_UNSUPPORTED)],
    largest=lambda **s: U31 - 112,
    widths={"sweep kernel: row of the group r + 16 * u, u < 7": 31, "sweep kernel: (frame * tokens_per_frame + token) * 384": 64,
            "register kernel: lane offset loff = p * 384 + ch0": 32, "register kernel: frame * tokens_per_frame * 384 + step * 16 * 384": 64})
_SEL = dict(
    count="n_frames", limits=[("n_frames * G * G * 1536 <= 0xffffffff", E_UNSUPPORTED)],
    largest=lambda G, **s: U32 // (G * G * C_FEAT * 4),
    widths={"cell * 1536 + 32 * k-group into one descriptor over feat": 32, "(int)rows, cell and padded-cell indices": 31, "sal[cell]": 64})
_SELBF = dict(
    count="n_frames", limits=[("n_frames * G * G * 768 <= 0xffffffff", E_UNSUPPORTED)],
    largest=lambda G, **s: U32 // (G * G * C_FEAT * 2),
    widths={"cell * 768 + 16 * k-group into one descriptor over feat_bf16": 32,
            "(int)rows, cell and padded-cell indices (the halo form runs below 2^30 cells only)": 31, "sal[cell]": 64})
_SIM = dict(
    count="n_pairs", limits=[("n_pairs * ceil(max(n1, n2) / 128) <= 0x7ffffff0 / 8", E_UNSUPPORTED)],
    largest=lambda n1, n2=0, **s: (0x7ffffff0 // 8) // _qblocks(max(n1, n2)),
    widths={"workgroup = 8 * (slot / qblocks) + xcd in one grid dimension": 31, "pair * stride, frame * frame_stride, row * D": 64,
            "keys[pair * n2 + column]": 64})
_ROWS = dict(
    count="n_pairs", limits=[("n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8", E_UNSUPPORTED)],
    largest=lambda n1, **s: (0x7ffffff0 // 8) // _qblocks(n1),
    widths={"workgroup = 8 * (slot / qblocks) + xcd in one grid dimension": 31, "pair * stride, frame * frame_stride, row * D": 64})
_VIT = dict(
    count="n_frames", limits=[("n_frames * T * 1536 <= 0x7fffffff * 64, T = (size / 16)^2 + 5", E_UNSUPPORTED)],
    largest=lambda size, **s: (U31 * 64) // (((size // 16) ** 2 + VIT_PREFIX) * VIT_MLP),
    widths={"rows * VMLP in the GEMM tile index (rows * 1536 / 64 stays below 2^31)": 31, "workspace carving, token rows": 64},
    out_of_reach="crosses 2^31 only from 89 478 486 token rows: a bf16 hidden activation of 275 GB, far above 24 GiB of one operand")
_VITF = dict(
    count="n_frames", limits=[("n_frames * T * 1536 * 4 <= 0xfffffff0, T = (size / 16)^2 + 5", E_UNSUPPORTED)],
    largest=lambda size, **s: U32F // (((size // 16) ** 2 + VIT_PREFIX) * VIT_MLP * 4),
    widths={"GEMM A operand: row * lda * 4 into one descriptor (widest: the MLP hidden activation)": 32, "workspace carving, token rows": 64})
_PER_PAIR = "indexes in 64 bits; one workgroup per pair"
_PER_FRAME = "indexes in 64 bits; one workgroup per frame"
_K4096 = [("K <= 4096 (n1 <= 4096)", E_UNSUPPORTED)]

LIMITS = {
    "sslam_preprocess_u8": _A0,
    "sslam_preprocess_u8_patches": dict(_A0, cuts=_A0["cuts"].replace("takes the general kernel", "is refused with SSLAM_E_UNSUPPORTED, as is a table of more than 7 "
                                                                      "horizontal taps (the caller takes sslam_preprocess_u8 then)")),
    "sslam_bn_tokens": _BN,
    "sslam_bn_tokens_bf16copy": _BN,
    "sslam_selector_saliency": _SEL,
    "sslam_selector_saliency_ws": _SEL,
    "sslam_selector_saliency_bf16": _SELBF,
    **{name: _SIM for name in ("sslam_sim_argmax", "sslam_sim_argmax_d", "sslam_sim_argmax_ws", "sslam_sim_argmax_ws_d",
                               "sslam_sim_argmax_pairs", "sslam_sim_argmax_pairs_d")},
    **{name: _ROWS for name in ("sslam_sim_argmax_rows", "sslam_sim_argmax_rows_d", "sslam_sim_argmax_rows_pairs", "sslam_sim_argmax_rows_pairs_d",
                                "sslam_row_lse", "sslam_row_lse_d", "sslam_row_lse_pairs", "sslam_row_lse_pairs_d")},
    "sslam_edge_pool": dict(count="n_frames", limits=[("n_frames <= 65535", E_UNSUPPORTED), ("size / 16 <= 65535", E_UNSUPPORTED)],
                            largest=lambda **s: 65535, widths={"grid.z = n_frames, grid.y = size / 16": 31, "frame * 3 * size^2": 64}),
    **{name: _VIT for name in ("sslam_vit_forward", "sslam_vit_forward_form", "sslam_vit_forward_patches", "sslam_vit_forward_patches_form")},
    "sslam_vit_forward_f32": _VITF,
    "sslam_vit_forward_f32_form": _VITF,
    "sslam_keypoint_depth": dict(count="n", limits=[("n * K <= 0x7fffffff", E_UNSUPPORTED)], largest=lambda K, **s: U31 // K,
                                 widths={"keypoint index n * K": 64, "frame * h * w": 64}),
    "sslam_select_keypoints": dict(count="G * G", limits=[("G * G <= 4096 and K <= 4096", E_UNSUPPORTED)], largest=lambda **s: 4096,
                                   widths={"frame * G * G, frame * K": 64}, frames=_PER_FRAME),
    "sslam_match_rank": dict(count="n1", limits=[("n1 <= 4096", E_UNSUPPORTED)], largest=lambda **s: 4096, widths={"pair * n1": 64}, frames=_PER_PAIR),
    **{name: dict(count="K", limits=_K4096, largest=lambda **s: 4096, widths={"frame * K, pair * n1": 64}, frames=_PER_PAIR)
       for name in ("sslam_pose_nn_pairs", "sslam_pose_depth_nn_pairs", "sslam_pose_ransac_pairs", "sslam_pose_refine_pairs")},
    **{name: dict(count="n1", limits=[("n1 <= 4096", E_UNSUPPORTED)], largest=lambda **s: 4096, widths={"pair * n1": 64}, frames=_PER_PAIR)
       for name in ("sslam_match_score_pairs", "sslam_match_score_known_pairs")},
}

# the entries that launch kernels and state no size limit: what keeps them right at any size that fits in memory
NO_LIMIT = {
    "sslam_keypoint_intensity": "never refuses by size: above 0xfffffff0 bytes of frames or 0x7fffff00 keypoints (or with more than 7 taps either "
                                "way, or an img that is not dword aligned) it falls back from intensity_fast_kernel (32-bit offsets into one "
                                "descriptor) to intensity_kernel (64 bits); one thread per keypoint",
    "sslam_f32_to_bf16": "indexes in 64 bits; one thread per 8 elements",
    "sslam_gather": "indexes in 64 bits; one thread per four floats of a row",
    **{name: "indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are int32: it runs below 2^31 rows only, "
             "the direct form above)" for name in ("sslam_refine", "sslam_refine_d", "sslam_gather_refine", "sslam_gather_refine_d",
                                                   "sslam_gather_refine_ws", "sslam_gather_refine_ws_d", "sslam_refine_bf16", "sslam_gather_refine_bf16")},
    **{name: _PER_PAIR for name in ("sslam_match_finalize", "sslam_match_finalize_pairs", "sslam_match_finalize_rule", "sslam_match_finalize_rule_pairs",
                                    "sslam_val_pair_stats", "sslam_val_pair_stats_pairs")},
    **{name: _PER_FRAME for name in ("sslam_val_frame_stats", "sslam_val_frame_stats_d")},
}

EXT_LIMITS = {
    "sslx_subcell_keypoints": dict(count="n_frames", limits=[("n_frames * K <= 0x7fffffff", E_UNSUPPORTED), ("G <= 64 and K <= 4096", E_UNSUPPORTED)],
                                   largest=lambda K, **s: U31 // K, widths={"keypoint index n_frames * K": 64, "frame * G * G": 64}),
}
EXT_NO_LIMIT = {"sslx_version": "takes no device operand", "sslx_arch": "takes no device operand", "sslx_launch_count": "takes no device operand"}

HOST_ONLY = list(lt.HOST_ONLY)          # packers, layouts, sizes, the version and the knob: no device operand, no kernel


def _line(entry, row):
    parts = ["; ".join(f"{expr}, else {'SSLAM_E_UNSUPPORTED' if code == E_UNSUPPORTED else code}" for expr, code in row["limits"])]
    if row.get("cuts"):
        parts.append(row["cuts"])
    if row.get("frames"):
        parts.append(row["frames"])
    parts.append("offsets: " + ", ".join(f"{k} {v}" for k, v in row["widths"].items()))
    if row.get("out_of_reach"):
        parts.append("untested - " + row["out_of_reach"])
    return f"{entry}: " + ". ".join(parts)


def header_lines(ext=False):
    """The table as the lines of the header's block."""
    rows, free = (EXT_LIMITS, {}) if ext else (LIMITS, NO_LIMIT)
    return [_line(e, r) for e, r in rows.items()] + [f"{e}: no limit - {why}" for e, why in free.items()]
