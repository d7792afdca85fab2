"""The operand contract of libsslam_hip.so as a table: for every entry that takes device pointers, the least alignment in bytes of
each pointer argument and the names of its stride arguments - what the block "ALIGNMENT AND STRIDES" of include/sslam_hip.h
states, line for line (tests/test_loose_operands_table.py compares the two and holds the table against sslam_amd.lib.EXPORTS).
tests/test_gpu_loose_operands.py runs every row: each operand at its alignment and no better, each pointer once at half of it.

An alignment is the widest access the entry's kernels make to the argument (1: bytes, 2: bf16 / uint16, 4: fp32 / int32 words,
8: int64 / float64 / an (x, y) pair loaded as one, 16: four-word vectors), or the entry's older, stricter demand where it had one.
No torch, no GPU: importable anywhere.
"""

_TABLES = dict(bounds_h=4, coefs_h=4, bounds_v=4, coefs_v=4)
_BN = dict(tokens=16, gamma=16, beta=16, run_mean=16, run_var=16, out_feat=16, out_mean=16, out_var=16)
_SEL = dict(feat=16, w1_packed=16, b1=4, w2=4, b2=4, sal=4)
_GR = dict(feat=16, kp_xy=4, packed=16, desc=16)
_SIM = dict(desc1=16, desc2=16, nn12=4, s12=4, nn21=4, s21=4, second12=4)
_SIMP = dict(bank=16, pair_first=4, pair_second=4, nn12=4, s12=4, nn21=4, s21=4, second12=4)
_ROWS = dict(desc1=16, desc2=16, nn12=4, s12=4, second12=4)
_ROWSP = dict(bank=16, pair_first=4, pair_second=4, nn12=4, s12=4, second12=4)
_LSE = dict(desc1=16, desc2=16, s12=4, lse=4, ce=4, s00=4)
_LSEP = dict(bank=16, pair_first=4, pair_second=4, s12=4, lse=4, ce=4, s00=4)
_RULE = dict(nn12=4, s12=4, second12=4, nn21=4, matches=8, value=4, count=4)
_FSTATS = dict(saliency=4, pooled=4, edge_max=4, descriptors=4, stats=4, desc_mean=4, desc_m2=4)
_PSTATS = dict(nn12=4, nn21=4, s12=4, ce=4, s00=4, stats=4, n_matches=4)
_VIT = dict(workspace=16, tokens_out=16)
_NN_OUT = dict(gt_matches=8, gt_count=4, gt_of_row=4, dist_sum=8, dist_median=8)
_SCORE = dict(matches=8, value=4, count=4, gt_of_row=4, gt_count=4, tp=4, fp=4, fn=4, value_sum=8)
_POSE_IN = dict(kp_bank=8, kp_depth_bank=4, pair_first=4, pair_second=4, matches=8, count=4)

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "sslam_preprocess_u8": dict(img=1, **_TABLES, out_chw=4),
    "sslam_preprocess_u8_patches": dict(img=4, **_TABLES, out_patches_bf16=2),
    "sslam_keypoint_intensity": dict(img=1, **_TABLES, kp_pixel=4, out=4),
    "sslam_bn_tokens": dict(_BN),
    "sslam_bn_tokens_bf16copy": dict(_BN, out_feat_bf16=16),
    "sslam_selector_saliency": dict(_SEL),
    "sslam_selector_saliency_ws": dict(_SEL, workspace=16),
    "sslam_f32_to_bf16": {"in": 16, "out_bf16": 16},
    "sslam_selector_saliency_bf16": dict(feat_bf16=16, w1_packed_bf16=16, b1=4, w2=4, b2=4, sal=4),
    "sslam_select_keypoints": dict(sal=4, kp_xy=4, scores=4, idx=4, kp_pixel=4, status=4),
    "sslam_gather": dict(feat=16, kp_xy=4, out=16),
    "sslam_refine": dict(x=16, packed=16, desc=16),
    "sslam_refine_d": dict(x=16, packed=16, desc=16),
    "sslam_gather_refine": dict(_GR),
    "sslam_gather_refine_d": dict(_GR),
    "sslam_gather_refine_ws": dict(_GR, workspace=4),
    "sslam_gather_refine_ws_d": dict(_GR, workspace=4),
    "sslam_refine_bf16": dict(x=16, packed_bf16=16, desc=4),
    "sslam_gather_refine_bf16": dict(feat=16, kp_xy=4, packed_bf16=16, desc=4),
    "sslam_sim_argmax": dict(_SIM),
    "sslam_sim_argmax_d": dict(_SIM),
    "sslam_sim_argmax_ws": dict(_SIM, workspace=8),
    "sslam_sim_argmax_ws_d": dict(_SIM, workspace=8),
    "sslam_sim_argmax_pairs": dict(_SIMP, workspace=8),
    "sslam_sim_argmax_pairs_d": dict(_SIMP, workspace=8),
    "sslam_sim_argmax_rows": dict(_ROWS),
    "sslam_sim_argmax_rows_d": dict(_ROWS),
    "sslam_sim_argmax_rows_pairs": dict(_ROWSP),
    "sslam_sim_argmax_rows_pairs_d": dict(_ROWSP),
    "sslam_match_finalize": dict(nn12=4, s12=4, nn21=4, scores1=4, scores2=4, intensity1=4, intensity2=4, matches=8, quality=4, count=4),
    "sslam_match_finalize_pairs": dict(nn12=4, s12=4, nn21=4, pair_first=4, pair_second=4, scores_bank=4, intensity_bank=4, matches=8,
                                       quality=4, count=4),
    "sslam_match_finalize_rule": dict(_RULE),
    "sslam_match_finalize_rule_pairs": dict(_RULE, pair_first=4, pair_second=4),
    "sslam_match_rank": dict(matches=8, value=4, count=4, out_matches=8, out_value=4, out_count=4, out_slot=4),
    "sslam_row_lse": dict(_LSE),
    "sslam_row_lse_d": dict(_LSE),
    "sslam_row_lse_pairs": dict(_LSEP),
    "sslam_row_lse_pairs_d": dict(_LSEP),
    "sslam_edge_pool": dict(images_chw=16, pooled=4, edge_max=4),
    "sslam_val_frame_stats": dict(_FSTATS),
    "sslam_val_frame_stats_d": dict(_FSTATS),
    "sslam_val_pair_stats": dict(saliency1=4, saliency2=4, **_PSTATS),
    "sslam_val_pair_stats_pairs": dict(saliency_bank=4, pair_first=4, pair_second=4, **_PSTATS),
    "sslam_vit_forward": dict(images_chw=16, **_VIT),
    "sslam_vit_forward_form": dict(images_chw=16, **_VIT),
    "sslam_vit_forward_patches": dict(patches_bf16=16, **_VIT),
    "sslam_vit_forward_patches_form": dict(patches_bf16=16, **_VIT),
    "sslam_vit_forward_f32": dict(images_chw=16, **_VIT),
    "sslam_vit_forward_f32_form": dict(images_chw=16, **_VIT),
    "sslam_pose_nn_pairs": dict(kp_bank=8, pair_first=4, pair_second=4, H=8, **_NN_OUT),
    "sslam_match_score_pairs": dict(_SCORE),
    "sslam_keypoint_depth": dict(depth=2, kp_pixel=8, kp_depth=4),
    "sslam_pose_depth_nn_pairs": dict(kp_bank=8, kp_depth_bank=4, pair_first=4, pair_second=4, T=8, valid_count=4, **_NN_OUT),
    "sslam_match_score_known_pairs": dict(_SCORE, unknown=4),
    "sslam_pose_ransac_pairs": dict(_POSE_IN, T=8, inlier_count=4, usable_count=4, best_hypothesis=4, refit_kept=4, inlier_of_slot=4, rms=8),
    "sslam_pose_refine_pairs": dict(_POSE_IN, T_in=8, T=8, status=4, iterations=4, selected_count=4, usable_count=4, inlier_count_in=4,
                                    inlier_count=4, inlier_of_slot=4, cost_in=8, cost=8, rms=8, info=8),
}

# the one argument whose misalignment is answered with another code: the tiled kernel of the patch entry serves a dword-aligned image
# only, and the caller then takes sslam_preprocess_u8 + sslam_vit_forward (include/sslam_hip.h)
REFUSED_AS_UNSUPPORTED = {("sslam_preprocess_u8_patches", "img")}

# entry -> its stride arguments (in floats).  Descriptor strides: any multiple of 4 floats, of either sign, 0 included; score
# strides: any value.  include/sslam_hip.h says what a stride means.
_DESC, _BANK = ("stride1", "stride2"), ("frame_stride",)
STRIDES = {
    **{name: _DESC for name in ("sslam_sim_argmax", "sslam_sim_argmax_d", "sslam_sim_argmax_ws", "sslam_sim_argmax_ws_d", "sslam_sim_argmax_rows",
                                "sslam_sim_argmax_rows_d", "sslam_row_lse", "sslam_row_lse_d")},
    **{name: _BANK for name in ("sslam_sim_argmax_pairs", "sslam_sim_argmax_pairs_d", "sslam_sim_argmax_rows_pairs",
                                "sslam_sim_argmax_rows_pairs_d", "sslam_row_lse_pairs", "sslam_row_lse_pairs_d")},
    "sslam_match_finalize": ("sstride1", "sstride2"),
    "sslam_match_finalize_pairs": ("score_stride",),
}
DESCRIPTOR_STRIDES = ("stride1", "stride2", "frame_stride")          # multiples of 4 floats; the score strides are free

# the entries that take no device pointer: host-side packers, layouts, sizes, the version and the test knob
HOST_ONLY = [
    "sslam_version", "sslam_arch", "sslam_launch_count",
    "sslam_pack_conv3x3_host", "sslam_pack_linear_host", "sslam_refiner_pack_host", "sslam_refiner_pack_host_d", "sslam_vit_pack_linear_host",
    "sslam_vit_pack_mlp_host", "sslam_pack_conv3x3_bf16_host", "sslam_refiner_pack_bf16_host", "sslam_vit_f32_pack_linear_host",
    "sslam_resample_table_host",
    "sslam_refiner_layout", "sslam_refiner_layout_d",
    "sslam_vit_workspace_bytes", "sslam_vit_workspace_bytes_form", "sslam_vit_f32_workspace_bytes", "sslam_selector_saliency_workspace_bytes",
    "sslam_sim_argmax_workspace_bytes", "sslam_gather_refine_workspace_bytes", "sslam_refiner_bf16_bytes", "sslam_workspace_bytes",
    "sslam_selector_bf16_halo_groups", "sslam_test_set_knob",
]


def header_lines():
    """The table as the lines of the header's block: `entry: arg a, arg a, ...[; strides: s, s]`."""
    out = []
    for entry, args in ALIGN.items():
        line = f"{entry}: " + ", ".join(f"{k} {v}" for k, v in args.items())
        if entry in STRIDES:
            line += "; strides: " + ", ".join(STRIDES[entry])
        out.append(line)
    return out


def is_host_only_name(name):
    """The only kinds of entry HOST_ONLY may hold (the issue's list)."""
    return (name in ("sslam_version", "sslam_arch", "sslam_launch_count", "sslam_resample_table_host", "sslam_workspace_bytes",
                     "sslam_selector_bf16_halo_groups", "sslam_test_set_knob")
            or name.endswith("_host") or "_host_" in name or "_layout" in name or "_workspace_bytes" in name or name.endswith("_bytes"))
