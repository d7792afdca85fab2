/*
 * sslam_hip.h - C ABI of libsslam_hip.so: the MI355X (gfx950) implementation of the semantic-slam per-frame
 * feature-extraction + descriptor-matching hot path.
 *
 * The reference (Siverteh/semantic-slam-master) is pure Python: there is no FFI / plugin layer to mirror, so this
 * header defines the boundary a maintainer binds with ctypes (INTEGRATION.md shows the stub).  One entry per fused
 * stage; each cites the reference code it replaces (paths relative to the reference repo).
 *
 * Conventions (all entries):
 *   - every pointer is a CALLER-OWNED DEVICE pointer unless the name ends in _host; the library never copies to
 *     the host and NEVER allocates or frees device memory.  The three entries whose fastest form needs scratch take it
 *     from the caller (sslam_selector_saliency_ws, sslam_gather_refine_ws, sslam_sim_argmax_ws and its pair-list form sslam_sim_argmax_pairs; sizes from sslam_workspace_bytes or the
 *     per-entry *_workspace_bytes); their forms without a workspace argument run a scratch-free launch shape with
 *     the same bits;
 *   - `stream` is a hipStream_t passed as void* (PyTorch: torch.cuda.current_stream().cuda_stream); calls only
 *     enqueue work - no synchronisation, no host read-back;
 *   - return value: SSLAM_OK or a negative SSLAM_E_* code; launch failures are reported via hipGetLastError;
 *   - stateless and thread-safe given distinct streams / workspaces.  The SSLAM_* environment variables named below
 *     are TEST-ONLY knobs (A/B timing, forcing a launch form in the parity tests): the environment is read once,
 *     when the library is loaded, never per call; every form they select produces the same bits;
 *   - all floating point is IEEE fp32 evaluated in the canonical order documented in oracle/sslam_oracle.h
 *     (contractions = one fused-multiply-add chain in increasing k on v_mfma_f32_32x32x2_f32), so results are
 *     bit-identical to the CPU oracle.
 */
#ifndef SSLAM_HIP_H
#define SSLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSLAM_OK 0
#define SSLAM_E_INVALID (-1)     /* null pointer / non-positive size / misaligned pointer (ALIGNMENT AND STRIDES below) */
#define SSLAM_E_UNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define SSLAM_E_LAUNCH (-3)      /* hipGetLastError() != hipSuccess after the launch */

/* ---- ALIGNMENT AND STRIDES, every entry that takes device pointers.  An entry's result is a function of its operands' VALUES, not
 * of their addresses: it is the same bits wherever the operands lie, down to the alignments below and at every stride named here
 * (tests/test_gpu_loose_operands.py runs each entry with every operand at its least alignment, just past and just before a
 * 256-byte boundary, and with padded, zero and negative strides).
 * Below, per entry, the LEAST alignment in bytes of each pointer argument: the widest access the entry's kernels make to it - 1 a
 * byte, 2 a bf16 or uint16, 4 an fp32 or int32 word, 8 an int64, a float64 or an (x, y) pair loaded as one, 16 a four-word vector -
 * or the stricter demand the entry has always made (sslam_bn_tokens wants 16 throughout).  A pointer that misses its alignment:
 * SSLAM_E_INVALID before anything is launched, nothing written.  An optional pointer that is NULL is aligned.  Arguments that are
 * frame slices of a larger array need no more than this: a caller may hand `scores + f * K` or `sal + f * G * G` for any f, K, G.
 * A workspace is aligned like any other argument and a misaligned one is refused, not ignored.  The img of sslam_preprocess_u8 and
 * sslam_keypoint_intensity may lie anywhere; sslam_preprocess_u8_patches serves a dword-aligned one only and answers any other with
 * SSLAM_E_UNSUPPORTED, not SSLAM_E_INVALID, as for a resampling ratio it does not cover: the caller takes sslam_preprocess_u8 then.
 * The pointers INSIDE sslam_vit_weights_t / sslam_vit_weights_f32_t are not checked: 16-byte aligned, every one.
 * STRIDES are signed 64-bit counts of floats, named after the semicolon.  Pair p (or frame f of a bank) starts at
 * base + p * stride in plain pointer arithmetic, so: stride 0 broadcasts one frame to every pair; a stride above rows * width
 * leaves a gap the kernels never read; a stride below it makes frames overlap (rows are only read); a NEGATIVE stride is
 * accepted and walks backwards from the base - the caller hands the address of pair 0 and owns every frame the call reaches.
 * stride1, stride2 and frame_stride must be multiples of 4 floats (every frame then keeps the base's 16-byte alignment), else
 * SSLAM_E_INVALID; they need not be multiples of the row width.  sstride1, sstride2 and score_stride may be any value.
 *   sslam_preprocess_u8: img 1, bounds_h 4, coefs_h 4, bounds_v 4, coefs_v 4, out_chw 4
 *   sslam_preprocess_u8_patches: img 4, bounds_h 4, coefs_h 4, bounds_v 4, coefs_v 4, out_patches_bf16 2
 *   sslam_keypoint_intensity: img 1, bounds_h 4, coefs_h 4, bounds_v 4, coefs_v 4, kp_pixel 4, out 4
 *   sslam_bn_tokens: tokens 16, gamma 16, beta 16, run_mean 16, run_var 16, out_feat 16, out_mean 16, out_var 16
 *   sslam_bn_tokens_bf16copy: tokens 16, gamma 16, beta 16, run_mean 16, run_var 16, out_feat 16, out_mean 16, out_var 16,
 *         out_feat_bf16 16
 *   sslam_selector_saliency: feat 16, w1_packed 16, b1 4, w2 4, b2 4, sal 4
 *   sslam_selector_saliency_ws: feat 16, w1_packed 16, b1 4, w2 4, b2 4, sal 4, workspace 16
 *   sslam_f32_to_bf16: in 16, out_bf16 16
 *   sslam_selector_saliency_bf16: feat_bf16 16, w1_packed_bf16 16, b1 4, w2 4, b2 4, sal 4
 *   sslam_select_keypoints: sal 4, kp_xy 4, scores 4, idx 4, kp_pixel 4, status 4
 *   sslam_gather: feat 16, kp_xy 4, out 16
 *   sslam_refine: x 16, packed 16, desc 16
 *   sslam_refine_d: x 16, packed 16, desc 16
 *   sslam_gather_refine: feat 16, kp_xy 4, packed 16, desc 16
 *   sslam_gather_refine_d: feat 16, kp_xy 4, packed 16, desc 16
 *   sslam_gather_refine_ws: feat 16, kp_xy 4, packed 16, desc 16, workspace 4
 *   sslam_gather_refine_ws_d: feat 16, kp_xy 4, packed 16, desc 16, workspace 4
 *   sslam_refine_bf16: x 16, packed_bf16 16, desc 4
 *   sslam_gather_refine_bf16: feat 16, kp_xy 4, packed_bf16 16, desc 4
 *   sslam_sim_argmax: desc1 16, desc2 16, nn12 4, s12 4, nn21 4, s21 4, second12 4; strides: stride1, stride2
 *   sslam_sim_argmax_d: desc1 16, desc2 16, nn12 4, s12 4, nn21 4, s21 4, second12 4; strides: stride1, stride2
 *   sslam_sim_argmax_ws: desc1 16, desc2 16, nn12 4, s12 4, nn21 4, s21 4, second12 4, workspace 8; strides: stride1, stride2
 *   sslam_sim_argmax_ws_d: desc1 16, desc2 16, nn12 4, s12 4, nn21 4, s21 4, second12 4, workspace 8; strides: stride1, stride2
 *   sslam_sim_argmax_pairs: bank 16, pair_first 4, pair_second 4, nn12 4, s12 4, nn21 4, s21 4, second12 4, workspace 8;
 *         strides: frame_stride
 *   sslam_sim_argmax_pairs_d: bank 16, pair_first 4, pair_second 4, nn12 4, s12 4, nn21 4, s21 4, second12 4, workspace 8;
 *         strides: frame_stride
 *   sslam_sim_argmax_rows: desc1 16, desc2 16, nn12 4, s12 4, second12 4; strides: stride1, stride2
 *   sslam_sim_argmax_rows_d: desc1 16, desc2 16, nn12 4, s12 4, second12 4; strides: stride1, stride2
 *   sslam_sim_argmax_rows_pairs: bank 16, pair_first 4, pair_second 4, nn12 4, s12 4, second12 4; strides: frame_stride
 *   sslam_sim_argmax_rows_pairs_d: bank 16, pair_first 4, pair_second 4, nn12 4, s12 4, second12 4; strides: frame_stride
 *   sslam_match_finalize: nn12 4, s12 4, nn21 4, scores1 4, scores2 4, intensity1 4, intensity2 4, matches 8, quality 4, count
 *         4; strides: sstride1, sstride2
 *   sslam_match_finalize_pairs: nn12 4, s12 4, nn21 4, pair_first 4, pair_second 4, scores_bank 4, intensity_bank 4, matches 8,
 *         quality 4, count 4; strides: score_stride
 *   sslam_match_finalize_rule: nn12 4, s12 4, second12 4, nn21 4, matches 8, value 4, count 4
 *   sslam_match_finalize_rule_pairs: nn12 4, s12 4, second12 4, nn21 4, matches 8, value 4, count 4, pair_first 4, pair_second 4
 *   sslam_match_rank: matches 8, value 4, count 4, out_matches 8, out_value 4, out_count 4, out_slot 4
 *   sslam_row_lse: desc1 16, desc2 16, s12 4, lse 4, ce 4, s00 4; strides: stride1, stride2
 *   sslam_row_lse_d: desc1 16, desc2 16, s12 4, lse 4, ce 4, s00 4; strides: stride1, stride2
 *   sslam_row_lse_pairs: bank 16, pair_first 4, pair_second 4, s12 4, lse 4, ce 4, s00 4; strides: frame_stride
 *   sslam_row_lse_pairs_d: bank 16, pair_first 4, pair_second 4, s12 4, lse 4, ce 4, s00 4; strides: frame_stride
 *   sslam_edge_pool: images_chw 16, pooled 4, edge_max 4
 *   sslam_val_frame_stats: saliency 4, pooled 4, edge_max 4, descriptors 4, stats 4, desc_mean 4, desc_m2 4
 *   sslam_val_frame_stats_d: saliency 4, pooled 4, edge_max 4, descriptors 4, stats 4, desc_mean 4, desc_m2 4
 *   sslam_val_pair_stats: saliency1 4, saliency2 4, nn12 4, nn21 4, s12 4, ce 4, s00 4, stats 4, n_matches 4
 *   sslam_val_pair_stats_pairs: saliency_bank 4, pair_first 4, pair_second 4, nn12 4, nn21 4, s12 4, ce 4, s00 4, stats 4,
 *         n_matches 4
 *   sslam_vit_forward: images_chw 16, workspace 16, tokens_out 16
 *   sslam_vit_forward_form: images_chw 16, workspace 16, tokens_out 16
 *   sslam_vit_forward_patches: patches_bf16 16, workspace 16, tokens_out 16
 *   sslam_vit_forward_patches_form: patches_bf16 16, workspace 16, tokens_out 16
 *   sslam_vit_forward_f32: images_chw 16, workspace 16, tokens_out 16
 *   sslam_vit_forward_f32_form: images_chw 16, workspace 16, tokens_out 16
 *   sslam_pose_nn_pairs: kp_bank 8, pair_first 4, pair_second 4, H 8, gt_matches 8, gt_count 4, gt_of_row 4, dist_sum 8,
 *         dist_median 8
 *   sslam_match_score_pairs: matches 8, value 4, count 4, gt_of_row 4, gt_count 4, tp 4, fp 4, fn 4, value_sum 8
 *   sslam_keypoint_depth: depth 2, kp_pixel 8, kp_depth 4
 *   sslam_pose_depth_nn_pairs: kp_bank 8, kp_depth_bank 4, pair_first 4, pair_second 4, T 8, valid_count 4, gt_matches 8,
 *         gt_count 4, gt_of_row 4, dist_sum 8, dist_median 8
 *   sslam_match_score_known_pairs: matches 8, value 4, count 4, gt_of_row 4, gt_count 4, tp 4, fp 4, fn 4, value_sum 8, unknown
 *         4
 *   sslam_pose_ransac_pairs: kp_bank 8, kp_depth_bank 4, pair_first 4, pair_second 4, matches 8, count 4, T 8, inlier_count 4,
 *         usable_count 4, best_hypothesis 4, refit_kept 4, inlier_of_slot 4, rms 8
 *   sslam_pose_refine_pairs: kp_bank 8, kp_depth_bank 4, pair_first 4, pair_second 4, matches 8, count 4, T_in 8, T 8, status 4,
 *         iterations 4, selected_count 4, usable_count 4, inlier_count_in 4, inlier_count 4, inlier_of_slot 4, cost_in 8, cost
 *         8, rms 8, info 8 */

/* ---- SIZE LIMITS, every entry that launches a kernel.  An entry is correct over the whole range it accepts and refuses one past it:
 * below, per entry, the counts or byte sizes it accepts as the expression its dispatch code tests, and what it returns where the
 * expression is false - before anything is launched, nothing written.  Where an entry cuts a call into launch groups by itself
 * instead of refusing (sslam_preprocess_u8 and its patch form only), the line says how; every other entry leaves the cutting to
 * its caller (sslam_amd.pipeline: ExtractorConfig.launch_group(), HipViT / HipViTF32.chunk_frames).  "offsets:" names the offset and
 * index expressions of the entry's kernels with their width in bits - 31: a signed int that must stay non-negative, 32: an
 * unsigned byte offset into one buffer descriptor, 64: long long, size_t or pointer arithmetic (profiles/size_limits.txt is the
 * audit they are read from).  An entry with "no limit" indexes in 64 bits throughout and launches one workgroup or thread per
 * frame, pair or row; what bounds it is the memory its operands take.  Shape limits stated with an entry (K, n1 <= 4096; G * G <=
 * 4096; the descriptor widths 128 and 256; SSLAM_MAX_TAPS) are repeated here only where they are the entry's size limit.
 * tests/size_table.py holds this block as data; tests/test_size_limits_cpu.py calls every entry one above each limit, and
 * tests/test_gpu_size_limits.py runs the accepted side with operands past 2^31 bytes, bit for bit against the CPU oracle.
 *   sslam_preprocess_u8: h * w * 3 <= 0x7fffffff, else SSLAM_E_UNSUPPORTED; (min(n, per_group) + 7) / 8 * 8 * tiles <= 0x7fffffff,
 *         else SSLAM_E_UNSUPPORTED. n: any; cut into launch groups of per_group = min(65535, max(1, 0xfffffff0 / (h * w * 3)))
 *         frames, rounded down to a multiple of 4 where h * w * 3 is none and per_group >= 4; a group whose base is not dword
 *         aligned takes the general kernel. offsets: tiled kernel: frame * (h * w * 3) + (row * w + col) * 3 into the group's
 *         descriptor 32, tiled kernel: output frame * 3 * size^2 64, general kernel: frame * h * w * 3 64, group base n0 * h * w *
 *         3 64
 *   sslam_preprocess_u8_patches: h * w * 3 <= 0x7fffffff, else SSLAM_E_UNSUPPORTED; (min(n, per_group) + 7) / 8 * 8 * tiles <=
 *         0x7fffffff, else SSLAM_E_UNSUPPORTED. n: any; cut into launch groups of per_group = min(65535, max(1, 0xfffffff0 / (h *
 *         w * 3))) frames, rounded down to a multiple of 4 where h * w * 3 is none and per_group >= 4; a group whose base is not
 *         dword aligned is refused with SSLAM_E_UNSUPPORTED, as is a table of more than 7 horizontal taps (the caller takes
 *         sslam_preprocess_u8 then). offsets: tiled kernel: frame * (h * w * 3) + (row * w + col) * 3 into the group's descriptor
 *         32, tiled kernel: output frame * 3 * size^2 64, general kernel: frame * h * w * 3 64, group base n0 * h * w * 3 64
 *   sslam_bn_tokens: group * (tokens_per_frame - n_prefix) <= 0x7fffffff - 112, else SSLAM_E_UNSUPPORTED. offsets: sweep kernel:
 *         row of the group r + 16 * u, u < 7 31, sweep kernel: (frame * tokens_per_frame + token) * 384 64, register kernel: lane
 *         offset loff = p * 384 + ch0 32, register kernel: frame * tokens_per_frame * 384 + step * 16 * 384 64
 *   sslam_bn_tokens_bf16copy: group * (tokens_per_frame - n_prefix) <= 0x7fffffff - 112, else SSLAM_E_UNSUPPORTED. offsets: sweep
 *         kernel: row of the group r + 16 * u, u < 7 31, sweep kernel: (frame * tokens_per_frame + token) * 384 64, register
 *         kernel: lane offset loff = p * 384 + ch0 32, register kernel: frame * tokens_per_frame * 384 + step * 16 * 384 64
 *   sslam_selector_saliency: n_frames * G * G * 1536 <= 0xffffffff, else SSLAM_E_UNSUPPORTED. offsets: cell * 1536 + 32 * k-group
 *         into one descriptor over feat 32, (int)rows, cell and padded-cell indices 31, sal[cell] 64
 *   sslam_selector_saliency_ws: n_frames * G * G * 1536 <= 0xffffffff, else SSLAM_E_UNSUPPORTED. offsets: cell * 1536 + 32 *
 *         k-group into one descriptor over feat 32, (int)rows, cell and padded-cell indices 31, sal[cell] 64
 *   sslam_selector_saliency_bf16: n_frames * G * G * 768 <= 0xffffffff, else SSLAM_E_UNSUPPORTED. offsets: cell * 768 + 16 *
 *         k-group into one descriptor over feat_bf16 32, (int)rows, cell and padded-cell indices (the halo form runs below 2^30
 *         cells only) 31, sal[cell] 64
 *   sslam_sim_argmax: n_pairs * ceil(max(n1, n2) / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 *
 *         (slot / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64, keys[pair * n2 +
 *         column] 64
 *   sslam_sim_argmax_d: n_pairs * ceil(max(n1, n2) / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 *
 *         (slot / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64, keys[pair * n2 +
 *         column] 64
 *   sslam_sim_argmax_ws: n_pairs * ceil(max(n1, n2) / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 *
 *         (slot / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64, keys[pair * n2 +
 *         column] 64
 *   sslam_sim_argmax_ws_d: n_pairs * ceil(max(n1, n2) / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 *
 *         (slot / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64, keys[pair * n2 +
 *         column] 64
 *   sslam_sim_argmax_pairs: n_pairs * ceil(max(n1, n2) / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8
 *         * (slot / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64, keys[pair * n2 +
 *         column] 64
 *   sslam_sim_argmax_pairs_d: n_pairs * ceil(max(n1, n2) / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup =
 *         8 * (slot / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64, keys[pair * n2 +
 *         column] 64
 *   sslam_sim_argmax_rows: n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 * (slot /
 *         qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64
 *   sslam_sim_argmax_rows_d: n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 * (slot
 *         / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64
 *   sslam_sim_argmax_rows_pairs: n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 *
 *         (slot / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64
 *   sslam_sim_argmax_rows_pairs_d: n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 *
 *         (slot / qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64
 *   sslam_row_lse: n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 * (slot / qblocks)
 *         + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64
 *   sslam_row_lse_d: n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 * (slot /
 *         qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64
 *   sslam_row_lse_pairs: n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 * (slot /
 *         qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64
 *   sslam_row_lse_pairs_d: n_pairs * ceil(n1 / 128) <= 0x7ffffff0 / 8, else SSLAM_E_UNSUPPORTED. offsets: workgroup = 8 * (slot /
 *         qblocks) + xcd in one grid dimension 31, pair * stride, frame * frame_stride, row * D 64
 *   sslam_edge_pool: n_frames <= 65535, else SSLAM_E_UNSUPPORTED; size / 16 <= 65535, else SSLAM_E_UNSUPPORTED. offsets: grid.z =
 *         n_frames, grid.y = size / 16 31, frame * 3 * size^2 64
 *   sslam_vit_forward: n_frames * T * 1536 <= 0x7fffffff * 64, T = (size / 16)^2 + 5, else SSLAM_E_UNSUPPORTED. offsets: rows *
 *         VMLP in the GEMM tile index (rows * 1536 / 64 stays below 2^31) 31, workspace carving, token rows 64. untested - crosses
 *         2^31 only from 89 478 486 token rows: a bf16 hidden activation of 275 GB, far above 24 GiB of one operand
 *   sslam_vit_forward_form: n_frames * T * 1536 <= 0x7fffffff * 64, T = (size / 16)^2 + 5, else SSLAM_E_UNSUPPORTED. offsets: rows
 *         * VMLP in the GEMM tile index (rows * 1536 / 64 stays below 2^31) 31, workspace carving, token rows 64. untested -
 *         crosses 2^31 only from 89 478 486 token rows: a bf16 hidden activation of 275 GB, far above 24 GiB of one operand
 *   sslam_vit_forward_patches: n_frames * T * 1536 <= 0x7fffffff * 64, T = (size / 16)^2 + 5, else SSLAM_E_UNSUPPORTED. offsets:
 *         rows * VMLP in the GEMM tile index (rows * 1536 / 64 stays below 2^31) 31, workspace carving, token rows 64. untested -
 *         crosses 2^31 only from 89 478 486 token rows: a bf16 hidden activation of 275 GB, far above 24 GiB of one operand
 *   sslam_vit_forward_patches_form: n_frames * T * 1536 <= 0x7fffffff * 64, T = (size / 16)^2 + 5, else SSLAM_E_UNSUPPORTED.
 *         offsets: rows * VMLP in the GEMM tile index (rows * 1536 / 64 stays below 2^31) 31, workspace carving, token rows 64.
 *         untested - crosses 2^31 only from 89 478 486 token rows: a bf16 hidden activation of 275 GB, far above 24 GiB of one
 *         operand
 *   sslam_vit_forward_f32: n_frames * T * 1536 * 4 <= 0xfffffff0, T = (size / 16)^2 + 5, else SSLAM_E_UNSUPPORTED. offsets: GEMM A
 *         operand: row * lda * 4 into one descriptor (widest: the MLP hidden activation) 32, workspace carving, token rows 64
 *   sslam_vit_forward_f32_form: n_frames * T * 1536 * 4 <= 0xfffffff0, T = (size / 16)^2 + 5, else SSLAM_E_UNSUPPORTED. offsets:
 *         GEMM A operand: row * lda * 4 into one descriptor (widest: the MLP hidden activation) 32, workspace carving, token rows
 *         64
 *   sslam_keypoint_depth: n * K <= 0x7fffffff, else SSLAM_E_UNSUPPORTED. offsets: keypoint index n * K 64, frame * h * w 64
 *   sslam_select_keypoints: G * G <= 4096 and K <= 4096, else SSLAM_E_UNSUPPORTED. indexes in 64 bits; one workgroup per frame.
 *         offsets: frame * G * G, frame * K 64
 *   sslam_match_rank: n1 <= 4096, else SSLAM_E_UNSUPPORTED. indexes in 64 bits; one workgroup per pair. offsets: pair * n1 64
 *   sslam_pose_nn_pairs: K <= 4096 (n1 <= 4096), else SSLAM_E_UNSUPPORTED. indexes in 64 bits; one workgroup per pair. offsets:
 *         frame * K, pair * n1 64
 *   sslam_pose_depth_nn_pairs: K <= 4096 (n1 <= 4096), else SSLAM_E_UNSUPPORTED. indexes in 64 bits; one workgroup per pair.
 *         offsets: frame * K, pair * n1 64
 *   sslam_pose_ransac_pairs: K <= 4096 (n1 <= 4096), else SSLAM_E_UNSUPPORTED. indexes in 64 bits; one workgroup per pair.
 *         offsets: frame * K, pair * n1 64
 *   sslam_pose_refine_pairs: K <= 4096 (n1 <= 4096), else SSLAM_E_UNSUPPORTED. indexes in 64 bits; one workgroup per pair.
 *         offsets: frame * K, pair * n1 64
 *   sslam_match_score_pairs: n1 <= 4096, else SSLAM_E_UNSUPPORTED. indexes in 64 bits; one workgroup per pair. offsets: pair * n1
 *         64
 *   sslam_match_score_known_pairs: n1 <= 4096, else SSLAM_E_UNSUPPORTED. indexes in 64 bits; one workgroup per pair. offsets: pair
 *         * n1 64
 *   sslam_keypoint_intensity: no limit - never refuses by size: above 0xfffffff0 bytes of frames or 0x7fffff00 keypoints (or with
 *         more than 7 taps either way, or an img that is not dword aligned) it falls back from intensity_fast_kernel (32-bit
 *         offsets into one descriptor) to intensity_kernel (64 bits); one thread per keypoint
 *   sslam_f32_to_bf16: no limit - indexes in 64 bits; one thread per 8 elements
 *   sslam_gather: no limit - indexes in 64 bits; one thread per four floats of a row
 *   sslam_refine: no limit - indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are int32: it
 *         runs below 2^31 rows only, the direct form above)
 *   sslam_refine_d: no limit - indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are int32: it
 *         runs below 2^31 rows only, the direct form above)
 *   sslam_gather_refine: no limit - indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are int32:
 *         it runs below 2^31 rows only, the direct form above)
 *   sslam_gather_refine_d: no limit - indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are
 *         int32: it runs below 2^31 rows only, the direct form above)
 *   sslam_gather_refine_ws: no limit - indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are
 *         int32: it runs below 2^31 rows only, the direct form above)
 *   sslam_gather_refine_ws_d: no limit - indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are
 *         int32: it runs below 2^31 rows only, the direct form above)
 *   sslam_refine_bf16: no limit - indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are int32:
 *         it runs below 2^31 rows only, the direct form above)
 *   sslam_gather_refine_bf16: no limit - indexes in 64 bits; one workgroup per 32 rows (row indices of the distinct-row form are
 *         int32: it runs below 2^31 rows only, the direct form above)
 *   sslam_match_finalize: no limit - indexes in 64 bits; one workgroup per pair
 *   sslam_match_finalize_pairs: no limit - indexes in 64 bits; one workgroup per pair
 *   sslam_match_finalize_rule: no limit - indexes in 64 bits; one workgroup per pair
 *   sslam_match_finalize_rule_pairs: no limit - indexes in 64 bits; one workgroup per pair
 *   sslam_val_pair_stats: no limit - indexes in 64 bits; one workgroup per pair
 *   sslam_val_pair_stats_pairs: no limit - indexes in 64 bits; one workgroup per pair
 *   sslam_val_frame_stats: no limit - indexes in 64 bits; one workgroup per frame
 *   sslam_val_frame_stats_d: no limit - indexes in 64 bits; one workgroup per frame */

#define SSLAM_C 384   /* backbone embed dim (ViT-S/16), dino_backbone.py:50 */
#define SSLAM_HID 384 /* refiner hidden dim, configs/train_config.yaml:13 */
#define SSLAM_D 128   /* descriptor dim, configs/train_config.yaml:12: the default width; the _d entries also take 256 */

/* library version (major*10000 + minor*100 + patch) and the gfx target it was compiled for */
int sslam_version(void);
const char *sslam_arch(void);
/* number of kernel launches enqueued by this process so far (lets tests prove the HIP path ran) */
long long sslam_launch_count(void);

/* One caller-owned device scratch buffer (bytes, multiple of 256; 0 if none is needed) that serves every *_ws entry of
 * a pipeline step enqueued on one stream - the stages run in stream order and share it: n_frames frames of a G x G grid
 * through sslam_selector_saliency_ws and, with K keypoints each, sslam_gather_refine_ws; n_pairs pairs of K keypoints through
 * sslam_sim_argmax_ws (n_pairs may be 0). */
long long sslam_workspace_bytes(int n_frames, int G, int K, int n_pairs);
/* per-entry needs (what sslam_workspace_bytes takes the maximum of) */
long long sslam_selector_saliency_workspace_bytes(int n_frames, int G);
long long sslam_gather_refine_workspace_bytes(int n_frames, int K);
long long sslam_sim_argmax_workspace_bytes(int n2, int n_pairs);

/* TEST-ONLY: override one of the load-time knobs (name = its environment variable, e.g. "SSLAM_CONV_TAIL"); unset != 0
 * restores the value read from the environment when the library was loaded (else the built-in default).  Not thread-safe against running calls; product code never calls it.  Knobs:
 * SSLAM_M1_VARIANT, SSLAM_CONV_VARIANT, SSLAM_CONV_LATENCY_ROWS, SSLAM_CONV_LAT2_ROWS, SSLAM_CONV_NO_HALO, SSLAM_CONV_TAIL,
 * SSLAM_CONVBF_NO_HALO, SSLAM_CONVBF_TAIL, SSLAM_CONVBF_VARIANT, SSLAM_VIT_NO_FUSED_MLP, SSLAM_BN_FORM,
 * SSLAM_RT_STOP, SSLAM_REFINE_DISTINCT, SSLAM_CONV_BORDER (csrc/common.h says what each selects). */
int sslam_test_set_knob(const char *name, long long value, int unset);

/* ---- weight packing (host side, plain C++; run once per checkpoint) ------------------------------------------
 * The kernels read weights in an LDS-image order: K split into chunks, each chunk stored [n][k] with k permuted
 * inside groups of 8 as (0,2,4,6,1,3,5,7) so that one ds_read_b128 feeds four consecutive 32x32x2 MFMA steps.
 *
 * sslam_pack_conv3x3_host: w (hs,384,3,3) [keypoint_selector.py:31, state_dict key conv.0.weight]
 *                          -> out (9*384*hs floats).
 * sslam_pack_linear_host:  w (n_out, k_in) [nn.Linear weight, descriptor_refiner.py:35,43,103,105]
 *                          -> out (n_out*k_in floats) as [k/8][n][8]; k_in % 8 == 0. */
int sslam_pack_conv3x3_host(const float *w_host, int hs, float *out_host);
int sslam_pack_linear_host(const float *w_host, int n_out, int k_in, float *out_host);

/* ---- A0: preprocessing.  Replaces transforms.Compose([Resize, ToTensor, Normalize]) applied at
 * visualize_matches_sequence.py:59-67,72 (Pillow antialiased bilinear resize, /255, ImageNet mean/std).
 * sslam_resample_table_host builds Pillow's fixed-point coefficient table for one axis (filter 0 = bilinear,
 * 1 = bicubic): bounds (out_size*2 int32: first input index, tap count), coefs (out_size*ksize int32);
 * returns ksize (<= SSLAM_MAX_TAPS) or a negative error.
 * img (n, h, w, 3) uint8 -> out (n, 3, size, size) fp32. */
#define SSLAM_MAX_TAPS 32
int sslam_resample_table_host(int in_size, int out_size, int filter, int32_t *bounds_host, int32_t *coefs_host,
                              int coefs_capacity);
int sslam_preprocess_u8(const uint8_t *img, int n, int h, int w, int size, const int32_t *bounds_h,
                        const int32_t *coefs_h, int ksize_h, const int32_t *bounds_v, const int32_t *coefs_v,
                        int ksize_v, float *out_chw, void *stream);
/* The same arithmetic, written as the patch-embedding operand of sslam_vit_forward_patches instead of the planar image:
 * out (n, (size/16)^2, 768) bf16, row = patch (py, px), k = c*256 + ky*16 + kx - the normalised fp32 value of
 * sslam_preprocess_u8 rounded to bf16 (round-to-nearest-even) once; size % 16 == 0.  SSLAM_E_UNSUPPORTED for resampling
 * ratios the tiled kernel does not cover (more than 7 horizontal taps, or an image base that is not dword-aligned): take
 * sslam_preprocess_u8 + sslam_vit_forward then. */
int sslam_preprocess_u8_patches(const uint8_t *img, int n, int h, int w, int size, const int32_t *bounds_h,
                                const int32_t *coefs_h, int ksize_h, const int32_t *bounds_v, const int32_t *coefs_v,
                                int ksize_v, void *out_patches_bf16, void *stream);

/* ---- A2: token drop + BatchNorm1d over tokens.  Replaces DinoBackbone.forward after the ViT call,
 * dino_backbone.py:91-106.  tokens (n_frames, tokens_per_frame, 384); statistics over `group` consecutive frames
 * (group = 1 reproduces per-frame B=1 calls).  train != 0: batch statistics, also written to
 * out_mean / out_var (n_frames/group, 384; biased variance); train == 0: run_mean / run_var are used.
 * out_feat (n_frames, cells, 384) with cells = tokens_per_frame - n_prefix.
 * Pinned bit for bit to the oracle (tests/test_gpu_trained_ranges.py) in both modes, for n_prefix 0 / 1 / 5, another eps, one cell
 * past each launch-form boundary (784, 1 600, 3 600 cells) and on degenerate channels: a constant channel has batch variance
 * exactly 0 and is scaled by 1/sqrtf(eps) (output beta' + x*alpha, exactly 0 under gamma 1, beta 0); a channel whose spread is
 * far below its mean (1e4 +- 1e-3) is ill-conditioned in fp32 - finite and equal to the oracle, not close to float64. */
int sslam_bn_tokens(const float *tokens, int n_frames, int tokens_per_frame, int n_prefix, int group,
                    const float *gamma, const float *beta, const float *run_mean, const float *run_var, int train,
                    float eps, float *out_feat, float *out_mean, float *out_var, void *stream);

/* ---- A3: saliency CNN.  Replaces KeypointSelector.forward, keypoint_selector.py:45-67
 * (conv3x3 384->hs + ReLU + conv1x1 hs->1 + sigmoid).  feat (n_frames, G, G, 384) NHWC; w1_packed from
 * sslam_pack_conv3x3_host; b1 (hs), w2 (hs), b2 (1); hs in {128, 256}.  sal (n_frames, G, G).
 * Four launch shapes, chosen by size, all bit-identical (same fma chain per output; csrc/selector.hip): the halo
 * and the stage form of the 128-row throughput kernel, and two latency forms for few frames.  The second latency form
 * (two workgroups per 32-cell tile; up to six 28x28 frames) needs 16 bytes of scratch per cell: the _ws entry takes it from
 * the caller (workspace_bytes >= sslam_selector_saliency_workspace_bytes; workspace may be NULL: then, and in the entry
 * without a workspace, the 8-wave latency form runs instead).  G up to 64 is tested in every form.
 * The sigmoid is 1 / (1 + e) with e the canonical exp of -logit (argument clamped to [-87, 88], oracle ora_expf), for every
 * finite logit: exactly 1.0f from about 17 upwards, and from -88 downwards ONE value, 1 / (1 + exp(88)) = 6.0546e-39
 * (bits 0x0041edc4) - a SUBNORMAL, never 0: saliency is strictly positive, and the kernels rely on fp32 denormals not being
 * flushed.  NaN / Inf logits are outside the contract. */
int sslam_selector_saliency(const float *feat, int n_frames, int G, const float *w1_packed, const float *b1,
                            const float *w2, const float *b2, int hs, float *sal, void *stream);
int sslam_selector_saliency_ws(const float *feat, int n_frames, int G, const float *w1_packed, const float *b1,
                               const float *w2, const float *b2, int hs, float *sal, void *workspace,
                               long long workspace_bytes, void *stream);

/* ---- A3, bf16 THROUGHPUT mode (BASELINE.json configs[1] "bf16 conv stack").  Same layer as
 * sslam_selector_saliency with bf16 operands (round-to-nearest-even), fp32 accumulation on v_mfma_f32_32x32x16_bf16 and
 * the fp32 epilogue.  NOT index-exact against the fp32 reference: callers report the agreement rate next to it.
 * sslam_f32_to_bf16: the bf16 copy of the feature map (n % 8 == 0).
 * sslam_pack_conv3x3_bf16_host: w (hs,384,3,3) fp32 -> 9*384*hs bf16 in MFMA-fragment order. */
int sslam_f32_to_bf16(const float *in, void *out_bf16, long long n, void *stream);
/* sslam_bn_tokens that also writes the bf16 copy of out_feat (same shape) in the same pass */
int sslam_bn_tokens_bf16copy(const float *tokens, int n_frames, int tokens_per_frame, int n_prefix, int group,
                             const float *gamma, const float *beta, const float *run_mean, const float *run_var, int train,
                             float eps, float *out_feat, void *out_feat_bf16, float *out_mean, float *out_var, void *stream);
int sslam_pack_conv3x3_bf16_host(const float *w_host, int hs, void *out_bf16_host);
int sslam_selector_saliency_bf16(const void *feat_bf16, int n_frames, int G, const void *w1_packed_bf16, const float *b1,
                                 const float *w2, const float *b2, int hs, float *sal, void *stream);
/* Which kernel sslam_selector_saliency_bf16 launches for this shape (host only, no GPU work; the entry itself dispatches on
 * it): 5..8 = the halo form with that many 64-row groups of the image in LDS, 0 = the stage form (hs != 256, or a grid whose
 * halo image needs more than 8 groups - G = 128 upwards - and would not fit the LDS).  < 0: invalid arguments. */
int sslam_selector_bf16_halo_groups(int n_frames, int G, int hs);

/* ---- A4 + A5 (+ A8): NMS + percentile threshold + branchy top-k.  Replaces KeypointSelector.select_keypoints /
 * _apply_nms, keypoint_selector.py:69-226, and DinoBackbone.patch_to_pixel, dino_backbone.py:154-165.
 * sal (n_frames, G, G) -> kp_xy (n_frames, K, 2) fp32 (x, y) patch units; scores (n_frames, K);
 * idx (n_frames, K) int32 flat cell index (may be NULL); kp_pixel (n_frames, K, 2) = kp*16+8 (may be NULL);
 * status (n_frames) int32: 0 ok, 1 = the reference's torch.topk would raise (K exceeds the cells).
 * No host synchronisation: the whole data-dependent control flow runs on the device, one workgroup per frame.
 * G*G <= 4096, K <= 4096, 0 <= nms_radius <= 8.
 * Tested over that whole range (tests/test_gpu_select_range.py): every radius 0..8 - windows wider than the grid included - on
 * grids from 1 x 1 to 64 x 64, every arm of the control flow at each radius 5..8, K beyond the cells, idx / kp_pixel NULL, and the
 * reference's own output at radius 4..8 (tests/golden/select_range.npz). */
int sslam_select_keypoints(const float *sal, int n_frames, int G, int K, int nms_radius, double min_score_percentile,
                           float *kp_xy, float *scores, int32_t *idx, float *kp_pixel, int32_t *status,
                           void *stream);

/* ---- A6: bilinear feature gather.  Replaces DinoBackbone.extract_at_keypoints, dino_backbone.py:114-152
 * (grid_sample bilinear, align_corners=True, zero padding).  feat (n_frames, G, G, 384), kp_xy (n_frames, K, 2)
 * -> out (n_frames, K, 384). */
int sslam_gather(const float *feat, int n_frames, int G, const float *kp_xy, int K, float *out, void *stream);

/* ---- A7: descriptor MLP.  Replaces DescriptorRefiner.forward / ResidualBlock.forward,
 * descriptor_refiner.py:58-126.  Refiner weights are passed as ONE packed device buffer laid out by
 * sslam_refiner_pack_host (offsets in floats are returned by sslam_refiner_layout).
 * x (rows, 384) -> desc (rows, 128).  0 <= n_blocks <= 8, every depth bit-identical to the oracle (tests at 0, 1, 2, 3, 8).
 * Finite inputs give finite descriptors: a row whose hidden activations are all equal (all dead, for one) passes LayerNorm as
 * (0 * 1/sqrtf(1e-5f)) * gamma + beta = beta; the output is v / max(sqrtf(sum v^2), 1e-12f) with the correctly rounded divide,
 * so a zero output stays +0, a norm below 1e-12 (squares that underflow or are subnormal) divides by 1e-12, and a sum of
 * squares that overflows to +inf gives 0 - as F.normalize does in fp32. */
typedef struct {
    int n_blocks;          /* residual blocks (num_layers - 2; 2 in the shipped config) */
    long long total;       /* floats in the packed buffer */
    long long in_w, in_b;  /* packed input_proj.weight, input_proj.bias */
    long long blk[8][8];   /* per block: norm1.w, norm1.b, fc1.w(packed), fc1.b, norm2.w, norm2.b, fc2.w(packed), fc2.b */
    long long out_w, out_b;
} sslam_refiner_layout_t;
int sslam_refiner_layout(int n_blocks, sslam_refiner_layout_t *layout_host);
/* w_host: 4 + 8*n_blocks host pointers in state_dict order (see oracle/sslam_oracle.h ora_refine) */
int sslam_refiner_pack_host(const float *const *w_host, int n_blocks, float *out_host);
int sslam_refine(const float *x, long long rows, const float *packed, int n_blocks, float *desc, void *stream);

/* ---- A6 + A7 fused: gather straight into the MLP's LDS tile (the pipeline's fast path). */
int sslam_gather_refine(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed,
                        int n_blocks, float *desc, void *stream);
/* The same descriptors with every DISTINCT keypoint of a frame run through the MLP once.  sslam_select_keypoints usually ends in
 * the reference's pad (the NMS survivors, then the top raw saliencies, where the survivors re-appear: SURVEY H2), so ~7 % of a
 * frame's keypoints repeat an earlier one; equal coordinates give equal descriptors.  A launch per frame finds, for every slot,
 * the lowest slot of its frame with the same 64 coordinate BITS (+0.0 and -0.0 stay apart, a NaN coordinate never merges), a
 * second packs the distinct rows of all frames into one list, the MLP kernel runs the list (its arithmetic per row is that of
 * sslam_gather_refine, and rows are independent in it: the same bits), and a copy fills the repeated slots.  Taken for launches of
 * more than one round of MLP workgroups (24 576 rows) with K <= 4096; smaller ones, a NULL workspace or one shorter than
 * sslam_gather_refine_workspace_bytes (0 where the direct launch is taken) run the launch of sslam_gather_refine.
 * After the list form the workspace holds, as int32: [f] the number of distinct keypoints of frame f, [n_frames] their sum. */
int sslam_gather_refine_ws(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed,
                           int n_blocks, float *desc, void *workspace, long long workspace_bytes, void *stream);

/* ---- A6 + A7, bf16 THROUGHPUT mode (BASELINE.json configs[1]): the same gather + MLP with bf16
 * GEMM operands (v_mfma_f32_32x32x16_bf16), fp32 accumulation / residual / LayerNorm statistics / L2 normalisation;
 * LayerNorm is folded into the following GEMM (W*gamma, column sums, b + W beta are precomputed by the packer).
 * NOT bit-exact against the fp32 reference.  packed_bf16: sslam_refiner_bf16_bytes(n_blocks) bytes written by
 * sslam_refiner_pack_bf16_host from the same pointer list as sslam_refiner_pack_host. */
long long sslam_refiner_bf16_bytes(int n_blocks);
int sslam_refiner_pack_bf16_host(const float *const *w_host, int n_blocks, void *out_host);
int sslam_refine_bf16(const float *x, long long rows, const void *packed_bf16, int n_blocks, float *desc, void *stream);
int sslam_gather_refine_bf16(const float *feat, int n_frames, int G, const float *kp_xy, int K, const void *packed_bf16,
                             int n_blocks, float *desc, void *stream);

/* ---- A9: per-keypoint intensity.  Replaces visualize_matches_sequence.py:87-95 (Pillow BICUBIC resize to
 * (size,size) -> "L" -> /255 -> gray[round(y), round(x)]); only the pixels that are looked up are resampled.
 * img (n, h, w, 3) uint8; kp_pixel (n, K, 2); tables from sslam_resample_table_host(filter = 1). */
int sslam_keypoint_intensity(const uint8_t *img, int n, int h, int w, int size, const int32_t *bounds_h,
                             const int32_t *coefs_h, int ksize_h, const int32_t *bounds_v, const int32_t *coefs_v,
                             int ksize_v, const float *kp_pixel, int K, float *out, void *stream);

/* ---- M1..M5 core: cosine-similarity GEMM + row / column arg-max.  Replaces torch.mm + argmax(dim=1) +
 * argmax(dim=0) at visualize_matches_sequence.py:144-148 (and visualize_matches.py:105-109, train.py:423-425,
 * test/test_descriptor_quality.py:116-123, test/test_tracking.py:159-160).
 * For each of n_pairs pairs p: d1 = desc1 + p*stride1 (n1 x 128), d2 = desc2 + p*stride2 (n2 x 128)
 * (strides in floats; stride 0 broadcasts).  nn12/s12 (n_pairs, n1): first arg-max / max over d2 for each row of
 * d1; nn21/s21 (n_pairs, n2): the column direction.  second12 (n_pairs, n1): the largest similarity of the row with
 * the winner removed (-inf if n2 == 1) - what the ratio tests of visualize_matches.py:116-121 and
 * test/test_descriptor_quality.py:129-131 need, without sorting rows.  s12 / s21 / second12 may be NULL.
 * sslam_sim_argmax_ws, batched calls (n_pairs >= 16) with workspace_bytes >= sslam_sim_argmax_workspace_bytes(n2, n_pairs)
 * = n_pairs*n2*8 bytes of caller-owned scratch: the similarity matrix is evaluated once and the column direction reduced
 * with 64-bit (value, ~index) keys and atomic max - deterministic.  Smaller calls, a NULL / short workspace, and the entry
 * without a workspace evaluate it once per direction and need no scratch.  Same bits either way.
 * Precondition: finite descriptors (the refiner's L2-normalised rows are).  With NaN / Inf in the inputs the VALUES and the
 * choice among candidates are unspecified (torch.argmax would return the first NaN), but every index written stays inside
 * [0, n2) resp. [0, n1), so sslam_match_finalize and the sibling matchers never index out of range.
 * Tested bit for bit where no similarity is positive (tests/test_gpu_sim_signs.py): all-negative and mixed-sign sets, the winner in
 * the last stage of candidates, rows and columns of exact zeros, in both forms and at both widths; the same file sets every
 * threshold of sslam_match_finalize and sslam_match_finalize_rule to the value compared and one ulp either side of it. */
int sslam_sim_argmax(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2,
                     int n_pairs, int32_t *nn12, float *s12, int32_t *nn21, float *s21, float *second12, void *stream);
int sslam_sim_argmax_ws(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2,
                        int n_pairs, int32_t *nn12, float *s12, int32_t *nn21, float *s21, float *second12,
                        void *workspace, long long workspace_bytes, void *stream);

/* ---- M1: mutual check + thresholds + quality + ordered compaction.  Replaces
 * SequenceMatcher.match_with_quality, visualize_matches_sequence.py:149-197, given the arg-max arrays above.
 * scores / intensities are (n_pairs-strided) per-frame arrays like the descriptors; intensity1/2 may be NULL.
 * Outputs per pair: matches (cap = n1 rows of 2 int64, ascending idx1), quality (n1 fp32), count (1 int32). */
int sslam_match_finalize(const int32_t *nn12, const float *s12, const int32_t *nn21, int n1, int n2, int n_pairs,
                         const float *scores1, long long sstride1, const float *scores2, long long sstride2,
                         const float *intensity1, const float *intensity2, float w_desc, float w_sal,
                         float min_saliency, float min_sim, float min_intensity, int64_t *matches, float *quality,
                         int32_t *count, void *stream);

/* ---- M1 over a PAIR LIST in device memory: the two entries above for pairs no stride can express - several spacings of an
 * online step in one launch pair, a frame against a caller's keyframes, loop-closure candidates.
 * bank (n_bank, K, 128) fp32, frame_stride floats between frames (alignment rules of sslam_sim_argmax_ws: a 16-byte aligned
 * base, a stride that is a multiple of 4 floats).  pair_first / pair_second: DEVICE int32 arrays of n_pairs frame indices into
 * the bank; pair p matches d1 = frame pair_first[p] against d2 = frame pair_second[p], n1 = n2 = K.  Any two frames make a
 * pair: in any order, the same frame twice, a pair listed twice.  The lists are read by the kernels, never by the host: the
 * calls only enqueue, a list may be written by earlier work of the same stream, and a captured graph replays with whatever
 * the lists hold then.
 * Per pair the arithmetic, the two launch forms, the rule and the knob that choose between them and the workspace
 * (sslam_sim_argmax_workspace_bytes(K, n_pairs)) are those of sslam_sim_argmax_ws: the same bits as the strided entries on the
 * same two frames.  Outputs as there, one row per listed pair in list order.
 * ABSENT pairs: a pair either of whose indices lies outside [0, n_bank) - write -1 - is absent.  Its workgroups decide that
 * from the two index words before any address is formed from them and read no bank: no index value makes the library read
 * outside the banks described here.  An absent pair's rows: nn12 = nn21 = 0, s12 = s21 = second12 = 0.0f, count = 0, matches
 * and quality zeroed like the slots past the count.
 * sslam_match_finalize_pairs: scores_bank (n_bank, K) with score_stride floats between frames and intensity_bank (may be NULL)
 * with the same stride are indexed by the same two lists. */
int sslam_sim_argmax_pairs(const float *bank, long long frame_stride, int n_bank, int K, const int32_t *pair_first,
                           const int32_t *pair_second, int n_pairs, int32_t *nn12, float *s12, int32_t *nn21, float *s21,
                           float *second12, void *workspace, long long workspace_bytes, void *stream);
int sslam_match_finalize_pairs(const int32_t *nn12, const float *s12, const int32_t *nn21, int K, int n_bank,
                               const int32_t *pair_first, const int32_t *pair_second, int n_pairs, const float *scores_bank,
                               long long score_stride, const float *intensity_bank, float w_desc, float w_sal,
                               float min_saliency, float min_sim, float min_intensity, int64_t *matches, float *quality,
                               int32_t *count, void *stream);

/* ---- M2 / M4 / M5: the sibling matchers' rules on the device - the finalize stage of sslam_match_finalize[_pairs] with another
 * rule, given nn12 / s12 / second12 / nn21 of sslam_sim_argmax[_pairs] (strided form: n_pairs-strided arrays, pair p's rows at
 * p*n1 resp. p*n2; pair-list form: n1 = n2 = K, the two DEVICE lists of sslam_sim_argmax_pairs over a bank of n_bank frames decide
 * only whether a pair is absent).  One workgroup per pair; outputs per pair as there: matches (n1 rows of 2 int64 (idx1, idx2),
 * ascending idx1), value (n1 fp32), count (1 int32); slots past the count are zeroed; an absent pair has count 0 and zero rows.
 * For row i with j = nn12[i] (a j outside [0, n2) is never used: the row is not kept):
 *   SSLAM_RULE_RATIO_BEST   M2, MatchVisualizer.find_matches, visualize_matches.py:102-124 (mutual :114, ratio test :117-121):
 *                           keep iff nn21[j] == i and s12[i] > max(second12[i], -1) * param; value = s12[i] (the original
 *                           writes -1 over the winner and takes the row's max, so with n2 == 1 the runner-up is -1);
 *   SSLAM_RULE_RATIO_SECOND M4, find_mutual_nearest_neighbors, test/test_descriptor_quality.py:97-142 (mutual :126, ratio
 *                           :129-131, distance :140): keep iff nn21[j] == i and second12[i] / (s12[i] + 1e-8f) < param, the add
 *                           and the divide each rounded to fp32 once; value = 1.0f - s12[i].  n2 < 2: SSLAM_E_INVALID before
 *                           anything is launched (the original's np.sort(...)[:, 1] raises);
 *   SSLAM_RULE_TRACKED      M5, the tracking count of track_frame_sequence, test/test_tracking.py:158-161: keep iff
 *                           s12[i] > param - no mutual check; nn21 and second12 are not read and may be NULL; value = s12[i];
 *                           count is the original's `matches`.
 * param (ratio_thresh / ratio_threshold / match_threshold) is fp32: the originals compare fp32 arrays with a Python scalar,
 * which numpy rounds to fp32 first.  Every comparison is false on a NaN: such a row is not kept.
 * SSLAM_E_INVALID, before anything is launched: a NULL nn12 / s12 / matches / value / count, an unknown rule, NULL second12 or
 * nn21 where the rule reads them, NULL or misaligned pair lists, non-positive sizes. */
#define SSLAM_RULE_RATIO_BEST 1
#define SSLAM_RULE_RATIO_SECOND 2
#define SSLAM_RULE_TRACKED 3
int sslam_match_finalize_rule(const int32_t *nn12, const float *s12, const float *second12, const int32_t *nn21, int n1, int n2,
                              int n_pairs, int rule, float param, int64_t *matches, float *value, int32_t *count, void *stream);
int sslam_match_finalize_rule_pairs(const int32_t *nn12, const float *s12, const float *second12, const int32_t *nn21, int K,
                                    int n_bank, const int32_t *pair_first, const int32_t *pair_second, int n_pairs, int rule,
                                    float param, int64_t *matches, float *value, int32_t *count, void *stream);

/* ---- The row direction alone, for callers that need no nn21 (SSLAM_RULE_TRACKED; test/test_tracking.py:159-160 takes only
 * sim_matrix.max(axis=1)): nn12, s12 (may be NULL) and second12 (may be NULL) of sslam_sim_argmax resp. sslam_sim_argmax_pairs -
 * the same bits as those entries write in either of their launch forms - from ONE launch of the row direction of the two-pass
 * form, half its work; no workspace.  Arguments, alignment rules and absent pairs (nn12 = 0, s12 = second12 = 0.0f) as there. */
int sslam_sim_argmax_rows(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2,
                          int n_pairs, int32_t *nn12, float *s12, float *second12, void *stream);
int sslam_sim_argmax_rows_pairs(const float *bank, long long frame_stride, int n_bank, int K, const int32_t *pair_first,
                                const int32_t *pair_second, int n_pairs, int32_t *nn12, float *s12, float *second12, void *stream);

/* ---- A1: DINOv3 ViT-S/16 forward.  Replaces the third-party call
 * `self.dino.forward_features(images)` at dino_backbone.py:85 (timm model "vit_small_patch16_dinov3"): 16x16 patch
 * embedding, [CLS] + 4 register tokens, 12 pre-LN blocks (6 heads x 64, q/v/proj bias, axial RoPE theta 100 on the
 * patch tokens, LayerScale, MLP 1536 GELU), final LayerNorm.  bf16 MFMA operands, fp32 accumulation / LayerNorm /
 * softmax / residual stream: tolerance-level parity with an fp32 evaluation (not bit-exact).
 * All pointers are DEVICE pointers; vectors fp32; matrices bf16, nn.Linear (n_out, k_in) re-ordered by
 * sslam_vit_pack_linear_host into the order the GEMM kernel streams them: one 1 KB MFMA fragment per (192-column tile,
 * k-step of 16, 32-column slice): element (n, k) -> [n/192][k/16][(n%192)/32][(k%16)/8][n%32][k%8].
 * wqkv = rows [q_proj; k_proj; v_proj] (1152, 384), bqkv likewise with ZEROS for the k rows (no key bias), the q rows of
 * both multiplied by log2(e)/sqrt(64) (softmax runs in the exp2 domain); wo / bo and wdown / bdown multiplied row-wise by
 * the block's LayerScale (ls1, ls2) - the caller folds these constants before packing (sslam_amd/vit_hip.py does);
 * patch_w = Conv2d weight reshaped (384, 768); prefix = [cls; reg0..3] (5, 384); rope_cos / rope_sin (G*G, 64) fp32.
 * images_chw (n, 3, size, size) fp32 (the output of sslam_preprocess_u8) -> tokens_out (n, 5 + (size/16)^2, 384). */
typedef struct {
    const float *ln1_g, *ln1_b;
    const void *wqkv;
    const float *bqkv;
    const void *wo;
    const float *bo, *ln2_g, *ln2_b;
    const void *wup;
    const float *bup;
    const void *wdown;
    const float *bdown;
    const void *wmlp;      /* optional (may be NULL): up_proj + down_proj as ONE stream for the fused MLP kernel
                              (sslam_vit_pack_mlp_host); used for batches of more than ~8 frames, wup / wdown otherwise */
} sslam_vit_layer_t;
typedef struct {
    const void *patch_w;
    const float *patch_b, *prefix;
    sslam_vit_layer_t layer[12];
    const float *norm_g, *norm_b, *rope_cos, *rope_sin;
} sslam_vit_weights_t;
/* host helper: fp32 nn.Linear weight (n_out, k_in), n_out % 192 == 0, k_in % 384 == 0 -> the packed bf16 image above */
int sslam_vit_pack_linear_host(const float *w, int n_out, int k_in, uint16_t *out);
/* host helper: up_proj (1536, 384) + down_proj (384, 1536) [rows times row_scale = LayerScale 2, or NULL] -> the 2 x 1536 x 384
 * bf16 stream of the fused MLP kernel (per 64-wide hidden chunk: 48 KB of up rows, then 48 KB of down columns) */
int sslam_vit_pack_mlp_host(const float *w_up, const float *w_down, const float *row_scale, uint16_t *out);
long long sslam_vit_workspace_bytes(int n_frames, int size);
int sslam_vit_forward(const float *images_chw, int n_frames, int size, const sslam_vit_weights_t *weights_host_struct,
                      void *workspace, long long workspace_bytes, float *tokens_out, void *stream);
/* the same forward from the bf16 patch rows of sslam_preprocess_u8_patches (n, (size/16)^2, 768): no fp32 image, no
 * im2patch pass; bit-identical tokens (the patch embedding rounds the image to bf16 either way) */
int sslam_vit_forward_patches(const void *patches_bf16, int n_frames, int size, const sslam_vit_weights_t *weights_host_struct,
                              void *workspace, long long workspace_bytes, float *tokens_out, void *stream);

/* ---- A1 with the reference's numerics: the same forward in fp32 (the reference's timm model runs in fp32,
 * dino_backbone.py:85) on v_mfma_f32_32x32x2_f32 - fp32 operands, fma-chain contractions, fp32 LayerNorm / softmax / erf-GELU /
 * residual stream.  Agrees with an fp32 torch evaluation of the same weights to ~1e-5 relative (summation order).
 * All pointers DEVICE pointers to fp32; nothing is folded into the weights (ls1 / ls2 are the LayerScale vectors).  The four
 * per-layer matrices - wqkv = rows [q_proj; k_proj; v_proj] (1152, 384), wo (384, 384), wup (1536, 384), wdown (384, 1536) - are
 * re-ordered by sslam_vit_f32_pack_linear_host into the MFMA fragment order their kernel streams from L2 (same values, same
 * size); bqkv has zeros for the k rows; patch_w is the Conv2d weight viewed as (384, 768), as it is; prefix, rope_cos / rope_sin
 * as in sslam_vit_weights_t - DINOv3's construction, the 32 angles of a cell tiled twice: columns d and d + 32 of a row are equal
 * and this entry reads columns 0..31 only (a caller with other tables must not use it; sslam_amd/vit_hip.py checks).
 * Workspace: sslam_vit_f32_workspace_bytes(n_frames, size) bytes (x, LayerNorm output, q / k / v, MLP hidden: 13.7 KB per token;
 * for n_frames <= SSLAM_ATTN_KEY_SPLIT_MAX_FRAMES also the key-split attention's partials, 7.9 KB per token; for 9 - 12 frames
 * the larger need of 8 key-split frames).  It never decreases with n_frames: a buffer sized for a batch serves every smaller
 * launch in either form.  sslam_vit_forward_f32_form checks the requested form's own need (ONE_PASS: no partials). */
typedef struct {
    const float *ln1_g, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ls1, *ln2_g, *ln2_b, *wup, *bup, *wdown, *bdown, *ls2;
} sslam_vit_layer_f32_t;
typedef struct {
    const float *patch_w, *patch_b, *prefix;
    sslam_vit_layer_f32_t layer[12];
    const float *norm_g, *norm_b, *rope_cos, *rope_sin;
} sslam_vit_weights_f32_t;
/* host helper: fp32 nn.Linear weight (n_out, k_in), n_out % 128 == 0, k_in % 32 == 0 -> element (n, k) at
 * [n/32][k/8][(k%8)/4][n%32][k%4] */
int sslam_vit_f32_pack_linear_host(const float *w, int n_out, int k_in, float *out);
long long sslam_vit_f32_workspace_bytes(int n_frames, int size);
int sslam_vit_forward_f32(const float *images_chw, int n_frames, int size, const sslam_vit_weights_f32_t *weights_host_struct,
                          void *workspace, long long workspace_bytes, float *tokens_out, void *stream);
/* The same forward with the attention's launch form named by the caller.  The reference's callers run the backbone at B = 1
 * (visualize_matches_sequence.py:72-74) and B = 4 (train.py:300-302): a launch of a few frames leaves most of the chip idle
 * while 42 workgroups per frame walk all key tiles one after the other.  attention_form:
 *   SSLAM_ATTN_ONE_PASS  (0) one workgroup per (frame, head, 128 queries) over all keys - the throughput form;
 *   SSLAM_ATTN_KEY_SPLIT (1) five workgroups per (frame, head, 128 queries), one contiguous key range each, un-normalised
 *                            partials (O, running maximum, row sum) in the workspace, merged in the fixed order 0..4 by a second
 *                            launch: deterministic, independent of the batch, ~1e-6 relative from the one-pass form (another
 *                            summation order of the same softmax); n_frames <= SSLAM_ATTN_KEY_SPLIT_MAX_FRAMES, else
 *                            SSLAM_E_INVALID (the workspace holds the partials only up to that size).  The same form runs the
 *                            down projection (K = 1536) with the four waves of a workgroup summing one K quarter each, the
 *                            quarters added in a fixed order: the few-frame form of the forward as a whole.
 * sslam_vit_forward_f32 is this entry with form = KEY_SPLIT when n_frames <= SSLAM_ATTN_KEY_SPLIT_MAX_FRAMES, else ONE_PASS; a
 * caller that cuts one batch into several launches passes the form of the WHOLE batch to each, so that a frame's tokens do not
 * depend on where the cuts fall (sslam_amd/vit_hip.py does). */
#define SSLAM_ATTN_ONE_PASS 0
#define SSLAM_ATTN_KEY_SPLIT 1
#define SSLAM_ATTN_KEY_SPLIT_MAX_FRAMES 8
int sslam_vit_forward_f32_form(const float *images_chw, int n_frames, int size, const sslam_vit_weights_f32_t *weights_host_struct,
                               void *workspace, long long workspace_bytes, float *tokens_out, int attention_form, void *stream);

/* The bf16 forward (sslam_vit_forward / sslam_vit_forward_patches above) with its launch form named by the caller.  The unnamed
 * entries pick by the launch's token rows (SMALL up to 8 192 rows, THROUGHPUT above) and stay exactly as they are.  form:
 *   SSLAM_VIT_FORM_THROUGHPUT (0) 128-row GEMM workgroups over two / three / four 192-column tiles, one-pass attention, the
 *                                 fused MLP launch when wmlp is given - at any frame count;
 *   SSLAM_VIT_FORM_SMALL      (1) one 192-column tile per GEMM workgroup, one-pass attention, two-launch MLP - at any frame
 *                                 count (a caller that cuts a long batch can pin the form of a short last group);
 *   SSLAM_VIT_FORM_FEW_FRAME  (2) n_frames <= SSLAM_VIT_FEW_FRAME_MAX_FRAMES.  SMALL's QKV and up launches, and
 *       - key-split attention: the 64-key tiles of a frame are cut into R = ceil(tiles / ceil(tiles / 4)) contiguous ranges
 *         of ceil(tiles / 4) tiles (R <= 4; a function of the token count only), one workgroup per (frame, head, 128 queries,
 *         range), every range starting from the one-pass shift (the maximum over key tile 0), leaves un-normalised fp32
 *         partials (O, shift m, row sum l) in the workspace;
 *       - merge + output projection + residual in one launch: per 32 tokens of a frame, wave h merges head h in the order
 *         0, 1, .. with M = max m_s and weights 2^(m_s - M), normalises and rounds to bf16 once - the merged tile is the MFMA
 *         operand of the projection as it stands - and the six waves sum K = 384 head by head into 64 output columns each;
 *       - the down projection (K = 1536) in 32-row workgroups whose four waves take one 384-wide K chunk each, the chunks
 *         added in LDS as ((q0 + q1) + q2) + q3, q0 starting from the bias.
 *     Every sum has one order fixed by the token count: a frame's tokens are the same bits alone, at any position among up
 *     to 8 frames, and in any cut of such a batch into launches that all name this form.  Against SMALL it is another summation
 *     order of the same arithmetic (and a range's P is rounded to bf16 relative to the range's own shift).
 * sslam_vit_workspace_bytes_form: the named form's need - THROUGHPUT / SMALL = sslam_vit_workspace_bytes, FEW_FRAME = that plus
 * the attention partials (8.5 KB per query and range); for one form it never decreases with n_frames, so a buffer sized for a
 * batch serves every shorter launch of it.  SSLAM_E_INVALID, before anything is launched, for an unknown form, for FEW_FRAME
 * with n_frames > SSLAM_VIT_FEW_FRAME_MAX_FRAMES and for a workspace smaller than the form's need. */
#define SSLAM_VIT_FORM_THROUGHPUT 0
#define SSLAM_VIT_FORM_SMALL 1
#define SSLAM_VIT_FORM_FEW_FRAME 2
#define SSLAM_VIT_FEW_FRAME_MAX_FRAMES 8
long long sslam_vit_workspace_bytes_form(int n_frames, int size, int form);
int sslam_vit_forward_form(const float *images_chw, int n_frames, int size, const sslam_vit_weights_t *weights_host_struct,
                           void *workspace, long long workspace_bytes, float *tokens_out, int form, void *stream);
int sslam_vit_forward_patches_form(const void *patches_bf16, int n_frames, int size, const sslam_vit_weights_t *weights_host_struct,
                                   void *workspace, long long workspace_bytes, float *tokens_out, int form, void *stream);

/* ---- Checkpoint validation: the forward of the trainer's losses under no_grad (train.py:451-499 validate -> :292-408
 * _forward_pass; losses/self_supervised.py), as per-frame and per-pair statistics a host function composes into the seven
 * loss terms and five batch metrics for any batch size (sslam_amd/validation.py states the composition).  Forward only.
 * Every sum below has one order fixed by the shapes alone: a frame's or a pair's results are the same bits in any launch.
 *
 * sslam_row_lse / sslam_row_lse_pairs: for every row i of frame a against all rows j of frame b, with
 *   x_ij = clamp(s_ij / temperature, -50, 50) (self_supervised.py:58-59; s_ij the similarity bits of sslam_sim_argmax):
 *     ce[pair, i]  = log sum_j exp(x_ij - max_j x_ij)       the row's cross-entropy against its nearest neighbour (:62)
 *     lse[pair, i] = max_j x_ij + ce[pair, i]               = log sum_j exp(x_ij)
 *     s00[pair]    = s_00                                   (the target of the trainer's zero-padded match rows, train.py:445)
 *   s12 (n_pairs, n1) must be the row maxima of the same pairs, as sslam_sim_argmax / sslam_sim_argmax_rows (and their _pairs
 *   forms) write them: the kernel sums exp(x_ij - clamp(s12_i / temperature)) in one pass.  Each of lse, ce, s00 may be NULL
 *   (lse and ce not both).  Pairs are named as in sslam_sim_argmax_rows / sslam_sim_argmax_rows_pairs (strides in floats; an
 *   index outside [0, n_bank), -1 by convention, is an absent pair: zero rows, s00 = 0).  temperature > 0, finite.
 *   The K x K logits are never written to memory; exp and log are the library's canonical fmaf-only forms.
 *   Tested (tests/test_gpu_validation_edges.py) with both clamp arms reached in every row, n1 != n2, stride1 = 0, 9 and 17
 *   pairs of two query blocks each, every NULL combination of the outputs, and outputs lying between sentinel rows. */
int sslam_row_lse(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2, int n_pairs,
                  const float *s12, float temperature, float *lse, float *ce, float *s00, void *stream);
int sslam_row_lse_pairs(const float *bank, long long frame_stride, int n_bank, int K, const int32_t *pair_first,
                        const int32_t *pair_second, int n_pairs, const float *s12, float temperature, float *lse, float *ce,
                        float *s00, void *stream);
/* sslam_edge_pool: the image side of EdgeAwarenessLoss.forward (self_supervised.py:248-260) in one pass over the fp32
 * normalised image (n, 3, size, size) that sslam_preprocess_u8 writes, size % 16 == 0 (else SSLAM_E_UNSUPPORTED):
 *   gray = 0.299 c0 + 0.587 c1 + 0.114 c2; 3 x 3 Sobel x and y with ZERO padding at the border; mag = sqrt(gx^2 + gy^2 + 1e-8);
 *   pooled (n, size/16, size/16) = the 16 x 16 block means of mag (what adaptive_avg_pool2d gives at this size, before the
 *   reference's division by the batch maximum: a positive factor the host applies); edge_max (n) = the frame's maximum of mag.
 * images_chw 16-byte aligned.  No scratch: the maximum is an integer atomic max on the bits of the positive magnitudes.
 * Tested (tests/test_gpu_validation_edges.py) at sizes 512, 544, 1024 and 1040 - one to three column segments of 512 pixels, the
 * last 32 or 16 wide - where a cell's block mean has the same bits wherever the cell lies in a segment. */
int sslam_edge_pool(const float *images_chw, int n_frames, int size, float *pooled, float *edge_max, void *stream);
/* sslam_val_frame_stats: one row of SSLAM_VAL_FRAME_STATS floats per frame from its saliency map (n, G, G):
 *   SAL_MEAN, SAL_VAR (biased, :196), SAL_MAX, SAL_DX = sum |s[y][x+1] - s[y][x]|, SAL_DY = sum |s[y+1][x] - s[y][x]| (:300-301),
 *   SAL_HIGH = number of cells > 0.6 (:309), SAL_SS = sum (s - mean)^2;
 *   with pooled / edge_max of sslam_edge_pool (both or neither; without them the EDGE slots are 0): EDGE_MEAN = mean P,
 *   EDGE_A = sum (P - mean P)(s - mean s), EDGE_E = sum (P - mean P)^2 (:270-275), EDGE_MAX = edge_max;
 *   with descriptors (n, K, 128) (or NULL): desc_mean (n, 128) the mean over the K rows per dimension, desc_m2 (n, 128) the sum
 *   of squares about it (two passes) - frames combine by the pairwise update of mean and M2 (:102-109). */
#define SSLAM_VAL_FRAME_STATS 12
#define SSLAM_VAL_SAL_MEAN 0
#define SSLAM_VAL_SAL_VAR 1
#define SSLAM_VAL_SAL_MAX 2
#define SSLAM_VAL_SAL_DX 3
#define SSLAM_VAL_SAL_DY 4
#define SSLAM_VAL_SAL_HIGH 5
#define SSLAM_VAL_SAL_SS 6
#define SSLAM_VAL_EDGE_A 7
#define SSLAM_VAL_EDGE_E 8
#define SSLAM_VAL_EDGE_MEAN 9
#define SSLAM_VAL_EDGE_MAX 10
int sslam_val_frame_stats(const float *saliency, const float *pooled, const float *edge_max, const float *descriptors, int n_frames,
                          int G, int K, float *stats, float *desc_mean, float *desc_m2, void *stream);
/* sslam_val_pair_stats / sslam_val_pair_stats_pairs: one row of SSLAM_VAL_PAIR_STATS floats per pair (a, b):
 *   PAIR_REPEAT  = mean (s_a - s_b)^2 over the G x G cells (RepeatabilityLoss, :180-182);
 *   PAIR_MATCHES = number of rows i with nn21[nn12[i]] == i, the mutual nearest neighbours of _find_matches (train.py:423-428;
 *                  no thresholds), also as an integer in n_matches (n_pairs);
 *   PAIR_CE_SUM  = sum of ce[i] over those rows;
 *   PAIR_PAD_CE  = lse_0 - x_00 = ce[0] + (clamp(s12[0] / T) - clamp(s00 / T)): a zero-padded match row.
 * nn12, nn21, s12 from sslam_sim_argmax[_pairs], ce and s00 from sslam_row_lse[_pairs] over the same pairs; the strided form
 * takes frame p of saliency1 and of saliency2 (n_pairs, G, G each), the listed form a bank (n_bank, G, G) and the two lists
 * (an absent pair: a zero row, n_matches 0). */
#define SSLAM_VAL_PAIR_STATS 4
#define SSLAM_VAL_PAIR_REPEAT 0
#define SSLAM_VAL_PAIR_CE_SUM 1
#define SSLAM_VAL_PAIR_PAD_CE 2
#define SSLAM_VAL_PAIR_MATCHES 3
int sslam_val_pair_stats(const float *saliency1, const float *saliency2, int G, const int32_t *nn12, const int32_t *nn21,
                         const float *s12, const float *ce, const float *s00, int n1, int n2, int n_pairs, float temperature,
                         float *stats, int32_t *n_matches, void *stream);
int sslam_val_pair_stats_pairs(const float *saliency_bank, int G, int n_bank, const int32_t *pair_first, const int32_t *pair_second,
                               const int32_t *nn12, const int32_t *nn21, const float *s12, const float *ce, const float *s00, int K,
                               int n_pairs, float temperature, float *stats, int32_t *n_matches, void *stream);

/* ---- Descriptor width 128 or 256.  SSLAM_D above is the DEFAULT width, the one every entry without a width argument works at
 * (each of them is its _d form with d = SSLAM_D).  The _d entries below take the width as `int d`, the last argument before
 * `stream` (before the output pointer in the two host-side packers): d = 128 runs the very kernels of the unsuffixed entry,
 * d = 256 their second instantiation - the refiner's output projection over two 32-column tiles per wave (output_proj.weight
 * (256, 384); column layout wave*64 + 32*t + crow(e, h); the L2 norm one fma chain over the lane's 32 outputs in (t, e) order,
 * then the same row tree), descriptors / banks with rows of 256 floats, and every similarity ONE fma chain over k = 0 .. 255
 * ascending - bit-identical to the oracle at that width (ora_refine(d_out = 256), ora_sim_argmax(d = 256)).
 * Any other d: SSLAM_E_UNSUPPORTED before anything is launched; NULL / misaligned / non-positive arguments: SSLAM_E_INVALID as in
 * the unsuffixed entry.  Strides stay explicit, in floats.  Outputs,
 * workspace sizes (sslam_sim_argmax_workspace_bytes, sslam_gather_refine_workspace_bytes: neither depends on d), absent pairs and
 * launch forms are those of the unsuffixed entries.  The packed refiner buffer of width d holds sslam_refiner_layout_d(...).total
 * floats: the layout of sslam_refiner_layout with out_w (d x 384, packed) and out_b (d) at the end.
 * sslam_val_frame_stats_d: descriptors (n, K, d) -> desc_mean / desc_m2 (n, d); at 256 one thread per dimension sums the K rows in
 * increasing index (at 128: two row-parity half-sums).  The bf16 throughput entries have no 256 form. */
int sslam_refiner_layout_d(int n_blocks, int d, sslam_refiner_layout_t *layout_host);
int sslam_refiner_pack_host_d(const float *const *w_host, int n_blocks, int d, float *out_host);
int sslam_refine_d(const float *x, long long rows, const float *packed, int n_blocks, float *desc, int d, void *stream);
int sslam_gather_refine_d(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed, int n_blocks,
                          float *desc, int d, void *stream);
int sslam_gather_refine_ws_d(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed, int n_blocks,
                             float *desc, void *workspace, long long workspace_bytes, int d, void *stream);
int sslam_sim_argmax_d(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2, int n_pairs,
                       int32_t *nn12, float *s12, int32_t *nn21, float *s21, float *second12, int d, void *stream);
int sslam_sim_argmax_ws_d(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2, int n_pairs,
                          int32_t *nn12, float *s12, int32_t *nn21, float *s21, float *second12, void *workspace,
                          long long workspace_bytes, int d, void *stream);
int sslam_sim_argmax_pairs_d(const float *bank, long long frame_stride, int n_bank, int K, const int32_t *pair_first,
                             const int32_t *pair_second, int n_pairs, int32_t *nn12, float *s12, int32_t *nn21, float *s21,
                             float *second12, void *workspace, long long workspace_bytes, int d, void *stream);
int sslam_sim_argmax_rows_d(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2,
                            int n_pairs, int32_t *nn12, float *s12, float *second12, int d, void *stream);
int sslam_sim_argmax_rows_pairs_d(const float *bank, long long frame_stride, int n_bank, int K, const int32_t *pair_first,
                                  const int32_t *pair_second, int n_pairs, int32_t *nn12, float *s12, float *second12, int d,
                                  void *stream);
int sslam_row_lse_d(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2, int n_pairs,
                    const float *s12, float temperature, float *lse, float *ce, float *s00, int d, void *stream);
int sslam_row_lse_pairs_d(const float *bank, long long frame_stride, int n_bank, int K, const int32_t *pair_first,
                          const int32_t *pair_second, int n_pairs, const float *s12, float temperature, float *lse, float *ce,
                          float *s00, int d, void *stream);
int sslam_val_frame_stats_d(const float *saliency, const float *pooled, const float *edge_max, const float *descriptors,
                            int n_frames, int G, int K, float *stats, float *desc_mean, float *desc_m2, int d, void *stream);

/* ---- Rank a match list by its value and keep the best `best` rows of every pair: what the reference's callers do with a
 * matcher's list (visualize_matches_sequence.py:224-225: np.argsort(-match_quality)[:max_matches], max_matches 50 from the command
 * line, 100 by default; visualize_matches.py:150-151: sorted(matches, key=similarity, reverse=True)[:max_matches]).
 * matches (n_pairs, n1, 2), value (n_pairs, n1), count (n_pairs): the outputs of sslam_match_finalize[_pairs] (value = quality) or
 * sslam_match_finalize_rule[_pairs]; only the first count[p] rows of a pair are read, count[p] clamped to [0, n1] (the arrays need
 * not come from those entries; an absent pair carries count 0).
 * THE ORDER: better value first, equal values in ascending input slot (for a finalize entry's list: ascending idx1).  Better is
 * LARGER with ascending = 0 and SMALLER with ascending = 1 (SSLAM_RULE_RATIO_SECOND's value is a cosine distance).  -0.0f and
 * +0.0f are equal; NaN rows come last in either direction, in slot order (numpy's order).  This is the reference's stable M2
 * order, and one of the orders its M1 argsort may return - the only one wherever the values are pairwise distinct.
 * With kept = min(count[p], best): out_matches (n_pairs, best, 2), out_value (n_pairs, best) and out_slot (n_pairs, best; may be
 * NULL) hold in rows 0 .. kept - 1 the kept rows, their values (the input's bits) and the input slot each came from, so that a
 * caller can gather other per-match arrays; rows kept .. best - 1 are zero; out_count[p] = kept.  The outputs are a function of the
 * inputs alone.  One launch (one 256-thread workgroup per pair, the pair on the grid's x dimension: any n_pairs), no atomics, no
 * scratch, no allocation, no host read: capturable.
 * SSLAM_E_INVALID: a NULL pointer other than out_slot; n1, n_pairs or best <= 0; best > n1; ascending not 0 or 1; an output that
 * starts where an input starts.  SSLAM_E_UNSUPPORTED: n1 > SSLAM_RANK_MAX_N1 (the keys of a pair live in 32 KB of LDS).  Every
 * refusal comes before anything is launched.  The entry reads no descriptors: it takes no width and has no _pairs form. */
#define SSLAM_RANK_MAX_N1 4096
int sslam_match_rank(const int64_t *matches, const float *value, const int32_t *count, int n1, int n_pairs, int best, int ascending,
                     int64_t *out_matches, float *out_value, int32_t *out_count, int32_t *out_slot, void *stream);

/* ---- Score a sequence against its poses: the reference's two headline quality scores, per listed frame pair.
 * sslam_pose_nn_pairs: RepeatabilityTester.compute_repeatability (test/test_repeatability.py:79-128) and
 * DescriptorQualityTester.compute_ground_truth_matches (test/test_descriptor_quality.py:144-185).
 *   kp_bank (n_bank, K, 2) fp32 pixel (x, y), what sslam_select_keypoints writes as keypoints_pixel; 8-byte aligned.  Of a pair
 *   (a, b) = (pair_first[p], pair_second[p]) - int32 DEVICE lists as in sslam_sim_argmax_pairs, an index outside [0, n_bank),
 *   -1 by convention, an ABSENT pair - the first n1 rows of frame a are the queries and the first n2 rows of frame b the
 *   candidates (n1, n2 <= K; a sequence passes n1 = n2 = K, a caller with two sets of unequal size a two-frame bank with K the
 *   larger).  H: (n_pairs, 9) float64 row-major homographies frame a -> frame b, or NULL for the raw coordinates.
 *   Per row i, all in float64, every product and sum rounded once (no contraction):
 *     X = (h00*x + h01*y) + h02, Y and W likewise from rows 1 and 2; the warped point is (X / W, Y / W);
 *     the distance to candidate j is sqrt(dx*dx + dy*dy); the nearest candidate is the LOWEST index among equal distances
 *     (numpy's argmin; duplicate keypoints of frame b tie exactly).
 *   Outputs, capacity n1 per pair as sslam_match_finalize has it:
 *     gt_matches (n_pairs, n1, 2) int64  rows (i, argmin) with distance < threshold, ascending in i; zero rows past the count;
 *     gt_count   (n_pairs) int32         their number = the reference's `repeatable` count;
 *     gt_of_row  (n_pairs, n1) int32     the argmin of row i, or -1 where the row is not within the threshold;
 *     dist_sum   (n_pairs) float64       the sum of the n1 nearest distances (the thread's rows ascending, lanes by xor 32 .. 1,
 *                                        waves in order: one order per n1), the reference's mean times n1;
 *     dist_median (n_pairs) float64      np.median of them: the mean of the two middle values of the sorted distances.
 *   An absent pair: zero rows, count 0, sum and median 0, gt_of_row -1 in every row (no row has a ground-truth partner).
 *   A row whose W is exactly 0 has an infinite distance: it is not within any threshold, and the pair's dist_sum is infinite, as
 *   numpy's.  Non-finite entries of H, NaN keypoints and 0 / 0 (W and X or Y both zero) are outside the contract, as NaN
 *   descriptors are for the matchers: the outputs stay inside their arrays and are otherwise unspecified.
 *   One launch, one workgroup per pair (frame b's points, then the sorted distances, in LDS); no atomics, no scratch, no
 *   allocation, no host read: capturable.
 * sslam_match_score_pairs: evaluate_matches (test/test_descriptor_quality.py:187-231) on a match list (matches (n_pairs, n1, 2),
 *   value (n_pairs, n1), count (n_pairs)) as sslam_match_finalize_rule[_pairs] writes it, against gt_of_row / gt_count of the
 *   entry above over the same pairs (count clamped to [0, n1]; an idx1 outside [0, n1) is a false positive):
 *     tp = rows with gt_of_row[idx1] == idx2, fp = count - tp, fn = gt_count - tp (n_pairs int32 each);
 *     value_sum (n_pairs) float64 = the sum of the first count values (M4: cosine distances), in one fixed order.
 *   PRECONDITION: idx1 is unique within the match list, as it is in gt_matches (both hold one row per query at most); then
 *   tp / fp / fn are the sizes of the reference's set intersection and differences.  One launch, capturable.
 * SSLAM_E_INVALID: a NULL pointer other than H; a non-positive size; n1 or n2 above K; a threshold that is negative, NaN or
 * infinite; a misaligned kp_bank, H or pair list.  SSLAM_E_UNSUPPORTED: K (n1 for the score entry) above SSLAM_EVAL_MAX_K.
 * Every refusal comes before anything is launched. */
#define SSLAM_EVAL_MAX_K 4096
int sslam_pose_nn_pairs(const float *kp_bank, int n_bank, int K, int n1, int n2, const int32_t *pair_first,
                        const int32_t *pair_second, int n_pairs, const double *H, double threshold, int64_t *gt_matches,
                        int32_t *gt_count, int32_t *gt_of_row, double *dist_sum, double *dist_median, void *stream);
int sslam_match_score_pairs(const int64_t *matches, const float *value, const int32_t *count, const int32_t *gt_of_row,
                            const int32_t *gt_count, int n1, int n_pairs, int32_t *tp, int32_t *fp, int32_t *fn,
                            double *value_sum, void *stream);

/* ---- The same scores against a translation-aware ground truth: depth and the full relative pose (csrc/evaluate.hip).
 * The entries above keep the reference's ground truth, H = K R K^-1 with the translation dropped; these use the D of RGB-D:
 * back-project a keypoint with its depth, move it by [R | t], project it into the other frame.  All arithmetic is float64, every
 * product, quotient and sum rounded once in the order written (no contraction).  Each entry is one launch that only enqueues:
 * no atomics, no scratch, no allocation, no host read (capturable); every refusal comes before anything is launched.
 * sslam_keypoint_depth: the depth sibling of sslam_keypoint_intensity, per frame at extraction time.
 *   depth (n, h, w) uint16, TUM's raw values; kp_pixel (n, K, 2) fp32 (x, y), 8-byte aligned; scale_x, scale_y take keypoint
 *   units to depth pixels (w / input_size and h / input_size for a pipeline's keypoints, 1 for the reference's convention).
 *     u = (double)x * scale_x, c = floor(u + 0.5); v = (double)y * scale_y, r = floor(v + 0.5);
 *   kp_depth (n, K) int32 = depth[frame][r][c], or -1 where 0 <= c < w && 0 <= r < h is false - judged on the DOUBLES, before
 *   any conversion to an integer, so a NaN or a huge coordinate gives -1.  A raw 0 stays 0: TUM's "no measurement".
 * sslam_pose_depth_nn_pairs: sslam_pose_nn_pairs with the warp replaced.  kp_bank, n_bank, K, n1, n2, the pair lists and the
 *   threshold are as there; kp_depth_bank (n_bank, K) int32 is what the entry above wrote for the same bank; T (n_pairs, 12)
 *   float64 row-major [R | t] takes camera-a coordinates to camera-b coordinates in metres (8-byte aligned, never NULL).
 *   For row i of frame a with raw depth d:
 *     u = x*scale_x, v = y*scale_y, z = d / depth_scale;
 *     X = ((u - cx) * z) / fx, Y = ((v - cy) * z) / fy, Z = z;
 *     X' = ((r00*X + r01*Y) + r02*Z) + t0, Y' and Z' likewise from rows 1 and 2;
 *     u' = (fx * X') / Z' + cx, v' = (fy * Y') / Z' + cy;  the warped keypoint is (u' / scale_x, v' / scale_y);
 *   from there the search of sslam_pose_nn_pairs bit for bit: sqrt(dx*dx + dy*dy), the LOWEST index among equal distances, the
 *   threshold in keypoint units.  A row HAS NO GROUND TRUTH when d <= 0 (no measurement, or -1 from outside the image), when
 *   Z' > 0 is false (a NaN gives false), or when -0.5 <= u' < view_w - 0.5 && -0.5 <= v' < view_h - 0.5 is false (the
 *   projection is outside frame b's view, view_w x view_h depth pixels).
 *   Outputs as sslam_pose_nn_pairs, with:
 *     gt_of_row   the argmin, -1 for a row with ground truth but no keypoint within the threshold, -2 for a row without one;
 *     valid_count (n_pairs) int32  the rows with ground truth; gt_matches and gt_count range over those rows only;
 *     dist_sum    the fixed-order sum of the valid rows' nearest distances (the order of sslam_pose_nn_pairs, an invalid row
 *                 adding +0.0);
 *     dist_median the median over the valid rows: the others sort as +inf, and it is (dist[(v-1)>>1] + dist[v>>1]) / 2 with
 *                 v = valid_count, 0.0 when v == 0.
 *   An absent pair: the absent pair's rows of sslam_pose_nn_pairs (gt_of_row -1), valid_count 0.
 *   There is no occlusion test against frame b's depth.  Non-finite entries of T and NaN keypoints in a row that passes the
 *   three tests are outside the contract, as for the entry above.
 * sslam_match_score_known_pairs: sslam_match_score_pairs that knows about -2.  unknown (n_pairs) int32 = the listed rows whose
 *   gt_of_row[idx1] == -2: such a match cannot be called wrong, so it is no false positive.  tp as before,
 *   fp = count - tp - unknown, fn = gt_count - tp; value_sum over ALL listed rows in the existing order; an idx1 outside [0, n1)
 *   stays a false positive.  With no -2 present tp / fp / fn / value_sum are those of sslam_match_score_pairs bit for bit.
 * SSLAM_E_INVALID: a NULL pointer (T included); a non-positive size; n1 or n2 above K; a threshold that is negative, NaN or
 * infinite; fx, fy, depth_scale, scale_x, scale_y, view_w or view_h not finite and positive; cx or cy not finite; a misaligned
 * pointer.  SSLAM_E_UNSUPPORTED: K (n1 for the score entry) above SSLAM_EVAL_MAX_K; n * K above 2^31 - 1 in the gather. */
int sslam_keypoint_depth(const uint16_t *depth, int n, int h, int w, const float *kp_pixel, int K, double scale_x, double scale_y,
                         int32_t *kp_depth, void *stream);
int sslam_pose_depth_nn_pairs(const float *kp_bank, const int32_t *kp_depth_bank, int n_bank, int K, int n1, int n2,
                              const int32_t *pair_first, const int32_t *pair_second, int n_pairs, const double *T, double fx, double fy,
                              double cx, double cy, double depth_scale, double scale_x, double scale_y, double view_w, double view_h,
                              double threshold, int64_t *gt_matches, int32_t *gt_count, int32_t *gt_of_row, int32_t *valid_count,
                              double *dist_sum, double *dist_median, void *stream);
int sslam_match_score_known_pairs(const int64_t *matches, const float *value, const int32_t *count, const int32_t *gt_of_row,
                                  const int32_t *gt_count, int n1, int n_pairs, int32_t *tp, int32_t *fp, int32_t *fn, int32_t *unknown,
                                  double *value_sum, void *stream);

/* ---- Geometric verification: the relative pose of every listed pair from its match list and the depths under the keypoints
 * (csrc/pose_estimate.hip).  The scoring entries above take the pose as an input; this one produces it: RANSAC over 3-point
 * samples, Horn's closed-form absolute orientation, a refit over the inliers.  All arithmetic is float64; every product, quotient,
 * sum and square root is rounded once, in the order written (no contraction); the sampler is 64-bit integer arithmetic.  One launch
 * for all pairs, one workgroup per pair, one thread per hypothesis; no atomics, no scratch, no allocation, no host read: capturable.
 *   kp_bank (n_bank, K, 2) fp32, kp_depth_bank (n_bank, K) int32, pair_first / pair_second (n_pairs) int32: as
 *   sslam_pose_depth_nn_pairs takes them (an index outside [0, n_bank) makes the pair ABSENT).  matches (n_pairs, n1, 2) int64 and
 *   count (n_pairs) int32: the lists a finalize entry or sslam_match_rank wrote, rows (idx1 in frame a, idx2 in frame b); only the
 *   first count[p] SLOTS of a pair are listed, count[p] clamped to [0, n1].  fx .. view_h as in sslam_pose_depth_nn_pairs (view_w
 *   and view_h are checked and otherwise take no part: the keypoint of frame b exists, so no view test is made); threshold in
 *   keypoint units; n_hyp hypotheses, 1 .. SSLAM_POSE_MAX_HYP; seed: any 64-bit value.
 * USABLE ROWS.  A listed slot is usable when 0 <= idx1 < K, 0 <= idx2 < K and both raw depths are > 0.  Its points are the
 *   back-projections of sslam_pose_depth_nn_pairs: for keypoint (x, y) with raw depth d,
 *     u = x*scale_x, v = y*scale_y, z = d / depth_scale;  X = ((u - cx) * z) / fx, Y = ((v - cy) * z) / fy, Z = z;
 *   X_a from frame a's keypoint idx1, X_b from frame b's keypoint idx2.  n_usable counts the usable slots; "usable row u" is the
 *   u-th of them in slot order, u = 0 .. n_usable - 1.
 * SAMPLER.  mix(x): x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31 (splitmix64's
 *   finalizer, modulo 2^64).  draw(h, k, n) = ((mix(seed + 0x9e3779b97f4a7c15 * (3*h + k + 1)) >> 32) * n) >> 32, a function of
 *   (seed, h, k) and the range alone - not of the pair's position or frames.  Hypothesis h samples the usable rows
 *     i0 = draw(h, 0, n_usable);   i1 = draw(h, 1, n_usable - 1), plus 1 if >= i0;
 *     i2 = draw(h, 2, n_usable - 2), plus 1 if >= min(i0, i1), then plus 1 if >= max(i0, i1):   three distinct rows, no rejection.
 * SOLVER, the same for a hypothesis and for the refit, over a set of rows with a stated order of sums; every sum starts from +0.0:
 *     c_a = (sum X_a) / n, c_b = (sum X_b) / n, component by component (n the number of rows, as a double);
 *     M[i][j] = sum (X_a[i] - c_a[i]) * (X_b[j] - c_b[j])                                   (i, j over x, y, z: Sxx = M[0][0], ...)
 *     N (symmetric 4 x 4):  N00 = (Sxx + Syy) + Szz   N01 = Syz - Szy           N02 = Szx - Sxz           N03 = Sxy - Syx
 *                                                     N11 = (Sxx - Syy) - Szz   N12 = Sxy + Syx           N13 = Szx + Sxz
 *                                                                               N22 = (Syy - Sxx) - Szz   N23 = Syz + Szy
 *                                                                                                         N33 = (Szz - Sxx) - Syy
 *   Cyclic Jacobi on A = N with V = I: exactly 8 sweeps over (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a rotation is skipped
 *   when a_pq == 0.0; otherwise
 *     theta = (a_qq - a_pp) / (2 * a_pq);   t = sgn / (|theta| + sqrt(theta*theta + 1)), sgn = -1 for theta < 0, else +1;
 *     c = 1 / sqrt(t*t + 1);   s = t * c;   h = t * a_pq;   a_pp = a_pp - h;   a_qq = a_qq + h;   a_pq = 0;
 *     for the two r outside {p, q}, with g = a_rp, k = a_rq (symmetric entries):  a_rp = c*g - s*k;   a_rq = s*g + c*k;
 *     for every row r of V, with g = v_rp, k = v_rq:                              v_rp = c*g - s*k;   v_rq = s*g + c*k.
 *   (w, x, y, z) = the column of V under the largest diagonal entry of A, the lowest index on equality; each divided by
 *   sqrt(((w*w + x*x) + y*y) + z*z); all four negated when w < 0.  With ww = w*w, ...:
 *     r00 = ((ww + xx) - yy) - zz   r01 = 2 * (x*y - w*z)         r02 = 2 * (x*z + w*y)
 *     r10 = 2 * (x*y + w*z)         r11 = ((ww - xx) + yy) - zz   r12 = 2 * (y*z - w*x)
 *     r20 = 2 * (x*z - w*y)         r21 = 2 * (y*z + w*x)         r22 = ((ww - xx) - yy) + zz
 *     t_i = c_b[i] - ((r_i0 * c_a[0] + r_i1 * c_a[1]) + r_i2 * c_a[2]).
 *   A hypothesis sums its three rows in the order i0, i1, i2: ((0 + r0) + r1) + r2.  No transcendental function anywhere.
 * SCORE of a pose [R | t] on a usable row: X', Y', Z', u', v' from X_a by the formulas of sslam_pose_depth_nn_pairs;
 *   dx = u' / scale_x - x_b, dy = v' / scale_y - y_b against frame b's keypoint; s = dx*dx + dy*dy; the row is an INLIER iff
 *   Z' > 0 and sqrt(s) < threshold (a NaN fails both).  A pose with a non-finite entry has no inliers.
 *   The best hypothesis has the most inliers, the lowest h on equality.
 * REFIT, when the best hypothesis has 3 inliers at least: the solver over its inliers, n = their number.  THE ORDER of each sum:
 *   thread t of 256 adds, from +0.0, the terms of the usable rows t, t + 256, t + 512, ... ascending, a row that is no inlier
 *   adding +0.0; then lanes by xor 32 .. 1 within each wave of 64; then the four waves, ((w0 + w1) + w2) + w3: one order per
 *   n_usable, whatever n_hyp.  The refit is scored; it is KEPT iff its inlier count is >= the hypothesis'; else the hypothesis stays.
 * Outputs, per pair:
 *     T (n_pairs, 12) float64         [R | t] row-major, camera a -> camera b, as sslam_pose_depth_nn_pairs takes it;
 *     inlier_count, usable_count, best_hypothesis, refit_kept (n_pairs) int32 each: the inliers of T, n_usable, h, 0 or 1;
 *     inlier_of_slot (n_pairs, n1) int32    per slot: 1 an inlier of T, 0 not, -1 listed but not usable; 0 past the count;
 *     rms (n_pairs) float64           sqrt((sum s) / inlier_count) over the inliers of T, the sum in the refit's order; 0 without.
 *   NO POSE - an absent pair (no slot is usable: the whole mask is 0) or n_usable < 3: T = [I | 0], inlier_count 0,
 *   usable_count = n_usable, best_hypothesis -1, refit_kept 0, rms 0; the mask is 0 in the usable slots, -1 in the other listed ones.
 *   A pair's outputs are a function of that pair's rows, the camera, the threshold, n_hyp and the seed alone.  NaN keypoints under
 *   a positive depth are outside the contract, as for the entries above: the outputs stay inside their arrays.
 * SSLAM_E_INVALID: a NULL or misaligned pointer; a non-positive size; n1 above K; n_hyp outside 1 .. SSLAM_POSE_MAX_HYP; a threshold
 * that is negative, NaN or infinite; fx, fy, depth_scale, scale_x, scale_y, view_w or view_h not finite and positive; cx or cy not
 * finite.  SSLAM_E_UNSUPPORTED: K above SSLAM_EVAL_MAX_K.  Every refusal comes before anything is launched. */
#define SSLAM_POSE_MAX_HYP 1024
int sslam_pose_ransac_pairs(const float *kp_bank, const int32_t *kp_depth_bank, int n_bank, int K, const int32_t *pair_first,
                            const int32_t *pair_second, int n_pairs, const int64_t *matches, const int32_t *count, int n1, double fx,
                            double fy, double cx, double cy, double depth_scale, double scale_x, double scale_y, double view_w,
                            double view_h, double threshold, int n_hyp, uint64_t seed, double *T, int32_t *inlier_count,
                            int32_t *usable_count, int32_t *best_hypothesis, int32_t *refit_kept, int32_t *inlier_of_slot, double *rms,
                            void *stream);

/* ---- Pose refinement: robust Gauss-Newton on the reprojection error (csrc/pose_refine.hip).  The entry above ends in one Horn
 * solve, a 3-D point-to-point fit in which every inlier pulls equally; this one takes ANY initial pose of a pair - the entry's own,
 * a motion model's prediction, a pose from elsewhere - and minimises the Huber cost of the reprojection into frame b over the rows
 * that pose agrees with.  All arithmetic is float64: + - * / sqrt only, every operation rounded once in the order written (no
 * contraction), no transcendental function.  One launch for all pairs, one 256-thread workgroup per pair; no atomics, no scratch,
 * no allocation, no host read: capturable.  Results are written with ordinary stores.
 *   kp_bank .. threshold: the arguments of sslam_pose_ransac_pairs without n_hyp and seed, with the same meaning.
 *   T_in (n_pairs, 12) float64, 8-byte aligned: the initial [R | t] of every pair, row-major, camera a -> camera b.
 *   huber: finite and > 0, in keypoint units.   n_iter: the most Gauss-Newton steps, 0 .. SSLAM_REFINE_MAX_ITER.
 * USABLE ROWS: those of sslam_pose_ransac_pairs, in slot order; X_a, and frame b's keypoint (x_b, y_b), of usable row u.
 * SELECTED ROWS: the usable rows that are inliers of T_in by that entry's SCORE (Z' > 0 and sqrt(s) < threshold; a T_in with a
 *   non-finite entry has none).  They are fixed for the whole call.
 * ONE ROW under a pose [R | t], with kx = fx / scale_x and ky = fy / scale_y:
 *     X', Y', Z', u', v' from X_a by the formulas of sslam_pose_depth_nn_pairs;
 *     rx = u' / scale_x - x_b;   ry = v' / scale_y - y_b;   s = rx*rx + ry*ry;   d = sqrt(s);
 *     if d <= huber:  w = 1, rho = s;   otherwise (a NaN included):  w = huber / d,  rho = (2 * huber) * d - huber * huber;
 *     iz = 1 / Z';   a = kx * iz;   b = ky * iz;   c = -(a * (X' * iz));   e = -(b * (Y' * iz));
 *     Ju = (a, 0, c, c*Y', a*Z' - c*X', -(a*Y'));      Jv = (0, b, e, e*Y' - b*Z', -(e*X'), b*X');
 *   the rows of the 2 x 6 Jacobian of (rx, ry) in the LEFT perturbation X'' = X' + v + w x X' (camera b), parameters
 *   (vx, vy, vz, wx, wy, wz): the projection's 2 x 3 Jacobian at X' times [I | -[X']x].  The two zeros are +0.0 and are
 *   multiplied like any other entry.  The row's 28 terms:
 *     rho;    H_ij = w * (Ju[i]*Ju[j] + Jv[i]*Jv[j]) for i <= j, row-major (21);    g_i = w * (Ju[i]*rx + Jv[i]*ry) (6).
 * ONE PASS at a pose: cost = sum rho, H = sum H_ij, g = sum g_i over the selected rows, each of the 28 sums in THE ORDER of the
 *   entry above's refit - thread t of 256 adds, from +0.0, the terms of the usable rows t, t + 256, ... ascending, a usable row that
 *   is not selected adding +0.0; lanes by xor 32 .. 1; the four waves ((w0 + w1) + w2) + w3 - and `behind`, the number of selected
 *   rows whose Z' > 0 is false.
 * STEP from the totals of the pass at the current pose, H read as symmetric: an unpivoted LDL^T,
 *     for j = 0 .. 5:   D_j = H_jj, then for k = 0 .. j-1 ascending  D_j = D_j - (L_jk * L_jk) * D_k;
 *                       for i = j+1 .. 5:  L_ij = H_ij, then for k = 0 .. j-1 ascending  L_ij = L_ij - (L_ik * L_jk) * D_k;  L_ij = L_ij / D_j;
 *     y_i = -g_i, then for k = 0 .. i-1 ascending  y_i = y_i - L_ik * y_k                                       (i = 0 .. 5);
 *     delta_i = y_i / D_i, then for k = i+1 .. 5 ascending  delta_i = delta_i - L_ki * delta_k                  (i = 5 .. 0).
 *   A pivot D_j that is not finite and > 0 ENDS the iteration.  delta = (vx, vy, vz, wx, wy, wz).  The update:
 *     w = 1, x = 0.5 * wx, y = 0.5 * wy, z = 0.5 * wz;  each divided by sqrt(((w*w + x*x) + y*y) + z*z);  dR = r00 .. r22 of the
 *     entry above's quaternion formulas;
 *     R_ij <- (dR_i0 * R_0j + dR_i1 * R_1j) + dR_i2 * R_2j;       t_i <- ((dR_i0 * t_0 + dR_i1 * t_1) + dR_i2 * t_2) + v_i.
 * ITERATION.  Pass 0 at T_in gives cost_in.  Up to n_iter times: a step from the current pose gives a trial pose; the pass at the
 *   trial; the trial is ACCEPTED - becomes the current pose, its totals the current totals - iff its cost is finite, its `behind`
 *   is 0 and its cost < the current cost.  The first trial that is not accepted ends the iteration: n_iter + 1 passes at most.
 * KEEP RULE.  With a step accepted, the current pose is scored over ALL usable rows at `threshold` (a pose with a non-finite entry
 *   has no inliers); it is returned iff its inlier count >= T_in's (the number of selected rows).  Otherwise T = T_in.
 * Outputs, per pair:
 *     T (n_pairs, 12) float64             the returned pose;
 *     status (n_pairs) int32              0 refined and returned;  1 no step accepted (n_iter 0, a minimum already, a pivot that
 *                                         is not positive, the first trial rejected);  2 steps accepted but the result has fewer
 *                                         inliers than T_in and is not kept;  3 not attempted: an absent pair, a non-finite entry
 *                                         in T_in, or fewer than 3 selected rows;
 *     iterations (n_pairs) int32          the accepted steps (also under status 2);
 *     selected_count, usable_count, inlier_count_in, inlier_count (n_pairs) int32: the selected rows, n_usable, the inliers of
 *                                         T_in (= selected_count) and of T over the usable rows;
 *     inlier_of_slot (n_pairs, n1) int32  the entry above's encoding, for T;
 *     cost_in, cost (n_pairs) float64     the pass' cost at T_in and at T (cost = cost_in under status 1 and 2);
 *     rms (n_pairs) float64               the entry above's, for T;
 *     info (n_pairs, 21) float64          the upper triangle of the pass' H at T, row-major: the information matrix of the
 *                                         pose in the perturbation's parameters, in keypoint units^-2 (unit residual weight).
 *   Under status 1, 2 and 3 T = T_in bit for bit.  Under status 3 all six counts, cost_in, cost, rms and info are 0 and the mask is
 *   the entry above's NO POSE mask.  A pair's outputs are a function of that pair's rows, its T_in row, the camera, threshold, huber
 *   and n_iter alone.  T and T_in are different arrays.  NaN keypoints under a positive depth are outside the contract, as above.
 * SSLAM_E_INVALID: the entry above's list (n_hyp apart), plus: huber not finite and > 0; n_iter outside 0 .. SSLAM_REFINE_MAX_ITER; a
 * NULL or misaligned T_in.  SSLAM_E_UNSUPPORTED: K above SSLAM_EVAL_MAX_K.  Every refusal comes before anything is launched. */
#define SSLAM_REFINE_MAX_ITER 16
int sslam_pose_refine_pairs(const float *kp_bank, const int32_t *kp_depth_bank, int n_bank, int K, const int32_t *pair_first,
                            const int32_t *pair_second, int n_pairs, const int64_t *matches, const int32_t *count, int n1, double fx,
                            double fy, double cx, double cy, double depth_scale, double scale_x, double scale_y, double view_w,
                            double view_h, double threshold, const double *T_in, double huber, int n_iter, double *T, int32_t *status,
                            int32_t *iterations, int32_t *selected_count, int32_t *usable_count, int32_t *inlier_count_in,
                            int32_t *inlier_count, int32_t *inlier_of_slot, double *cost_in, double *cost, double *rms, double *info,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif
