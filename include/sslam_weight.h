/*
 * sslam_weight.h - C ABI of libsslam_weight.so: the eighth native library of the project (gfx950), confidence-weighted pose
 * refinement - the consumer of the keypoint confidence of sslam_conf.h.  The reference's UncertaintyEstimator says what its output
 * is for ("Used to weight features in bundle adjustment", semantic-slam/models/uncertainty_estimator.py); here a per-match weight
 * made of the two keypoints' confidences multiplies that match's terms in the robust Gauss-Newton of sslam_pose_refine_pairs, and
 * reaches every later stage through the 6 x 6 information matrix.
 * Same conventions as sslam_hip.h / sslam_conf.h: every pointer is a CALLER-OWNED DEVICE pointer, the library never allocates,
 * frees, synchronises or reads back; `stream` is a hipStream_t passed as void*; the return value is SSLAM_OK or a negative
 * SSLAM_E_* code of sslam_hip.h; every refusal comes before anything is launched and writes nothing.  Results are written with
 * ordinary vector stores; there is no workspace, there are no atomics and there is no scratch: both entries only enqueue and can
 * be captured in a graph.  Built with -ffp-contract=off and the correctly rounded divide and sqrt: every operation is rounded once
 * in the order written, and a result is the same bits as tests/weighted_refine_ref.py.  The entries carry the prefix sslu_.
 */
#ifndef SSLAM_WEIGHT_H
#define SSLAM_WEIGHT_H

#include <stdint.h>

#include "sslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ALIGNMENT, every entry that takes device pointers: the LEAST alignment in bytes of each pointer argument - the widest access
 * the entry's kernel makes to it.  A pointer that misses its alignment: SSLAM_E_INVALID before anything is launched, nothing
 * written.  A result is a function of the operands' values, not of their addresses (tests/test_gpu_weighted_refine.py runs every
 * pointer at its least alignment, just past and just before a 256-byte boundary).  No entry takes a stride.
 *   sslu_match_weights: conf_bank 4, pair_first 4, pair_second 4, matches 8, count 4, weight 4
 *   sslu_pose_refine_weighted_pairs: kp_bank 8, kp_depth_bank 4, pair_first 4, pair_second 4, matches 8, count 4, T_in 8, weight 4, T 8, status 4, iterations 4, selected_count 4, usable_count 4, inlier_count_in 4, inlier_count 4, inlier_of_slot 4, cost_in 8, cost 8, rms 8, info 8, weight_sum 8
 */

/* ---- SIZE LIMITS: the expressions the dispatch code tests, the code returned where one is false, and the widths in bits of the
 * kernels' index expressions (tests/weight_table.py restates them, tests/test_weighted_refine_cpu.py holds the header to the table).
 *   sslu_match_weights: n_pairs * n1 <= 0x7fffffff, else SSLAM_E_UNSUPPORTED. offsets: slot index pair * n1 64, frame * K 64
 *   sslu_pose_refine_weighted_pairs: n1 <= K, else SSLAM_E_INVALID; K <= 4096, else SSLAM_E_UNSUPPORTED. offsets: pair * n1 64, frame * K 64
 */

int sslu_version(void);
const char *sslu_arch(void);          /* "gfx950" */
long long sslu_launch_count(void);    /* kernels this library has launched in this process - a launch that returned
                                         SSLAM_E_LAUNCH is not counted (diagnostic; relaxed atomic) */

#define SSLU_WEIGHT_PRODUCT 0         /* w = c1 * c2 */
#define SSLU_WEIGHT_EXPECTED_ERROR 1  /* w = sigma0^2 / (sigma0^2 + e1^2 + e2^2), e = 1 / (c + 1e-6) - 1 */

/* ---- Per-match weights from per-keypoint confidences: conf_bank (n_bank, K) fp32, the pair list and the match lists of
 * sslam_pose_refine_pairs (pair_first, pair_second (n_pairs) int32; matches (n_pairs, n1, 2) int64; count (n_pairs) int32)
 * -> weight (n_pairs, n1) fp32, aligned with the match slots.  EVERY element of weight is written.
 *   Slot j of pair p is +0.0f when it holds no match: j >= count[p] clamped to [0, n1]; an index i1 or i2 outside [0, K); a pair
 *   that is absent by sslam_pose_refine_pairs' rule (a frame index outside [0, n_bank)).
 *   Otherwise, with c1 = conf_bank[pair_first[p]][i1] and c2 = conf_bank[pair_second[p]][i2]:
 *     SSLU_WEIGHT_PRODUCT:         w = c1 * c2                                            (one fp32 multiply)
 *     SSLU_WEIGHT_EXPECTED_ERROR:  in float64, per side  e = 1.0 / ((double)c + 1e-6) - 1.0  - the error at which
 *                                  compute_expected_error_loss is least, its confidence 1 / (1 + error) inverted with that
 *                                  function's own epsilon;  s2 = sigma0 * sigma0;
 *                                  w = s2 / ((s2 + e1*e1) + e2*e2), rounded once to fp32.
 *   No transcendental function.  Nothing depends on depth.  A NaN confidence gives a NaN weight, which the refinement below
 *   does not select.  A slot's weight is a function of that slot's two confidences, the mode and sigma0 alone.
 * Launch: one kernel, one thread per slot, coalesced stores; the two gathers are the only scattered accesses.
 * SSLAM_E_INVALID: a NULL pointer; n_bank, K, n_pairs or n1 <= 0; a mode that is neither of the two; sigma0 not finite and > 0 under
 * SSLU_WEIGHT_EXPECTED_ERROR (it is ignored under SSLU_WEIGHT_PRODUCT); a pointer that misses its alignment.
 * SSLAM_E_UNSUPPORTED: n_pairs * n1 above 2^31 - 1. */
int sslu_match_weights(const float *conf_bank, int n_bank, int K, const int32_t *pair_first, const int32_t *pair_second, int n_pairs,
                       const int64_t *matches, const int32_t *count, int n1, int mode, double sigma0, float *weight, void *stream);

/* ---- Weighted pose refinement (csrc_weight/weighted_refine.hip; the kernel body is csrc/pose_refine_common.h, shared with
 * sslam_pose_refine_pairs).  The arguments of sslam_pose_refine_pairs plus two:
 *   weight (n_pairs, n1) float32, 4-byte aligned: the weight g of every match slot;
 *   weight_sum (n_pairs) float64, 8-byte aligned: one more output.
 * The statement is sslam_pose_refine_pairs' (include/sslam_hip.h) with exactly these differences:
 * 1. COUNTS.  A usable row is GEOMETRICALLY IN if it is an inlier of T_in at `threshold` by that entry's SCORE.
 *    inlier_count_in counts those rows.
 * 2. SELECTED ROWS: the rows that are geometrically in and whose weight satisfies g > 0 && g - g == 0 in fp32 - a NaN, either
 *    infinity, either zero and a negative weight are not selected, a subnormal is.  selected_count counts the selected rows.
 *    Fewer than 3 selected rows: status 3.  Under status 3 every shared output holds exactly what sslam_pose_refine_pairs writes
 *    under its status 3 (T = T_in, all six counts - inlier_count_in too -, cost_in, cost, rms and info 0, the NO POSE mask),
 *    and weight_sum is 0.
 * 3. TERMS.  Per selected row, with Huber's w and rho of the raw pixel residual as there, and gw = (double)g * w:
 *      cost += (double)g * rho;    H_ij += gw * (Ju[i]*Ju[j] + Jv[i]*Jv[j]);    g_i += gw * (Ju[i]*rx + Jv[i]*ry);
 *    each of the 28 sums in THE ORDER stated there.  Huber acts on the raw residual, not on a weighted one.
 * 4. WEIGHT SUM.  weight_sum = the sum of (double)g over the selected rows, in the same order: thread t of 256 adds, from +0.0,
 *    the usable rows t, t + 256, ... ascending, a row that is not selected adding +0.0; lanes by xor 32 .. 1; the four waves
 *    ((w0 + w1) + w2) + w3.
 * 5. KEEP RULE.  The refined pose is returned iff its inlier count over ALL usable rows >= inlier_count_in.  inlier_of_slot,
 *    inlier_count and rms stay geometric and unweighted.
 * Two consequences:
 *   With every weight exactly 1.0f, all shared outputs equal sslam_pose_refine_pairs' byte for byte (1.0 * w = w), and
 *   weight_sum = selected_count.
 *   Scaling every weight by a power of two leaves T, status, iterations, the counts, the mask and rms byte-identical and scales
 *   cost_in, cost, info and weight_sum exactly (no product overflowing or leaving the normal range).
 * info is then the information matrix in keypoint units^-2 times the weights' unit: the banded graph, the sparse graph and the
 * window read it as they read the unweighted one.
 * Launch: one kernel, one 256-thread workgroup per pair; the weights of the first 1024 usable rows stand in LDS beside the rows
 * (45968 bytes static), later rows read theirs from global memory each pass; no atomics, no scratch: capturable.
 * A pair's outputs are a function of that pair's rows, their weights, its T_in row, the camera, threshold, huber and n_iter alone.
 * SSLAM_E_INVALID: sslam_pose_refine_pairs' list (n1 > K among it), plus a NULL or misaligned weight or weight_sum.
 * SSLAM_E_UNSUPPORTED: K above SSLAM_EVAL_MAX_K.  Every refusal comes before anything is launched. */
int sslu_pose_refine_weighted_pairs(const float *kp_bank, const int32_t *kp_depth_bank, int n_bank, int K, const int32_t *pair_first,
                                    const int32_t *pair_second, int n_pairs, const int64_t *matches, const int32_t *count, int n1,
                                    double fx, double fy, double cx, double cy, double depth_scale, double scale_x, double scale_y,
                                    double view_w, double view_h, double threshold, const double *T_in, double huber, int n_iter,
                                    const float *weight, double *T, int32_t *status, int32_t *iterations, int32_t *selected_count,
                                    int32_t *usable_count, int32_t *inlier_count_in, int32_t *inlier_count, int32_t *inlier_of_slot,
                                    double *cost_in, double *cost, double *rms, double *info, double *weight_sum, void *stream);

#ifdef __cplusplus
}
#endif
#endif
