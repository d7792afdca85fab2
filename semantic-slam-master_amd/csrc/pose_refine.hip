// pose_refine.hip - pose refinement: robust Gauss-Newton on the reprojection error of a pair's match list, from any initial pose.
//   sslam_pose_refine_pairs  per listed pair: the usable rows that are inliers of T_in are SELECTED once; up to n_iter Gauss-Newton
//                            steps on the Huber cost of their reprojection into frame b (left perturbation in camera b, an
//                            unpivoted 6 x 6 LDL^T, a quaternion update without sine or cosine), each step kept only if the cost
//                            falls; the result is returned if it has no fewer inliers than T_in; the pose, the counts, the mask,
//                            the costs and the 6 x 6 information matrix.
// All arithmetic is float64 in the order include/sslam_hip.h states (-ffp-contract=off).
// One 256-thread workgroup per pair.  A thread owns the usable rows t, t + 256, ... (16 at most): whether each is selected is one bit
// of a register, its 28 partial sums (cost, 21 of H, 6 of g) live in registers, and the first POSE_CHUNK usable rows - X_a as three
// doubles and frame b's keypoint, 32 KB of LDS - are staged once; rows past the chunk are read again from global memory every pass.
// Every thread solves the 6 x 6 system from the same totals.  No atomics, no scratch, no allocation, no host read: capturable.
#include "pose_refine_common.h"

namespace {

// the body, the sums, the solve and the update stand in pose_refine_common.h, shared with the weighted kernel of csrc_weight/
__global__ __launch_bounds__(POSE_THREADS) void pose_refine_kernel(const float *__restrict__ kp_bank, const int *__restrict__ kp_depth_bank,
                                                            int n_bank, int K, const int *__restrict__ pair_first,
                                                            const int *__restrict__ pair_second, const long long *__restrict__ matches,
                                                            const int *__restrict__ count, int n1, PoseCamera cam, double threshold,
                                                            const double *T_in, double huber, int n_iter,
                                                            double *T_out, int *__restrict__ status,
                                                            int *__restrict__ iterations, int *__restrict__ selected_count,
                                                            int *__restrict__ usable_count, int *__restrict__ inlier_count_in,
                                                            int *__restrict__ inlier_count, int *__restrict__ inlier_of_slot,
                                                            double *__restrict__ cost_in, double *__restrict__ cost_out,
                                                            double *__restrict__ rms, double *__restrict__ info) {
    pose_refine_body<false>(kp_bank, kp_depth_bank, n_bank, K, pair_first, pair_second, matches, count, n1, cam, threshold, T_in, huber, n_iter,
                            nullptr, T_out, status, iterations, selected_count, usable_count, inlier_count_in, inlier_count, inlier_of_slot,
                            cost_in, cost_out, rms, info, nullptr);
}

}  // namespace

extern "C" int sslam_pose_refine_pairs(const float *kp_bank, const int32_t *kp_depth_bank, int n_bank, int K, const int32_t *pair_first,
                                       const int32_t *pair_second, int n_pairs, const int64_t *matches, const int32_t *count, int n1,
                                       double fx, double fy, double cx, double cy, double depth_scale, double scale_x, double scale_y,
                                       double view_w, double view_h, double threshold, const double *T_in, double huber, int n_iter,
                                       double *T, int32_t *status, int32_t *iterations, int32_t *selected_count, int32_t *usable_count,
                                       int32_t *inlier_count_in, int32_t *inlier_count, int32_t *inlier_of_slot, double *cost_in,
                                       double *cost, double *rms, double *info, void *stream) {
    if (!pose_args_ok(kp_bank, kp_depth_bank, pair_first, pair_second, fx, fy, cx, cy, depth_scale, scale_x, scale_y, view_w, view_h,
                      threshold))
        return SSLAM_E_INVALID;
    if (!matches || !count || !T_in || !T || !status || !iterations || !selected_count || !usable_count || !inlier_count_in ||
        !inlier_count || !inlier_of_slot || !cost_in || !cost || !rms || !info)
        return SSLAM_E_INVALID;
    if (n_bank <= 0 || K <= 0 || n1 <= 0 || n_pairs <= 0 || n1 > K) return SSLAM_E_INVALID;
    if (n_iter < 0 || n_iter > REFINE_MAX_ITER || !finite_positive(huber)) return SSLAM_E_INVALID;
    if (sslam_misaligned(8, matches, T_in, T, cost_in, cost, rms, info) ||
        sslam_misaligned(4, count, status, iterations, selected_count, usable_count, inlier_count_in, inlier_count, inlier_of_slot))
        return SSLAM_E_INVALID;
    if (K > POSE_MAX_N1) return SSLAM_E_UNSUPPORTED;
    const PoseCamera cam = {fx, fy, cx, cy, depth_scale, scale_x, scale_y};
    hipLaunchKernelGGL(pose_refine_kernel, dim3((unsigned)n_pairs), dim3(POSE_THREADS), 0, (hipStream_t)stream, kp_bank, kp_depth_bank, n_bank,
                       K, pair_first, pair_second, (const long long *)matches, count, n1, cam, threshold, T_in, huber, n_iter, T, status,
                       iterations, selected_count, usable_count, inlier_count_in, inlier_count, inlier_of_slot, cost_in, cost, rms, info);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}
