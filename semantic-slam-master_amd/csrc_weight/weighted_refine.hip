// weighted_refine.hip - libsslam_weight.so: per-match weights from keypoint confidences, and the pose refinement that takes them.
//   sslu_match_weights               one thread per match slot: the two confidences gathered, their product or the inverted
//                                    expected-error form; +0.0f for a slot that holds no match.  Coalesced stores.
//   sslu_pose_refine_weighted_pairs  sslam_pose_refine_pairs' workgroup body (../csrc/pose_refine_common.h) instantiated with
//                                    weights: a row's weight multiplies its Huber terms, a row whose weight is not finite and > 0
//                                    is not selected.  The weights of the first POSE_CHUNK usable rows stand in LDS beside the
//                                    rows (4 KB more, 45968 bytes static in all); later rows read theirs from global memory.
// All arithmetic is in the order include/sslam_weight.h states (-ffp-contract=off).  No atomics, no scratch, no allocation, no
// host read: both entries are capturable.
#include "../csrc/pose_refine_common.h"

#include "../../include/sslam_weight.h"

namespace {

long long g_launches = 0;   // diagnostic launch counter (sslu_launch_count): relaxed atomic adds, the library's only mutable state

constexpr int WEIGHT_THREADS = 256;

__global__ __launch_bounds__(WEIGHT_THREADS) void match_weights_kernel(const float *__restrict__ conf_bank, int n_bank, int K,
                                                                      const int *__restrict__ pair_first,
                                                                      const int *__restrict__ pair_second,
                                                                      const long long *__restrict__ matches, const int *__restrict__ count,
                                                                      int n1, long long total, int mode, double s2,
                                                                      float *__restrict__ weight) {
    const long long i = (long long)blockIdx.x * WEIGHT_THREADS + threadIdx.x;
    if (i >= total) return;
    const long long p = i / n1;
    const int slot = (int)(i - p * n1);
    const int a = pair_first[p], b = pair_second[p];
    const bool present = (unsigned)a < (unsigned)n_bank && (unsigned)b < (unsigned)n_bank;      // pose_pair's rule
    const int cnt = count[p];
    const int c = cnt < 0 ? 0 : (cnt > n1 ? n1 : cnt);
    float w = 0.0f;
    if (present && slot < c) {
        const long long i1 = matches[2 * i], i2 = matches[2 * i + 1];
        if (i1 >= 0 && i1 < K && i2 >= 0 && i2 < K) {
            const float c1 = conf_bank[(long long)a * K + i1], c2 = conf_bank[(long long)b * K + i2];
            if (mode == SSLU_WEIGHT_PRODUCT) {
                w = c1 * c2;
            } else {
                const double e1 = 1.0 / ((double)c1 + 1e-6) - 1.0, e2 = 1.0 / ((double)c2 + 1e-6) - 1.0;
                w = (float)(s2 / ((s2 + e1 * e1) + e2 * e2));
            }
        }
    }
    weight[i] = w;
}

__global__ __launch_bounds__(POSE_THREADS) void pose_refine_weighted_kernel(
    const float *__restrict__ kp_bank, const int *__restrict__ kp_depth_bank, int n_bank, int K, const int *__restrict__ pair_first,
    const int *__restrict__ pair_second, const long long *__restrict__ matches, const int *__restrict__ count, int n1, PoseCamera cam,
    double threshold, const double *T_in, double huber, int n_iter, const float *__restrict__ weight, double *T_out,
    int *__restrict__ status, int *__restrict__ iterations, int *__restrict__ selected_count, int *__restrict__ usable_count,
    int *__restrict__ inlier_count_in, int *__restrict__ inlier_count, int *__restrict__ inlier_of_slot, double *__restrict__ cost_in,
    double *__restrict__ cost_out, double *__restrict__ rms, double *__restrict__ info, double *__restrict__ weight_sum) {
    pose_refine_body<true>(kp_bank, kp_depth_bank, n_bank, K, pair_first, pair_second, matches, count, n1, cam, threshold, T_in, huber, n_iter,
                           weight, T_out, status, iterations, selected_count, usable_count, inlier_count_in, inlier_count, inlier_of_slot,
                           cost_in, cost_out, rms, info, weight_sum);
}

}  // namespace

extern "C" int sslu_version(void) { return 100; }
extern "C" const char *sslu_arch(void) { return "gfx950"; }
extern "C" long long sslu_launch_count(void) { return __atomic_load_n(&g_launches, __ATOMIC_RELAXED); }

extern "C" int sslu_match_weights(const float *conf_bank, int n_bank, int K, const int32_t *pair_first, const int32_t *pair_second,
                                  int n_pairs, const int64_t *matches, const int32_t *count, int n1, int mode, double sigma0,
                                  float *weight, void *stream) {
    if (!conf_bank || !pair_first || !pair_second || !matches || !count || !weight) return SSLAM_E_INVALID;
    if (n_bank <= 0 || K <= 0 || n_pairs <= 0 || n1 <= 0) return SSLAM_E_INVALID;
    if (mode != SSLU_WEIGHT_PRODUCT && mode != SSLU_WEIGHT_EXPECTED_ERROR) return SSLAM_E_INVALID;
    if (mode == SSLU_WEIGHT_EXPECTED_ERROR && !finite_positive(sigma0)) return SSLAM_E_INVALID;
    if (sslam_misaligned(8, matches) || sslam_misaligned(4, conf_bank, pair_first, pair_second, count, weight)) return SSLAM_E_INVALID;
    const long long total = (long long)n_pairs * n1;
    if (total > 0x7fffffffLL) return SSLAM_E_UNSUPPORTED;
    const double s2 = mode == SSLU_WEIGHT_EXPECTED_ERROR ? sigma0 * sigma0 : 0.0;
    const unsigned blocks = (unsigned)((total + WEIGHT_THREADS - 1) / WEIGHT_THREADS);
    hipLaunchKernelGGL(match_weights_kernel, dim3(blocks), dim3(WEIGHT_THREADS), 0, (hipStream_t)stream, conf_bank, n_bank, K, pair_first,
                       pair_second, (const long long *)matches, count, n1, total, mode, s2, weight);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}

extern "C" int sslu_pose_refine_weighted_pairs(const float *kp_bank, const int32_t *kp_depth_bank, int n_bank, int K,
                                               const int32_t *pair_first, const int32_t *pair_second, int n_pairs, const int64_t *matches,
                                               const int32_t *count, int n1, double fx, double fy, double cx, double cy,
                                               double depth_scale, double scale_x, double scale_y, double view_w, double view_h,
                                               double threshold, const double *T_in, double huber, int n_iter, const float *weight,
                                               double *T, int32_t *status, int32_t *iterations, int32_t *selected_count,
                                               int32_t *usable_count, int32_t *inlier_count_in, int32_t *inlier_count,
                                               int32_t *inlier_of_slot, double *cost_in, double *cost, double *rms, double *info,
                                               double *weight_sum, void *stream) {
    if (!pose_args_ok(kp_bank, kp_depth_bank, pair_first, pair_second, fx, fy, cx, cy, depth_scale, scale_x, scale_y, view_w, view_h,
                      threshold))
        return SSLAM_E_INVALID;
    if (!matches || !count || !T_in || !weight || !T || !status || !iterations || !selected_count || !usable_count || !inlier_count_in ||
        !inlier_count || !inlier_of_slot || !cost_in || !cost || !rms || !info || !weight_sum)
        return SSLAM_E_INVALID;
    if (n_bank <= 0 || K <= 0 || n1 <= 0 || n_pairs <= 0 || n1 > K) return SSLAM_E_INVALID;
    if (n_iter < 0 || n_iter > REFINE_MAX_ITER || !finite_positive(huber)) return SSLAM_E_INVALID;
    if (sslam_misaligned(8, matches, T_in, T, cost_in, cost, rms, info, weight_sum) ||
        sslam_misaligned(4, count, weight, status, iterations, selected_count, usable_count, inlier_count_in, inlier_count, inlier_of_slot))
        return SSLAM_E_INVALID;
    if (K > POSE_MAX_N1) return SSLAM_E_UNSUPPORTED;
    const PoseCamera cam = {fx, fy, cx, cy, depth_scale, scale_x, scale_y};
    hipLaunchKernelGGL(pose_refine_weighted_kernel, dim3((unsigned)n_pairs), dim3(POSE_THREADS), 0, (hipStream_t)stream, kp_bank,
                       kp_depth_bank, n_bank, K, pair_first, pair_second, (const long long *)matches, count, n1, cam, threshold, T_in, huber,
                       n_iter, weight, T, status, iterations, selected_count, usable_count, inlier_count_in, inlier_count, inlier_of_slot,
                       cost_in, cost, rms, info, weight_sum);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);
    return SSLAM_OK;
}
