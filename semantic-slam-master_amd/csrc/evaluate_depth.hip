// evaluate_depth.hip - the scoring stage of evaluate.hip against a translation-aware ground truth: depth and the full pose.
//   sslam_keypoint_depth           the raw uint16 depth under every keypoint of a frame (the depth sibling of A9), -1 outside;
//   sslam_pose_depth_nn_pairs      sslam_pose_nn_pairs with the homography replaced by back-projection with the keypoint's depth,
//                                  the rigid transform [R | t] and projection into the other frame; a row without a measurement,
//                                  behind the other camera or outside its view HAS NO GROUND TRUTH (gt_of_row = -2);
//   sslam_match_score_known_pairs  sslam_match_score_pairs that counts the listed rows on -2 apart instead of as false positives.
// All arithmetic is float64 in the order include/sslam_hip.h states (-ffp-contract=off).  The search, the compaction and the
// sort are those of pose_nn_kernel (evaluate.hip), restated here so that the older entry's translation unit - whose bits its
// tests pin - stays as it is; what differs is the warp and the validity flag that rides through every later step.
// No atomics, no scratch, no allocation, no host read: all three launches can be captured.
#include "common.h"

namespace {

constexpr int EVAL_MAX_K = SSLAM_EVAL_MAX_K;
constexpr int EVAL_ROWS = 4;            // rows of frame a a thread carries in registers: EVAL_MAX_K / 1024
constexpr int EVAL_MAX_WAVES = 16;      // of a 1024-thread workgroup
static_assert(EVAL_ROWS * 1024 >= EVAL_MAX_K, "a workgroup's threads must cover every row");

inline int eval_threads(int n1) { return n1 <= 256 * EVAL_ROWS ? 256 : 1024; }
__host__ __device__ inline int eval_pow2(int n) {
    int P = 1;
    while (P < n) P <<= 1;
    return P;
}
inline bool finite_positive(double v) { return v > 0.0 && v - v == 0.0; }

struct DepthCamera {
    double fx, fy, cx, cy, depth_scale, scale_x, scale_y, view_w, view_h;
};

// One thread per keypoint.  The bounds are judged on the doubles: a coordinate no int holds never reaches a conversion.
__global__ __launch_bounds__(256) void keypoint_depth_kernel(const unsigned short *__restrict__ depth, long long total, int h, int w,
                                                              const float *__restrict__ kp_pixel, int K, double scale_x,
                                                              double scale_y, int *__restrict__ kp_depth) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const float2 q = reinterpret_cast<const float2 *>(kp_pixel)[t];
    const double u = (double)q.x * scale_x, v = (double)q.y * scale_y;
    const double c = __builtin_floor(u + 0.5), r = __builtin_floor(v + 0.5);
    int out = -1;
    if (c >= 0.0 && c < (double)w && r >= 0.0 && r < (double)h)      // a NaN fails every comparison
        out = depth[((t / K) * h + (long long)r) * w + (long long)c];
    kp_depth[t] = out;
}

// One workgroup per pair; LDS as in pose_nn_kernel plus the per-(chunk, wave) counts of the rows that have a ground truth.
__global__ __launch_bounds__(1024) void pose_depth_nn_kernel(const float *__restrict__ kp_bank, const int *__restrict__ kp_depth_bank,
                                                              int n_bank, int K, int n1, int n2, const int *__restrict__ pair_first,
                                                              const int *__restrict__ pair_second, const double *__restrict__ T,
                                                              DepthCamera cam, double threshold, int main_bytes,
                                                              long long *__restrict__ gt_matches, int *__restrict__ gt_count,
                                                              int *__restrict__ gt_of_row, int *__restrict__ valid_count,
                                                              double *__restrict__ dist_sum, double *__restrict__ dist_median) {
    extern __shared__ double eval_lds[];
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
    const long long p = blockIdx.x;
    gt_matches += p * n1 * 2;
    gt_of_row += p * n1;
    const int a = pair_first[p], b = pair_second[p];
    if ((unsigned)a >= (unsigned)n_bank || (unsigned)b >= (unsigned)n_bank) {      // an absent pair (uniform over the workgroup)
        for (int i = tid; i < n1; i += nt) {
            gt_matches[2 * i] = 0;
            gt_matches[2 * i + 1] = 0;
            gt_of_row[i] = -1;
        }
        if (tid == 0) {
            gt_count[p] = 0;
            valid_count[p] = 0;
            dist_sum[p] = 0.0;
            dist_median[p] = 0.0;
        }
        return;
    }
    float2 *pts = reinterpret_cast<float2 *>(eval_lds);
    double *dist = eval_lds;
    int *wcount = reinterpret_cast<int *>(reinterpret_cast<char *>(eval_lds) + main_bytes);    // [EVAL_ROWS][EVAL_MAX_WAVES]
    int *wvalid = wcount + EVAL_ROWS * EVAL_MAX_WAVES;                                          // [EVAL_ROWS][EVAL_MAX_WAVES]
    double *wsum = reinterpret_cast<double *>(wvalid + EVAL_ROWS * EVAL_MAX_WAVES);             // [EVAL_MAX_WAVES]

    const float2 *f1 = reinterpret_cast<const float2 *>(kp_bank) + (long long)a * K;
    const float2 *f2 = reinterpret_cast<const float2 *>(kp_bank) + (long long)b * K;
    const int *d1 = kp_depth_bank + (long long)a * K;
    for (int j = tid; j < n2; j += nt) pts[j] = f2[j];

    double m[12];
    for (int e = 0; e < 12; e++) m[e] = T[p * 12 + e];
    const double inf = __builtin_inf();
    double wx[EVAL_ROWS], wy[EVAL_ROWS], best_s[EVAL_ROWS], best_d[EVAL_ROWS];
    int best_j[EVAL_ROWS], valid[EVAL_ROWS];
#pragma unroll
    for (int c = 0; c < EVAL_ROWS; c++) {
        const int i = c * nt + tid;
        double x = 0.0, y = 0.0;
        valid[c] = 0;
        if (i < n1) {
            const float2 q = f1[i];
            const int d = d1[i];
            const double u = (double)q.x * cam.scale_x, v = (double)q.y * cam.scale_y, z = (double)d / cam.depth_scale;
            const double X = ((u - cam.cx) * z) / cam.fx, Y = ((v - cam.cy) * z) / cam.fy;
            const double X2 = ((m[0] * X + m[1] * Y) + m[2] * z) + m[3];
            const double Y2 = ((m[4] * X + m[5] * Y) + m[6] * z) + m[7];
            const double Z2 = ((m[8] * X + m[9] * Y) + m[10] * z) + m[11];
            const double u2 = (cam.fx * X2) / Z2 + cam.cx, v2 = (cam.fy * Y2) / Z2 + cam.cy;
            valid[c] = d > 0 && Z2 > 0.0 && -0.5 <= u2 && u2 < cam.view_w - 0.5 && -0.5 <= v2 && v2 < cam.view_h - 0.5;
            if (valid[c]) {                              // a row without ground truth searches from (0, 0); its result is dropped
                x = u2 / cam.scale_x;
                y = v2 / cam.scale_y;
            }
        }
        wx[c] = x;
        wy[c] = y;
        best_s[c] = inf;
        best_d[c] = inf;
        best_j[c] = 0;
    }
    __syncthreads();

    // the search of pose_nn_kernel: nearest by sqrt(dx*dx + dy*dy), the lowest index on equal distance; the root is taken only
    // for a candidate that lowers the squared distance, and the index moves only when the ROOT is lower
    for (int j = 0; j < n2; j++) {
        const float2 q = pts[j];                         // one address for the whole wave: an LDS broadcast
        const double qx = (double)q.x, qy = (double)q.y;
#pragma unroll
        for (int c = 0; c < EVAL_ROWS; c++) {
            const double dx = wx[c] - qx, dy = wy[c] - qy;
            const double s = dx * dx + dy * dy;
            if (s < best_s[c]) {
                const double d = __builtin_sqrt(s);
                if (d < best_d[c]) {
                    best_d[c] = d;
                    best_j[c] = j;
                }
                best_s[c] = s;
            }
        }
    }
    __syncthreads();                                     // the points are dead: their bytes become the distances

    const int P = eval_pow2(n1);
    double part = 0.0;
    int flag[EVAL_ROWS];
#pragma unroll
    for (int c = 0; c < EVAL_ROWS; c++) {
        const int i = c * nt + tid;
        flag[c] = valid[c] && best_d[c] < threshold;
        if (i < n1) {
            dist[i] = valid[c] ? best_d[c] : inf;        // a row without ground truth sorts behind every distance
            gt_of_row[i] = valid[c] ? (flag[c] ? best_j[c] : -1) : -2;
            part = part + (valid[c] ? best_d[c] : 0.0);  // the thread's rows in ascending index
        } else if (i < P) {
            dist[i] = inf;                               // padding (EVAL_ROWS * nt >= P)
        }
        const unsigned long long mk = __ballot(flag[c]), mv = __ballot(valid[c]);
        if (lane == 0) {
            wcount[c * EVAL_MAX_WAVES + wave] = __popcll(mk);
            wvalid[c * EVAL_MAX_WAVES + wave] = __popcll(mv);
        }
        flag[c] |= __popcll(mk & ((1ull << lane) - 1ull)) << 1;     // bit 0 the flag, above it the kept rows of lower lanes
    }
    part = part + __shfl_xor(part, 32);
    part = part + __shfl_xor(part, 16);
    part = part + __shfl_xor(part, 8);
    part = part + __shfl_xor(part, 4);
    part = part + __shfl_xor(part, 2);
    part = part + __shfl_xor(part, 1);
    if (lane == 0) wsum[wave] = part;
    __syncthreads();

    // kept rows in ascending row index, as in pose_nn_kernel; every thread also totals the rows that have a ground truth
    int total = 0, n_valid = 0;
#pragma unroll
    for (int c = 0; c < EVAL_ROWS; c++) {
        int before = total;
        for (int w = 0; w < n_waves; w++) {
            const int n = wcount[c * EVAL_MAX_WAVES + w];
            if (w < wave) before += n;
            total += n;
            n_valid += wvalid[c * EVAL_MAX_WAVES + w];
        }
        if (flag[c] & 1) {
            const int pos = before + (flag[c] >> 1);
            gt_matches[2 * pos] = c * nt + tid;
            gt_matches[2 * pos + 1] = best_j[c];
        }
    }
    for (int r = total + tid; r < n1; r += nt) {         // zeros past the count
        gt_matches[2 * r] = 0;
        gt_matches[2 * r + 1] = 0;
    }
    if (tid == 0) {
        double sum = wsum[0];
        for (int w = 1; w < n_waves; w++) sum = sum + wsum[w];
        gt_count[p] = total;
        valid_count[p] = n_valid;
        dist_sum[p] = sum;
    }

    // ascending bitonic sort of the P distances; all are >= +0 or +inf, no NaN
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < (P >> 1); t += nt) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;
                const double u = dist[i], v = dist[l];
                if ((u > v) == ((i & k) == 0)) {
                    dist[i] = v;
                    dist[l] = u;
                }
            }
        }
    __syncthreads();
    if (tid == 0)                                        // the median of the n_valid leading entries; both indices are below n_valid
        dist_median[p] = n_valid > 0 ? (dist[(n_valid - 1) >> 1] + dist[n_valid >> 1]) / 2.0 : 0.0;
}

// match_score_kernel (evaluate.hip) with the rows on -2 counted apart.  One 256-thread workgroup per pair; value_sum in its order.
__global__ __launch_bounds__(256) void match_score_known_kernel(const long long *__restrict__ matches, const float *__restrict__ value,
                                                                 const int *__restrict__ count, const int *__restrict__ gt_of_row,
                                                                 const int *__restrict__ gt_count, int n1, int *__restrict__ tp_out,
                                                                 int *__restrict__ fp_out, int *__restrict__ fn_out,
                                                                 int *__restrict__ unknown_out, double *__restrict__ value_sum) {
    __shared__ int s_tp[4], s_un[4];
    __shared__ double s_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p = blockIdx.x;
    matches += p * n1 * 2;
    value += p * n1;
    gt_of_row += p * n1;
    int c = count[p];
    c = c < 0 ? 0 : (c > n1 ? n1 : c);
    int tp = 0, un = 0;
    double sum = 0.0;
    for (int r = tid; r < c; r += 256) {
        const long long i1 = matches[2 * r], i2 = matches[2 * r + 1];
        if (i1 >= 0 && i1 < n1) {
            const int g = gt_of_row[i1];
            if (g == -2) un++;                           // no ground truth for this query: the match cannot be called wrong
            else if ((long long)g == i2) tp++;
        }
        sum = sum + (double)value[r];
    }
    for (int o = 32; o >= 1; o >>= 1) {
        tp += __shfl_xor(tp, o);
        un += __shfl_xor(un, o);
        sum = sum + __shfl_xor(sum, o);
    }
    if (lane == 0) {
        s_tp[wave] = tp;
        s_un[wave] = un;
        s_sum[wave] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        const int t = (s_tp[0] + s_tp[1]) + (s_tp[2] + s_tp[3]), u = (s_un[0] + s_un[1]) + (s_un[2] + s_un[3]);
        tp_out[p] = t;
        fp_out[p] = c - t - u;
        fn_out[p] = gt_count[p] - t;
        unknown_out[p] = u;
        value_sum[p] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    }
}

}  // namespace

extern "C" int sslam_keypoint_depth(const uint16_t *depth, int n, int h, int w, const float *kp_pixel, int K, double scale_x,
                                    double scale_y, int32_t *kp_depth, void *stream) {
    if (!depth || !kp_pixel || !kp_depth) return SSLAM_E_INVALID;
    if (n <= 0 || h <= 0 || w <= 0 || K <= 0) return SSLAM_E_INVALID;
    if (!finite_positive(scale_x) || !finite_positive(scale_y)) return SSLAM_E_INVALID;
    if ((uintptr_t)depth & 1 || (uintptr_t)kp_pixel & 7 || (uintptr_t)kp_depth & 3) return SSLAM_E_INVALID;
    const long long total = (long long)n * K;
    if (total > 0x7fffffffLL) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(keypoint_depth_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, total, h,
                       w, kp_pixel, K, scale_x, scale_y, kp_depth);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

extern "C" int sslam_pose_depth_nn_pairs(const float *kp_bank, const int32_t *kp_depth_bank, int n_bank, int K, int n1, int n2,
                                         const int32_t *pair_first, const int32_t *pair_second, int n_pairs, const double *T, double fx,
                                         double fy, double cx, double cy, double depth_scale, double scale_x, double scale_y,
                                         double view_w, double view_h, double threshold, int64_t *gt_matches, int32_t *gt_count,
                                         int32_t *gt_of_row, int32_t *valid_count, double *dist_sum, double *dist_median, void *stream) {
    if (!kp_bank || !kp_depth_bank || !pair_first || !pair_second || !T || !gt_matches || !gt_count || !gt_of_row || !valid_count ||
        !dist_sum || !dist_median)
        return SSLAM_E_INVALID;
    if (n_bank <= 0 || K <= 0 || n1 <= 0 || n2 <= 0 || n_pairs <= 0 || n1 > K || n2 > K) return SSLAM_E_INVALID;
    if (!(threshold >= 0.0) || threshold - threshold != 0.0) return SSLAM_E_INVALID;       // NaN, negative, infinite
    if (!finite_positive(fx) || !finite_positive(fy) || !finite_positive(depth_scale) || !finite_positive(scale_x) ||
        !finite_positive(scale_y))
        return SSLAM_E_INVALID;
    if (cx - cx != 0.0 || cy - cy != 0.0 || !finite_positive(view_w) || !finite_positive(view_h)) return SSLAM_E_INVALID;
    if ((uintptr_t)kp_bank & 7 || (uintptr_t)kp_depth_bank & 3 || (uintptr_t)pair_first & 3 || (uintptr_t)pair_second & 3 ||
        (uintptr_t)T & 7)
        return SSLAM_E_INVALID;
    if (sslam_misaligned(8, gt_matches, dist_sum, dist_median) || sslam_misaligned(4, gt_count, gt_of_row, valid_count)) return SSLAM_E_INVALID;
    if (K > EVAL_MAX_K) return SSLAM_E_UNSUPPORTED;
    const int P = eval_pow2(n1);
    const int main_bytes = (P > n2 ? P : n2) * 8;
    const size_t lds = (size_t)main_bytes + 2 * EVAL_ROWS * EVAL_MAX_WAVES * sizeof(int) + EVAL_MAX_WAVES * sizeof(double);
    const DepthCamera cam = {fx, fy, cx, cy, depth_scale, scale_x, scale_y, view_w, view_h};
    hipLaunchKernelGGL(pose_depth_nn_kernel, dim3((unsigned)n_pairs), dim3(eval_threads(n1)), lds, (hipStream_t)stream, kp_bank,
                       kp_depth_bank, n_bank, K, n1, n2, pair_first, pair_second, T, cam, threshold, main_bytes,
                       (long long *)gt_matches, gt_count, gt_of_row, valid_count, dist_sum, dist_median);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

extern "C" int sslam_match_score_known_pairs(const int64_t *matches, const float *value, const int32_t *count, const int32_t *gt_of_row,
                                             const int32_t *gt_count, int n1, int n_pairs, int32_t *tp, int32_t *fp, int32_t *fn,
                                             int32_t *unknown, double *value_sum, void *stream) {
    if (!matches || !value || !count || !gt_of_row || !gt_count || !tp || !fp || !fn || !unknown || !value_sum) return SSLAM_E_INVALID;
    if (n1 <= 0 || n_pairs <= 0) return SSLAM_E_INVALID;
    if (sslam_misaligned(8, matches, value_sum) || sslam_misaligned(4, value, count, gt_of_row, gt_count, tp, fp, fn, unknown))
        return SSLAM_E_INVALID;
    if (n1 > EVAL_MAX_K) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(match_score_known_kernel, dim3((unsigned)n_pairs), dim3(256), 0, (hipStream_t)stream, (const long long *)matches,
                       value, count, gt_of_row, gt_count, n1, tp, fp, fn, unknown, value_sum);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}
