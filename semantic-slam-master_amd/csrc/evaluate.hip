// evaluate.hip - the reference's two headline quality scores on the device, per frame pair of a keypoint bank, against either of two
// ground truths:
//   sslam_pose_nn_pairs    RepeatabilityTester.compute_repeatability (test/test_repeatability.py:79-128) and
//                          DescriptorQualityTester.compute_ground_truth_matches (test/test_descriptor_quality.py:144-185):
//                          warp frame 1's keypoints by a homography, find the nearest keypoint of frame 2, keep the rows nearer
//                          than a threshold, sum and take the median of the distances;
//   sslam_match_score_pairs  evaluate_matches (test/test_descriptor_quality.py:187-231): tp / fp / fn of a match list against
//                          those ground-truth rows, and the float64 sum of the list's values;
//   sslam_keypoint_depth           the raw uint16 depth under every keypoint of a frame (the depth sibling of A9), -1 outside;
//   sslam_pose_depth_nn_pairs      sslam_pose_nn_pairs with the homography replaced by back-projection with the keypoint's depth,
//                                  the rigid transform [R | t] and projection into the other frame; a row without a measurement,
//                                  behind the other camera or outside its view HAS NO GROUND TRUTH (gt_of_row = -2);
//   sslam_match_score_known_pairs  sslam_match_score_pairs that counts the listed rows on -2 apart instead of as false positives.
// The two searches are one kernel over a warp policy, the two list scores one kernel over a flag.
// All arithmetic is float64 in the order include/sslam_hip.h states (the file is compiled with -ffp-contract=off: a product and
// the sum it feeds are rounded separately, as numpy rounds them).  Every sum has one order fixed by the shapes alone, so a pair's
// outputs are the same bits in any launch.  No atomics, no scratch, no allocation, no host read: every launch can be captured.
#include "pose_common.h"

namespace {

constexpr int EVAL_MAX_K = SSLAM_EVAL_MAX_K;
constexpr int EVAL_ROWS = 4;            // rows of frame 1 a thread carries in registers: EVAL_MAX_K / 1024
constexpr int EVAL_MAX_WAVES = 16;      // of a 1024-thread workgroup
static_assert(EVAL_ROWS * 1024 >= EVAL_MAX_K, "a workgroup's threads must cover every row");

// threads of the workgroup that serves n1 rows: every thread owns at most EVAL_ROWS rows i = c * threads + tid
inline int eval_threads(int n1) { return n1 <= 256 * EVAL_ROWS ? 256 : 1024; }
__host__ __device__ inline int eval_pow2(int n) {
    int P = 1;
    while (P < n) P <<= 1;
    return P;
}

// A warp takes a row of frame 1 into frame 2's keypoint units.  load() reads a pair's N doubles once; row() yields the warped
// (x, y) of the keypoint q at bank row r and says whether the row has a ground truth.  PARTIAL: some rows may have none.
struct HomographyWarp {
    static constexpr bool PARTIAL = false;
    static constexpr int N = 9;
    const double *H;                                     // [n_pairs][9], or nullptr: the identity
    __device__ __forceinline__ void load(long long p, double *h) const {
        for (int e = 0; e < 9; e++) h[e] = e % 4 == 0 ? 1.0 : 0.0;
        if (H)                                           // one branch around the nine loads: they go out together
            for (int e = 0; e < 9; e++) h[e] = H[p * 9 + e];
    }
    __device__ __forceinline__ bool row(const double *h, long long, const float2 q, double &x, double &y) const {
        x = (double)q.x;
        y = (double)q.y;
        if (H) {
            const double X = (h[0] * x + h[1] * y) + h[2];
            const double Y = (h[3] * x + h[4] * y) + h[5];
            const double W = (h[6] * x + h[7] * y) + h[8];
            x = X / W;                                   // W == 0: an infinite coordinate, an infinite distance to every point
            y = Y / W;
        }
        return true;
    }
};

struct DepthWarp {
    static constexpr bool PARTIAL = true;
    static constexpr int N = 12;
    const int *kp_depth_bank;
    const double *T;                                     // [n_pairs][12]
    PoseCamera cam;
    double view_w, view_h;
    __device__ __forceinline__ void load(long long p, double *m) const {
        for (int e = 0; e < 12; e++) m[e] = T[p * 12 + e];
    }
    __device__ __forceinline__ bool row(const double *m, long long r, const float2 q, double &x, double &y) const {
        const int d = kp_depth_bank[r];
        double X, Y, z, u2, v2, Z2;
        pose_back_project(q, d, cam, X, Y, z);
        pose_project(m, X, Y, z, cam, u2, v2, Z2);
        const bool known = d > 0 && Z2 > 0.0 && -0.5 <= u2 && u2 < view_w - 0.5 && -0.5 <= v2 && v2 < view_h - 0.5;
        if (known) {                                     // a row without ground truth searches from (0, 0); its result is dropped
            x = u2 / cam.scale_x;
            y = v2 / cam.scale_y;
        }
        return known;
    }
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

// One workgroup per pair.  LDS: frame 2's points (n2 float2) while the rows search them, then - the points being dead - the
// P = pow2 >= n1 distances the median sorts, in the same bytes; behind them the per-(chunk, wave) counts of the kept rows, under a
// PARTIAL warp those of the rows that have a ground truth, and the per-wave sums.  valid_count is written under a PARTIAL warp only.
template <class Warp>
__global__ __launch_bounds__(1024) void pose_nn_kernel(const float *__restrict__ kp_bank, int n_bank, int K, int n1, int n2,
                                                        const int *__restrict__ pair_first, const int *__restrict__ pair_second,
                                                        const Warp warp, double threshold, int main_bytes,
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
            if constexpr (Warp::PARTIAL) valid_count[p] = 0;
            dist_sum[p] = 0.0;
            dist_median[p] = 0.0;
        }
        return;
    }
    float2 *pts = reinterpret_cast<float2 *>(eval_lds);
    double *dist = eval_lds;
    int *wcount = reinterpret_cast<int *>(reinterpret_cast<char *>(eval_lds) + main_bytes);    // [EVAL_ROWS][EVAL_MAX_WAVES]
    int *wvalid = wcount + EVAL_ROWS * EVAL_MAX_WAVES;                                          // the same, PARTIAL only
    double *wsum = reinterpret_cast<double *>(wcount + (Warp::PARTIAL ? 2 : 1) * EVAL_ROWS * EVAL_MAX_WAVES);      // [EVAL_MAX_WAVES]

    const float2 *f1 = reinterpret_cast<const float2 *>(kp_bank) + (long long)a * K;
    const float2 *f2 = reinterpret_cast<const float2 *>(kp_bank) + (long long)b * K;
    for (int j = tid; j < n2; j += nt) pts[j] = f2[j];

    double m[Warp::N];
    warp.load(p, m);
    const double inf = __builtin_inf();
    double wx[EVAL_ROWS], wy[EVAL_ROWS], best_s[EVAL_ROWS], best_d[EVAL_ROWS];
    int best_j[EVAL_ROWS], known[EVAL_ROWS];             // known: the row is one of the n1 and has a ground truth
#pragma unroll
    for (int c = 0; c < EVAL_ROWS; c++) {
        const int i = c * nt + tid;
        double x = 0.0, y = 0.0;
        known[c] = 0;
        if (i < n1) known[c] = warp.row(m, (long long)a * K + i, f1[i], x, y);
        wx[c] = x;
        wy[c] = y;
        best_s[c] = inf;
        best_d[c] = inf;
        best_j[c] = 0;                                   // numpy's argmin of a row of infinities
    }
    __syncthreads();

    // The nearest point by sqrt(dx*dx + dy*dy), the lowest index on equal distance.  sqrt is monotone, so a candidate can only
    // lower the distance when it lowers the squared one: the root is taken for those alone, and the index moves only when the
    // ROOT is lower - two squares that round to one root keep the earlier index, as argmin over the roots does.
    // Where the loop lies in its 64-byte instruction lines shows in the time (profiles/pose_stage_merge.txt: 1 % between two
    // places 16 bytes apart), so its place is pinned whatever the code before it comes to: a line boundary and four no-ops.
    asm volatile(".p2align 6\n s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0");
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
        flag[c] = known[c] && best_d[c] < threshold;
        if (i < n1) {
            if constexpr (Warp::PARTIAL) {
                dist[i] = known[c] ? best_d[c] : inf;    // a row without ground truth sorts behind every distance
                gt_of_row[i] = known[c] ? (flag[c] ? best_j[c] : -1) : -2;
                part = part + (known[c] ? best_d[c] : 0.0);
            } else {
                dist[i] = best_d[c];
                gt_of_row[i] = flag[c] ? best_j[c] : -1;
                part = part + best_d[c];                 // the thread's rows in ascending index
            }
        } else if (i < P) {
            dist[i] = inf;                               // padding sorts behind every distance (EVAL_ROWS * nt >= P)
        }
        const unsigned long long mk = __ballot(flag[c]);
        if (lane == 0) wcount[c * EVAL_MAX_WAVES + wave] = __popcll(mk);
        if constexpr (Warp::PARTIAL) {
            const unsigned long long mv = __ballot(known[c]);
            if (lane == 0) wvalid[c * EVAL_MAX_WAVES + wave] = __popcll(mv);
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

    // kept rows in ascending row index: row i = c * nt + tid comes after every row of the chunks below c and after the rows of
    // the lower waves and lanes of its own chunk; under a PARTIAL warp every thread also totals the rows that have a ground truth
    int total = 0, n_known = 0;
#pragma unroll
    for (int c = 0; c < EVAL_ROWS; c++) {
        int before = total;
        for (int w = 0; w < n_waves; w++) {
            const int n = wcount[c * EVAL_MAX_WAVES + w];
            if (w < wave) before += n;
            total += n;
            if constexpr (Warp::PARTIAL) n_known += wvalid[c * EVAL_MAX_WAVES + w];
        }
        if (flag[c] & 1) {
            const int pos = before + (flag[c] >> 1);
            gt_matches[2 * pos] = c * nt + tid;
            gt_matches[2 * pos + 1] = best_j[c];
        }
    }
    for (int r = total + tid; r < n1; r += nt) {         // zeros past the count, as the finalize kernels leave them
        gt_matches[2 * r] = 0;
        gt_matches[2 * r + 1] = 0;
    }
    if (tid == 0) {
        double sum = wsum[0];
        for (int w = 1; w < n_waves; w++) sum = sum + wsum[w];
        gt_count[p] = total;
        if constexpr (Warp::PARTIAL) valid_count[p] = n_known;
        dist_sum[p] = sum;
    }

    // ascending bitonic sort of the P distances (rank.hip sorts a pair's keys the same way); all are >= +0 or +inf, no NaN
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
    if (tid == 0) {                                      // np.median of the n_known leading entries: the mean of the middle two
        if constexpr (Warp::PARTIAL)
            dist_median[p] = n_known > 0 ? (dist[(n_known - 1) >> 1] + dist[n_known >> 1]) / 2.0 : 0.0;
        else
            dist_median[p] = (dist[(n1 - 1) >> 1] + dist[n1 >> 1]) / 2.0;
    }
}

// One 256-thread workgroup per pair.  value_sum: the thread's rows in ascending index, the 64 lanes by xor 32, 16, .. 1, the
// four waves in order.  KNOWN: gt_of_row may hold -2, and the listed rows on it are counted apart into unknown_out.
template <bool KNOWN>
__global__ __launch_bounds__(256) void match_score_kernel(const long long *__restrict__ matches, const float *__restrict__ value,
                                                           const int *__restrict__ count, const int *__restrict__ gt_of_row,
                                                           const int *__restrict__ gt_count, int n1, int *__restrict__ tp_out,
                                                           int *__restrict__ fp_out, int *__restrict__ fn_out,
                                                           int *__restrict__ unknown_out, double *__restrict__ value_sum) {
    __shared__ int s_tp[4], s_un[KNOWN ? 4 : 1];
    __shared__ double s_sum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p = blockIdx.x;
    matches += p * n1 * 2;
    value += p * n1;
    gt_of_row += p * n1;
    int c = count[p];
    c = c < 0 ? 0 : (c > n1 ? n1 : c);                   // the arrays need not come from a finalize kernel: never read past them
    int tp = 0, un = 0;
    double sum = 0.0;
    for (int r = tid; r < c; r += 256) {
        const long long i1 = matches[2 * r], i2 = matches[2 * r + 1];
        if (i1 >= 0 && i1 < n1) {
            const int g = gt_of_row[i1];                 // -1, -2 or an index: a negative i2 never hits
            if (KNOWN && g == -2) un++;                  // no ground truth for this query: the match cannot be called wrong
            else if ((long long)g == i2) tp++;
        }
        sum = sum + (double)value[r];
    }
    for (int o = 32; o >= 1; o >>= 1) {
        tp += __shfl_xor(tp, o);
        if constexpr (KNOWN) un += __shfl_xor(un, o);
        sum = sum + __shfl_xor(sum, o);
    }
    if (lane == 0) {
        s_tp[wave] = tp;
        if constexpr (KNOWN) s_un[wave] = un;
        s_sum[wave] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        const int t = (s_tp[0] + s_tp[1]) + (s_tp[2] + s_tp[3]);
        int u = 0;
        if constexpr (KNOWN) u = (s_un[0] + s_un[1]) + (s_un[2] + s_un[3]);
        tp_out[p] = t;
        fp_out[p] = c - t - u;
        fn_out[p] = gt_count[p] - t;
        if constexpr (KNOWN) unknown_out[p] = u;
        value_sum[p] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    }
}

// what the two searches check and launch alike; valid_count: the PARTIAL warp's extra output, else nullptr
template <class Warp>
int pose_nn_launch(const float *kp_bank, int n_bank, int K, int n1, int n2, const int32_t *pair_first, const int32_t *pair_second,
                   int n_pairs, const Warp &warp, double threshold, int64_t *gt_matches, int32_t *gt_count, int32_t *gt_of_row,
                   int32_t *valid_count, double *dist_sum, double *dist_median, void *stream) {
    if (!gt_matches || !gt_count || !gt_of_row || !dist_sum || !dist_median || (Warp::PARTIAL && !valid_count)) return SSLAM_E_INVALID;
    if (n_bank <= 0 || K <= 0 || n1 <= 0 || n2 <= 0 || n_pairs <= 0 || n1 > K || n2 > K) return SSLAM_E_INVALID;
    if (sslam_misaligned(8, gt_matches, dist_sum, dist_median) || sslam_misaligned(4, gt_count, gt_of_row, valid_count)) return SSLAM_E_INVALID;
    if (K > EVAL_MAX_K) return SSLAM_E_UNSUPPORTED;
    const int P = eval_pow2(n1);
    const int main_bytes = (P > n2 ? P : n2) * 8;
    const size_t lds = (size_t)main_bytes + (Warp::PARTIAL ? 2 : 1) * EVAL_ROWS * EVAL_MAX_WAVES * sizeof(int) + EVAL_MAX_WAVES * sizeof(double);
    hipLaunchKernelGGL(pose_nn_kernel<Warp>, dim3((unsigned)n_pairs), dim3(eval_threads(n1)), lds, (hipStream_t)stream, kp_bank, n_bank,
                       K, n1, n2, pair_first, pair_second, warp, threshold, main_bytes, (long long *)gt_matches, gt_count, gt_of_row,
                       valid_count, dist_sum, dist_median);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

// unknown: the KNOWN score's extra output, else nullptr
template <bool KNOWN>
int match_score_launch(const int64_t *matches, const float *value, const int32_t *count, const int32_t *gt_of_row, const int32_t *gt_count,
                       int n1, int n_pairs, int32_t *tp, int32_t *fp, int32_t *fn, int32_t *unknown, double *value_sum, void *stream) {
    if (!matches || !value || !count || !gt_of_row || !gt_count || !tp || !fp || !fn || (KNOWN && !unknown) || !value_sum) return SSLAM_E_INVALID;
    if (n1 <= 0 || n_pairs <= 0) return SSLAM_E_INVALID;
    if (sslam_misaligned(8, matches, value_sum) || sslam_misaligned(4, value, count, gt_of_row, gt_count, tp, fp, fn, unknown))
        return SSLAM_E_INVALID;
    if (n1 > EVAL_MAX_K) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(match_score_kernel<KNOWN>, dim3((unsigned)n_pairs), dim3(256), 0, (hipStream_t)stream, (const long long *)matches,
                       value, count, gt_of_row, gt_count, n1, tp, fp, fn, unknown, value_sum);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

}  // namespace

extern "C" int sslam_pose_nn_pairs(const float *kp_bank, int n_bank, int K, int n1, int n2, const int32_t *pair_first,
                                   const int32_t *pair_second, int n_pairs, const double *H, double threshold, int64_t *gt_matches,
                                   int32_t *gt_count, int32_t *gt_of_row, double *dist_sum, double *dist_median, void *stream) {
    if (!kp_bank || !pair_first || !pair_second || !finite_nonnegative(threshold)) return SSLAM_E_INVALID;
    if ((uintptr_t)kp_bank & 7 || (uintptr_t)pair_first & 3 || (uintptr_t)pair_second & 3 || (uintptr_t)H & 7) return SSLAM_E_INVALID;
    return pose_nn_launch(kp_bank, n_bank, K, n1, n2, pair_first, pair_second, n_pairs, HomographyWarp{H}, threshold, gt_matches, gt_count,
                          gt_of_row, nullptr, dist_sum, dist_median, stream);
}

extern "C" int sslam_match_score_pairs(const int64_t *matches, const float *value, const int32_t *count, const int32_t *gt_of_row,
                                       const int32_t *gt_count, int n1, int n_pairs, int32_t *tp, int32_t *fp, int32_t *fn,
                                       double *value_sum, void *stream) {
    return match_score_launch<false>(matches, value, count, gt_of_row, gt_count, n1, n_pairs, tp, fp, fn, nullptr, value_sum, stream);
}

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
    if (!pose_args_ok(kp_bank, kp_depth_bank, pair_first, pair_second, fx, fy, cx, cy, depth_scale, scale_x, scale_y, view_w, view_h,
                      threshold))
        return SSLAM_E_INVALID;
    if (!T || (uintptr_t)T & 7) return SSLAM_E_INVALID;
    const DepthWarp warp = {kp_depth_bank, T, {fx, fy, cx, cy, depth_scale, scale_x, scale_y}, view_w, view_h};
    return pose_nn_launch(kp_bank, n_bank, K, n1, n2, pair_first, pair_second, n_pairs, warp, threshold, gt_matches, gt_count, gt_of_row,
                          valid_count, dist_sum, dist_median, stream);
}

extern "C" int sslam_match_score_known_pairs(const int64_t *matches, const float *value, const int32_t *count, const int32_t *gt_of_row,
                                             const int32_t *gt_count, int n1, int n_pairs, int32_t *tp, int32_t *fp, int32_t *fn,
                                             int32_t *unknown, double *value_sum, void *stream) {
    return match_score_launch<true>(matches, value, count, gt_of_row, gt_count, n1, n_pairs, tp, fp, fn, unknown, value_sum, stream);
}
