// place.hip - libsslam_place.so: loop closures while the sequence runs (include/sslam_place.h states the arithmetic operation by
// operation; tests/place_ref.py restates it in numpy).
//   sslp_place_step      three kernels on one stream, the frame counter read from device memory by each:
//                        (a) raw_kernel        one workgroup of d threads, thread c one column: this frame's score-weighted column
//                                              sum (ssll_frame_signatures' fmaf chain) into raw[t], and the running sum;
//                        (b) similarity_kernel one workgroup of d threads per SSLP_FRAMES_PER_GROUP bank frames, the grid fixed by
//                                              capacity; a group wholly past t - min_gap leaves at once (group 0 stays: it writes
//                                              sig).  Each forms the mean and sig_t anew, then its frames' signatures into LDS, and
//                                              thread f of the first 32 runs frame f's one fmaf chain: S_tj into the workspace;
//                        (c) pick_kernel       one 256-thread workgroup: ssll_loop_candidates' picks for the row i = t, the outputs,
//                                              the counter.
//   sslp_edge_log_step   one workgroup, one wave per slot: lane l judges word l of the slot's 33, a wave vote decides, lanes write.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sslam_place.h"

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;
constexpr int FPG = SSLP_FRAMES_PER_GROUP;

long long g_launches = 0;   // diagnostic launch counter (sslp_launch_count): relaxed atomic adds, the library's only mutable state

inline bool width_ok(int d) { return d == 128 || d == 256; }
inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

__device__ __forceinline__ bool counter_ok(int t, long long capacity) { return t >= 0 && t < capacity; }
__device__ __forceinline__ bool fin(double v) { return v - v == 0.0; }

// ---------------------------------------------------------------------------------------------------------------- the raw sum
__global__ __launch_bounds__(NT) void raw_kernel(const int *__restrict__ tp, const float *__restrict__ desc, const float *__restrict__ scores,
                                                 int capacity, int k, int d, float *__restrict__ raw, float *__restrict__ sum) {
    const int t = *tp, c = threadIdx.x;
    if (!counter_ok(t, capacity)) return;                // uniform
    const float *dp = desc + c;
    float acc = 0.0f;
    for (int kk = 0; kk < k; kk++) acc = fmaf(scores[kk], dp[kk * d], acc);
    raw[t * d + c] = acc;
    sum[c] = (t == 0 ? 0.0f : sum[c]) + acc;
}

// the sum of p over the d threads of the workgroup, in ssll_frame_signatures' order; two barriers
__device__ __forceinline__ float column_sum(float p, int d, float *wsum, int c) {
    for (int o = 32; o >= 1; o >>= 1) p = p + __shfl_xor(p, o);
    if ((c & 63) == 0) wsum[c >> 6] = p;
    __syncthreads();
    float ss = wsum[0] + wsum[1];
    if (d == 256) ss = (ss + wsum[2]) + wsum[3];
    __syncthreads();                                     // wsum is written again
    return ss;
}

// ------------------------------------------------------------------------------------------------------------ the similarities
__global__ __launch_bounds__(NT) void similarity_kernel(const int *__restrict__ tp, const float *__restrict__ raw,
                                                        const float *__restrict__ sum, int capacity, int d, int min_gap, float min_sim,
                                                        float *__restrict__ S, float *__restrict__ sig) {
    __shared__ float wsum[WAVES];
    __shared__ float st[256];                            // sig_t
    __shared__ float sj[FPG * 257];                      // the group's signatures, a row every d + 1 words: thread f walks row f
    const int t = *tp, c = threadIdx.x;
    if (!counter_ok(t, capacity)) return;                // uniform
    const int m = t - min_gap + 1;                       // the frames 0 .. m - 1 are old enough (none if m <= 0)
    const int f0 = blockIdx.x * FPG;
    if (blockIdx.x > 0 && f0 >= m) return;               // uniform
    const float mean = sum[c] / (float)(t + 1);
    {
        const float cv = raw[t * d + c] - mean;
        const float ss = column_sum(cv * cv, d, wsum, c);
        const float v = cv / fmaxf(sqrtf(ss), 1e-12f);
        st[c] = v;
        if (blockIdx.x == 0) sig[c] = v;
    }
    const int f1 = f0 + FPG < m ? f0 + FPG : m, row = d + 1;
    for (int f = f0; f < f1; f++) {
        const float cv = raw[f * d + c] - mean;
        const float ss = column_sum(cv * cv, d, wsum, c);
        sj[(f - f0) * row + c] = cv / fmaxf(sqrtf(ss), 1e-12f);
    }
    __syncthreads();
    if (c < f1 - f0) {
        const float *r = sj + c * row;
        float acc = 0.0f;
        for (int q = 0; q < d; q++) acc = fmaf(st[q], r[q], acc);
        S[f0 + c] = acc >= min_sim ? acc : -__builtin_huge_valf();
    }
}

// ------------------------------------------------------------------------------------------------------------------- the picks
// is (ov, oj) ahead of (bv, bj)?  value descending, then frame ascending; a negative frame is no candidate
__device__ __forceinline__ bool ahead(float ov, int oj, float bv, int bj) { return oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj)); }

__global__ __launch_bounds__(NT) void pick_kernel(int *__restrict__ tp, const float *__restrict__ Sg, int capacity, int d, int min_gap,
                                                  int per_frame, int suppress, int *__restrict__ first, int *__restrict__ second,
                                                  float *__restrict__ sim, int *__restrict__ count, int *__restrict__ status,
                                                  float *__restrict__ sig) {
    __shared__ float S[SSLP_MAX_CAPACITY];               // S_tj, -inf where j is not (or no longer) eligible
    __shared__ float wv[WAVES];
    __shared__ int wj[WAVES];
    const int t = *tp, tid = threadIdx.x;
    if (!counter_ok(t, capacity)) {                      // uniform: the pair list reads "absent", the state is left alone
        if (tid < per_frame) first[tid] = -1, second[tid] = -1, sim[tid] = 0.0f;
        if (tid < d) sig[tid] = 0.0f;
        if (tid == 0) count[0] = 0, status[0] = 4;
        return;
    }
    const int m = t - min_gap + 1;
    const float none = -__builtin_huge_valf();
    for (int j = tid; j < m; j += NT) S[j] = Sg[j];
    __syncthreads();
    int cnt = 0;
#pragma unroll 1
    for (int s = 0; s < per_frame; s++) {
        float bv = none;
        int bj = -1;
        for (int j = tid; j < m; j += NT) {                // ascending: of equal values the lowest j stays
            const float v = S[j];
            if (v > bv) bv = v, bj = j;
        }
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oj = __shfl_xor(bj, o);
            if (ahead(ov, oj, bv, bj)) bv = ov, bj = oj;
        }
        if ((tid & 63) == 0) wv[tid >> 6] = bv, wj[tid >> 6] = bj;
        __syncthreads();
        bv = wv[0], bj = wj[0];
        for (int w = 1; w < WAVES; w++)
            if (ahead(wv[w], wj[w], bv, bj)) bv = wv[w], bj = wj[w];
        __syncthreads();                                     // wv, wj are written again
        if (bj < 0) break;                                   // uniform: nothing eligible is left
        if (tid == 0) first[s] = bj, second[s] = t, sim[s] = bv;
        cnt++;
        const int reach = suppress < m ? suppress : m;       // m <= 4096: bj + reach cannot wrap
        const int lo = bj - reach > 0 ? bj - reach : 0, hi = bj + reach < m - 1 ? bj + reach : m - 1;
        for (int j = lo + tid; j <= hi; j += NT) S[j] = none;
        __syncthreads();
    }
    if (tid == 0) {
        for (int s = cnt; s < per_frame; s++) first[s] = -1, second[s] = -1, sim[s] = 0.0f;
        count[0] = cnt;
        status[0] = 0;
        *tp = t + 1;                                         // every read of the counter in this launch came before the barriers above
    }
}

// ---------------------------------------------------------------------------------------------------------------- the edge log
__global__ __launch_bounds__(64 * SSLP_MAX_SLOTS) void edge_log_kernel(int *__restrict__ tp, int *__restrict__ log_first,
                                                                       int *__restrict__ log_second, double *__restrict__ log_T,
                                                                       double *__restrict__ log_info, const int *__restrict__ slot_first,
                                                                       const double *__restrict__ new_T, const double *__restrict__ new_info,
                                                                       const int *__restrict__ new_status, const int *__restrict__ new_inliers,
                                                                       int E, int n_odometry, int min_inliers, int loop_min_inliers,
                                                                       long long capacity, int *__restrict__ logged, int *__restrict__ status) {
    const int t = *tp, e = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (!counter_ok(t, capacity)) {                      // uniform
        if (l == 0) logged[e] = 0;
        if (threadIdx.x == 0) status[0] = 4;
        return;
    }
    const int a = slot_first[e];
    const double v = l < 12 ? new_T[e * 12 + l] : (l < 33 ? new_info[e * 21 + l - 12] : 0.0);
    const bool ok = __all(a >= 0 && a < t && new_status[e] != 3 && new_inliers[e] >= (e < n_odometry ? min_inliers : loop_min_inliers) && fin(v));
    const long long row = (long long)t * E + e;
    if (l < 12) log_T[row * 12 + l] = ok ? v : 0.0;
    else if (l < 33) log_info[row * 21 + l - 12] = ok ? v : 0.0;
    else if (l == 33) log_first[row] = ok ? a : -1;
    else if (l == 34) log_second[row] = t;
    else if (l == 35) logged[e] = ok;
    __syncthreads();                                     // every thread has read the counter
    if (threadIdx.x == 0) status[0] = 0, *tp = t + 1;
}

inline int launched(void) {
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}

inline int place_shape(int capacity) {
    if (capacity <= 0) return SSLAM_E_INVALID;
    return capacity > SSLP_MAX_CAPACITY ? SSLAM_E_UNSUPPORTED : SSLAM_OK;
}

}  // namespace

extern "C" int sslp_version(void) { return 100; }
extern "C" const char *sslp_arch(void) { return "gfx950"; }
extern "C" long long sslp_launch_count(void) { return __atomic_load_n(&g_launches, __ATOMIC_RELAXED); }

extern "C" size_t sslp_place_workspace_bytes(int capacity) {
    if (place_shape(capacity) != SSLAM_OK) return 0;
    return (size_t)capacity * sizeof(float);
}

extern "C" int sslp_place_step(int32_t *t, float *raw, float *sum, const float *desc, const float *scores, int capacity, int k, int d,
                               int min_gap, float min_sim, int per_frame, int suppress, void *workspace, int32_t *first, int32_t *second,
                               float *sim, int32_t *count, int32_t *status, float *sig, void *stream) {
    for (const void *p : {(const void *)t, (const void *)raw, (const void *)sum, (const void *)desc, (const void *)scores,
                          (const void *)workspace, (const void *)first, (const void *)second, (const void *)sim, (const void *)count,
                          (const void *)status, (const void *)sig})
        if (!p || misaligned(p, 4)) return SSLAM_E_INVALID;
    if (capacity <= 0 || k <= 0 || d <= 0 || min_gap < 1 || per_frame < 1 || suppress < 0 || !(min_sim - min_sim == 0.0f)) return SSLAM_E_INVALID;
    if (place_shape(capacity) != SSLAM_OK || k > SSLP_MAX_K || !width_ok(d) || per_frame > SSLP_MAX_PER_FRAME) return SSLAM_E_UNSUPPORTED;
    float *S = (float *)workspace;
    hipLaunchKernelGGL(raw_kernel, dim3(1), dim3((unsigned)d), 0, (hipStream_t)stream, (const int *)t, desc, scores, capacity, k, d, raw, sum);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    const int groups = (capacity + FPG - 1) / FPG;
    hipLaunchKernelGGL(similarity_kernel, dim3((unsigned)groups), dim3((unsigned)d), 0, (hipStream_t)stream, (const int *)t, (const float *)raw,
                       (const float *)sum, capacity, d, min_gap, min_sim, S, sig);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (int *)t, (const float *)S, capacity, d, min_gap, per_frame,
                       suppress, (int *)first, (int *)second, sim, (int *)count, (int *)status, sig);
    return launched();
}

extern "C" int sslp_edge_log_step(int32_t *t, int32_t *log_first, int32_t *log_second, double *log_T, double *log_info,
                                  const int32_t *slot_first, const double *new_T, const double *new_info, const int32_t *new_status,
                                  const int32_t *new_inliers, int n_slots, int n_odometry, int min_inliers, int loop_min_inliers,
                                  long long capacity, int32_t *logged, int32_t *status, void *stream) {
    for (const void *p : {(const void *)log_T, (const void *)log_info, (const void *)new_T, (const void *)new_info})
        if (!p || misaligned(p, 8)) return SSLAM_E_INVALID;
    for (const void *p : {(const void *)t, (const void *)log_first, (const void *)log_second, (const void *)slot_first, (const void *)new_status,
                          (const void *)new_inliers, (const void *)logged, (const void *)status})
        if (!p || misaligned(p, 4)) return SSLAM_E_INVALID;
    if (n_slots <= 0 || n_odometry < 0 || min_inliers < 0 || loop_min_inliers < 0 || capacity <= 0) return SSLAM_E_INVALID;
    if (n_slots > SSLP_MAX_SLOTS) return SSLAM_E_UNSUPPORTED;
    if (n_odometry > n_slots) return SSLAM_E_INVALID;
    if (capacity > 0x7fffffffffffffffLL / 168 / n_slots) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(edge_log_kernel, dim3(1), dim3(64u * (unsigned)n_slots), 0, (hipStream_t)stream, (int *)t, (int *)log_first,
                       (int *)log_second, log_T, log_info, (const int *)slot_first, new_T, new_info, (const int *)new_status,
                       (const int *)new_inliers, n_slots, n_odometry, min_inliers, loop_min_inliers, capacity, (int *)logged, (int *)status);
    return launched();
}
