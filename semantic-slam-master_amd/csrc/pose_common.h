// pose_common.h - what the pose kernels share (evaluate.hip, pose_estimate.hip, pose_refine.hip): the camera and the argument checks
// of the depth-taking entries, a pair's rows and the list of its usable ones, the back-projection, the projection under a pose, the
// score of a pose on a row, and the workgroup's float64 sums in the order include/sslam_hip.h states.
#pragma once
#include "common.h"

namespace {

constexpr int POSE_MAX_N1 = SSLAM_EVAL_MAX_K;
constexpr int POSE_CHUNK = 1024;         // usable rows in LDS at a time
constexpr int POSE_THREADS = 256;      // the workgroup, whatever n_hyp: ONE order of the refit's float64 sums per n_usable
constexpr int POSE_WAVES = POSE_THREADS / 64;

inline bool finite_positive(double v) { return v > 0.0 && v - v == 0.0; }
inline bool finite_nonnegative(double v) { return v >= 0.0 && v - v == 0.0; }      // a threshold: no NaN, negative or infinite one

struct PoseCamera {
    double fx, fy, cx, cy, depth_scale, scale_x, scale_y;
};

// What the entries that take a depth bank check alike - every failure is an invalid argument: the camera, the scales and the view,
// the threshold, and the bank and pair-list pointers.
inline bool pose_args_ok(const float *kp_bank, const int32_t *kp_depth_bank, const int32_t *pair_first, const int32_t *pair_second,
                         double fx, double fy, double cx, double cy, double depth_scale, double scale_x, double scale_y, double view_w,
                         double view_h, double threshold) {
    if (!kp_bank || !kp_depth_bank || !pair_first || !pair_second) return false;
    if (!finite_nonnegative(threshold)) return false;
    if (!finite_positive(fx) || !finite_positive(fy) || !finite_positive(depth_scale) || !finite_positive(scale_x) ||
        !finite_positive(scale_y))
        return false;
    if (cx - cx != 0.0 || cy - cy != 0.0 || !finite_positive(view_w) || !finite_positive(view_h)) return false;
    return !((uintptr_t)kp_bank & 7) && !sslam_misaligned(4, kp_depth_bank, pair_first, pair_second);
}

struct PoseRow {
    double ax, ay, az, bx, by, bz;      // X_a, X_b
    float2 kb;                          // frame b's keypoint
};

struct PosePair {
    const float2 *f1, *f2;
    const int *d1, *d2;
    const long long *matches;
    int K, count;                       // count: the list's, clamped to its n1 slots
    bool present;                       // both frames lie in the bank (uniform over the workgroup)
};

// workgroup p's pair; an absent pair reads frame 0 and has no usable row
__device__ __forceinline__ PosePair pose_pair(const float *kp_bank, const int *kp_depth_bank, int n_bank, int K, const int *pair_first,
                                              const int *pair_second, const long long *matches, const int *count, int n1, long long p) {
    const int a = pair_first[p], b = pair_second[p];
    PosePair pp;
    pp.present = (unsigned)a < (unsigned)n_bank && (unsigned)b < (unsigned)n_bank;
    const int cnt = count[p];
    pp.count = cnt < 0 ? 0 : (cnt > n1 ? n1 : cnt);
    pp.f1 = reinterpret_cast<const float2 *>(kp_bank) + (long long)(pp.present ? a : 0) * K;
    pp.f2 = reinterpret_cast<const float2 *>(kp_bank) + (long long)(pp.present ? b : 0) * K;
    pp.d1 = kp_depth_bank + (long long)(pp.present ? a : 0) * K;
    pp.d2 = kp_depth_bank + (long long)(pp.present ? b : 0) * K;
    pp.matches = matches + p * n1 * 2;
    pp.K = K;
    return pp;
}

// a keypoint and the raw depth under it, in the camera's metres
__device__ __forceinline__ void pose_back_project(const float2 q, int d, const PoseCamera &cam, double &X, double &Y, double &Z) {
    const double u = (double)q.x * cam.scale_x, v = (double)q.y * cam.scale_y, z = (double)d / cam.depth_scale;
    X = ((u - cam.cx) * z) / cam.fx;
    Y = ((v - cam.cy) * z) / cam.fy;
    Z = z;
}

__device__ __forceinline__ bool pose_usable(const PosePair &pp, int slot) {
    const long long i1 = pp.matches[2 * slot], i2 = pp.matches[2 * slot + 1];
    if (i1 < 0 || i1 >= pp.K || i2 < 0 || i2 >= pp.K) return false;
    return pp.d1[i1] > 0 && pp.d2[i2] > 0;
}

// The usable rows in list order: uslot[u] is the slot of the u-th one.  A slot that is not usable gets its mask entry here (-1 a
// listed row without depth, 0 past the count or of an absent pair), a usable one is left to the caller.  Every thread of the
// workgroup calls it (two barriers per POSE_THREADS slots) and gets the number of usable rows.
__device__ __forceinline__ int pose_list_usable(const PosePair &pp, int n1, unsigned short *uslot, int *wcnt, int *inlier_of_slot,
                                                int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    int n_usable = 0;
    for (int base = 0; base < n1; base += POSE_THREADS) {
        const int r = base + tid;
        const bool use = pp.present && r < pp.count && pose_usable(pp, r);
        if (r < n1 && !use) inlier_of_slot[r] = (pp.present && r < pp.count) ? -1 : 0;
        const unsigned long long mk = __ballot(use);
        if (lane == 0) wcnt[wave] = __popcll(mk);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < POSE_WAVES; w++) {
            const int n = wcnt[w];
            if (w < wave) before += n;
            total += n;
        }
        if (use) uslot[n_usable + before + __popcll(mk & ((1ull << lane) - 1ull))] = (unsigned short)r;
        n_usable += total;
        __syncthreads();
    }
    return n_usable;
}

// a USABLE slot's row
__device__ __forceinline__ PoseRow pose_row(const PosePair &pp, int slot, const PoseCamera &cam) {
    const long long i1 = pp.matches[2 * slot], i2 = pp.matches[2 * slot + 1];
    PoseRow r;
    r.kb = pp.f2[i2];
    pose_back_project(pp.f1[i1], pp.d1[i1], cam, r.ax, r.ay, r.az);
    pose_back_project(r.kb, pp.d2[i2], cam, r.bx, r.by, r.bz);
    return r;
}

// a point under [R | t], projected into the other camera: the depth pixel (u2, v2) and the depth Z2 there
__device__ __forceinline__ void pose_project(const double *m, double X, double Y, double Z, const PoseCamera &cam, double &u2, double &v2,
                                             double &Z2) {
    const double X2 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
    const double Y2 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
    Z2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
    u2 = (cam.fx * X2) / Z2 + cam.cx;
    v2 = (cam.fy * Y2) / Z2 + cam.cy;
}

// X_a under [R | t], projected into frame b, in keypoint units: the inlier test and the squared distance
__device__ __forceinline__ bool pose_inlier(const double *m, double X, double Y, double Z, const float2 kb, const PoseCamera &cam,
                                            double threshold, double &s) {
    double u2, v2, Z2;
    pose_project(m, X, Y, Z, cam, u2, v2, Z2);
    const double dx = u2 / cam.scale_x - (double)kb.x, dy = v2 / cam.scale_y - (double)kb.y;
    s = dx * dx + dy * dy;
    return Z2 > 0.0 && __builtin_sqrt(s) < threshold;      // a NaN fails both
}

__device__ __forceinline__ bool pose_finite(const double *m) {
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 12; e++) ok = ok && (m[e] - m[e] == 0.0);
    return ok;
}

// The float64 sums of the refit: thread t has added, from +0.0, the terms of the usable rows t, t + 256, ...
// ascending (a row that is no inlier adds +0.0); here lanes by xor 32 .. 1, then the four waves in order.  Every thread of the
// workgroup calls it (two barriers) and gets the totals.
template <int N>
__device__ __forceinline__ void pose_block_sum(double (&part)[N], double *wsum, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int e = 0; e < N; e++) {
        double p = part[e];
        p = p + __shfl_xor(p, 32);
        p = p + __shfl_xor(p, 16);
        p = p + __shfl_xor(p, 8);
        p = p + __shfl_xor(p, 4);
        p = p + __shfl_xor(p, 2);
        p = p + __shfl_xor(p, 1);
        if (lane == 0) wsum[wave * N + e] = p;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < N; e++) part[e] = ((wsum[e] + wsum[N + e]) + wsum[2 * N + e]) + wsum[3 * N + e];
    __syncthreads();                                     // wsum may be written again
}

__device__ __forceinline__ int pose_block_count(int n, int *wcnt, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) wcnt[wave] = n;
    __syncthreads();
    n = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
    __syncthreads();
    return n;
}

}  // namespace
