// pose_common.h - what the pose kernels share (pose_estimate.hip, pose_refine.hip): a pair's rows, the back-projection, the score of
// a pose on a row, and the workgroup's float64 sums in the order include/sslam_hip.h states.
#pragma once
#include "common.h"

namespace {

constexpr int POSE_MAX_N1 = SSLAM_EVAL_MAX_K;
constexpr int POSE_CHUNK = 1024;         // usable rows in LDS at a time
constexpr int POSE_THREADS = 256;      // the workgroup, whatever n_hyp: ONE order of the refit's float64 sums per n_usable
constexpr int POSE_WAVES = POSE_THREADS / 64;

inline bool finite_positive(double v) { return v > 0.0 && v - v == 0.0; }

struct PoseCamera {
    double fx, fy, cx, cy, depth_scale, scale_x, scale_y;
};

struct PoseRow {
    double ax, ay, az, bx, by, bz;      // X_a, X_b
    float2 kb;                          // frame b's keypoint
};

struct PosePair {
    const float2 *f1, *f2;
    const int *d1, *d2;
    const long long *matches;
    int K;
};

// the back-projection of sslam_pose_depth_nn_pairs
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

// a USABLE slot's row
__device__ __forceinline__ PoseRow pose_row(const PosePair &pp, int slot, const PoseCamera &cam) {
    const long long i1 = pp.matches[2 * slot], i2 = pp.matches[2 * slot + 1];
    PoseRow r;
    r.kb = pp.f2[i2];
    pose_back_project(pp.f1[i1], pp.d1[i1], cam, r.ax, r.ay, r.az);
    pose_back_project(r.kb, pp.d2[i2], cam, r.bx, r.by, r.bz);
    return r;
}

// X_a under [R | t], projected into frame b, in keypoint units: the inlier test and the squared distance
__device__ __forceinline__ bool pose_inlier(const double *m, double X, double Y, double Z, const float2 kb, const PoseCamera &cam,
                                            double threshold, double &s) {
    const double X2 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
    const double Y2 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
    const double Z2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
    const double u2 = (cam.fx * X2) / Z2 + cam.cx, v2 = (cam.fy * Y2) / Z2 + cam.cy;
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
