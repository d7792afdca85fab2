// pose_refine_common.h - what the two refinement kernels share (csrc/pose_refine.hip, csrc_weight/weighted_refine.hip): the layout of
// the 28 sums, a row's terms, the 6 x 6 solve, the pose update and the whole workgroup body - selection, passes, accept loop, keep
// rule, outputs.  The body is one template: WEIGHTED false is sslam_pose_refine_pairs as include/sslam_hip.h states it, WEIGHTED
// true multiplies a row's terms by its weight as include/sslam_weight.h states it.  Nothing of the weighted form is compiled into
// the unweighted instantiation: no weight is read, staged or multiplied there.
#pragma once
#include "pose_common.h"

namespace {

constexpr int REFINE_MAX_ITER = SSLAM_REFINE_MAX_ITER;
constexpr int REFINE_SUMS = 28;          // cost, H's upper triangle row-major (21), g (6)

__device__ __forceinline__ constexpr int refine_h(int i, int j) {      // H(i, j) in the sums, either triangle
    return i <= j ? 1 + 6 * i - (i * (i - 1)) / 2 + (j - i) : 1 + 6 * j - (j * (j - 1)) / 2 + (i - j);
}

// a selected row's terms under [R | t] added to the thread's partial sums (an unselected row adds +0.0 to each); WEIGHTED: the
// row's weight g multiplies rho, and g * w stands where w stood
template <bool WEIGHTED>
__device__ __forceinline__ void refine_terms(const double *m, double X, double Y, double Z, const float2 kb, const PoseCamera &cam, double kx,
                                             double ky, double huber, bool sel, double g, double (&S)[REFINE_SUMS], int &behind) {
    const double X2 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
    const double Y2 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
    const double Z2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
    const double u2 = (cam.fx * X2) / Z2 + cam.cx, v2 = (cam.fy * Y2) / Z2 + cam.cy;
    const double rx = u2 / cam.scale_x - (double)kb.x, ry = v2 / cam.scale_y - (double)kb.y;
    const double s = rx * rx + ry * ry, d = __builtin_sqrt(s);
    const bool quad = d <= huber;                        // a NaN takes the linear branch and stays a NaN
    const double w0 = quad ? 1.0 : huber / d;
    const double rho0 = quad ? s : (2.0 * huber) * d - huber * huber;
    const double w = WEIGHTED ? g * w0 : w0, rho = WEIGHTED ? g * rho0 : rho0;
    const double iz = 1.0 / Z2, a = kx * iz, b = ky * iz, c = -(a * (X2 * iz)), e = -(b * (Y2 * iz));
    const double Ju[6] = {a, 0.0, c, c * Y2, a * Z2 - c * X2, -(a * Y2)};
    const double Jv[6] = {0.0, b, e, e * Y2 - b * Z2, -(e * X2), b * X2};
    S[0] = S[0] + (sel ? rho : 0.0);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) S[refine_h(i, j)] = S[refine_h(i, j)] + (sel ? w * (Ju[i] * Ju[j] + Jv[i] * Jv[j]) : 0.0);
#pragma unroll
    for (int i = 0; i < 6; i++) S[22 + i] = S[22 + i] + (sel ? w * (Ju[i] * rx + Jv[i] * ry) : 0.0);
    behind += sel && !(Z2 > 0.0);
}

// H delta = -g by an unpivoted LDL^T, every index static; false at the first pivot that is not finite and > 0
__device__ __forceinline__ bool refine_solve(const double (&S)[REFINE_SUMS], double (&delta)[6]) {
    double L[6][6], D[6], y[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double v = S[refine_h(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) v = v - (L[j][k] * L[j][k]) * D[k];
        D[j] = v;
        ok = ok && v > 0.0 && v - v == 0.0;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = S[refine_h(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - (L[i][k] * L[j][k]) * D[k];
            L[i][j] = s / v;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = -S[22 + i];
#pragma unroll
        for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double v = y[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v = v - L[k][i] * delta[k];
        delta[i] = v;
    }
    return ok;
}

// [R | t] <- [dR R | dR t + v] with dR from the unit quaternion of (1, wx / 2, wy / 2, wz / 2)
__device__ __forceinline__ void refine_update(const double *m, const double (&delta)[6], double *out) {
    double w = 1.0, x = 0.5 * delta[3], y = 0.5 * delta[4], z = 0.5 * delta[5];
    const double nrm = __builtin_sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm;
    x = x / nrm;
    y = y / nrm;
    z = z / nrm;
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    double R[9];
    R[0] = ((ww + xx) - yy) - zz;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = ((ww - xx) + yy) - zz;
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = ((ww - xx) - yy) + zz;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[4 * i + j] = (R[3 * i] * m[j] + R[3 * i + 1] * m[4 + j]) + R[3 * i + 2] * m[8 + j];
        out[4 * i + 3] = ((R[3 * i] * m[3] + R[3 * i + 1] * m[7]) + R[3 * i + 2] * m[11]) + delta[i];
    }
}

// a weight that a row is selected with: finite and > 0 (a NaN, an infinity, either zero and a negative fail; a subnormal passes)
__device__ __forceinline__ bool refine_weight_ok(float g) { return g > 0.0f && g - g == 0.0f; }

// The workgroup of pair blockIdx.x, every thread of it.  WEIGHTED false: `weight` and `weight_sum` are not touched.
template <bool WEIGHTED>
__device__ __forceinline__ void pose_refine_body(const float *__restrict__ kp_bank, const int *__restrict__ kp_depth_bank, int n_bank, int K,
                                                 const int *__restrict__ pair_first, const int *__restrict__ pair_second,
                                                 const long long *__restrict__ matches, const int *__restrict__ count, int n1,
                                                 const PoseCamera &cam, double threshold, const double *T_in, double huber, int n_iter,
                                                 const float *__restrict__ weight, double *T_out, int *__restrict__ status,
                                                 int *__restrict__ iterations, int *__restrict__ selected_count,
                                                 int *__restrict__ usable_count, int *__restrict__ inlier_count_in,
                                                 int *__restrict__ inlier_count, int *__restrict__ inlier_of_slot,
                                                 double *__restrict__ cost_in, double *__restrict__ cost_out, double *__restrict__ rms,
                                                 double *__restrict__ info, double *__restrict__ weight_sum) {
    __shared__ unsigned short uslot[POSE_MAX_N1];        // the slot of the u-th usable row
    __shared__ double c_x[POSE_CHUNK], c_y[POSE_CHUNK], c_z[POSE_CHUNK];
    __shared__ float2 c_kb[POSE_CHUNK];
    __shared__ float c_g[WEIGHTED ? POSE_CHUNK : 1];     // the weights of the chunk's rows (WEIGHTED only)
    __shared__ double wsum[POSE_WAVES * REFINE_SUMS];
    __shared__ int wcnt[POSE_WAVES];

    const int tid = threadIdx.x, nt = POSE_THREADS;
    const long long p = blockIdx.x;
    inlier_of_slot += p * n1;
    T_out += p * 12;
    T_in += p * 12;
    info += p * 21;
    if constexpr (WEIGHTED) weight += p * n1;
    const PosePair pp = pose_pair(kp_bank, kp_depth_bank, n_bank, K, pair_first, pair_second, matches, count, n1, p);

    // ---- the usable rows in list order, as the RANSAC kernel lists them; a slot that is not usable gets its mask entry there
    const int n_usable = pose_list_usable(pp, n1, uslot, wcnt, inlier_of_slot, tid);

    double tin[12];
#pragma unroll
    for (int e = 0; e < 12; e++) tin[e] = T_in[e];
    const bool fin_in = pose_finite(tin);

    // ---- the first chunk into LDS, and the selection: the inliers of T_in, one bit per row of this thread
    const int n_lds = n_usable < POSE_CHUNK ? n_usable : POSE_CHUNK;
    for (int i = tid; i < n_lds; i += nt) {
        const PoseRow r = pose_row(pp, uslot[i], cam);
        c_x[i] = r.ax;
        c_y[i] = r.ay;
        c_z[i] = r.az;
        c_kb[i] = r.kb;
        if constexpr (WEIGHTED) c_g[i] = weight[uslot[i]];
    }
    __syncthreads();
    unsigned selected = 0u;
    int n_sel = 0, n_in = 0;
    double gs[1] = {0.0};
    for (int u = tid, k = 0; u < n_usable; u += nt, k++) {
        double X, Y, Z, s;
        float2 kb;
        if (u < POSE_CHUNK) {
            X = c_x[u], Y = c_y[u], Z = c_z[u], kb = c_kb[u];
        } else {
            const PoseRow r = pose_row(pp, uslot[u], cam);
            X = r.ax, Y = r.ay, Z = r.az, kb = r.kb;
        }
        bool in = pose_inlier(tin, X, Y, Z, kb, cam, threshold, s) && fin_in;
        if constexpr (WEIGHTED) {
            const float g = u < POSE_CHUNK ? c_g[u] : weight[uslot[u]];
            n_in += in;
            in = in && refine_weight_ok(g);
            gs[0] = gs[0] + (in ? (double)g : 0.0);
        }
        selected |= (unsigned)in << k;
        n_sel += in;
    }
    n_sel = pose_block_count(n_sel, wcnt, tid);
    if constexpr (WEIGHTED) {
        n_in = pose_block_count(n_in, wcnt, tid);
        pose_block_sum<1>(gs, wsum, tid);
    } else {
        n_in = n_sel;
    }

    if (n_sel < 3) {                                     // not attempted (uniform): absent, a non-finite T_in, too few selected rows
        for (int u = tid; u < n_usable; u += nt) inlier_of_slot[uslot[u]] = 0;
        if (tid < 12) T_out[tid] = T_in[tid];
        if (tid >= 64 && tid < 64 + 21) info[tid - 64] = 0.0;
        if (tid == 0) {
            status[p] = 3;
            iterations[p] = 0;
            selected_count[p] = 0;
            usable_count[p] = 0;
            inlier_count_in[p] = 0;
            inlier_count[p] = 0;
            cost_in[p] = 0.0;
            cost_out[p] = 0.0;
            rms[p] = 0.0;
            if constexpr (WEIGHTED) weight_sum[p] = 0.0;
        }
        return;
    }

    // ---- pass 0 at T_in, pass k at the k-th trial; a trial that does not lower the cost ends the iteration
    const double kx = cam.fx / cam.scale_x, ky = cam.fy / cam.scale_y;
    double cur[12], trial[12], best[REFINE_SUMS];
    double c_in = 0.0;
    int accepted = 0;
#pragma unroll
    for (int e = 0; e < 12; e++) cur[e] = trial[e] = tin[e];
#pragma unroll 1
    for (int pass = 0; pass <= n_iter; pass++) {
        double S[REFINE_SUMS];
#pragma unroll
        for (int e = 0; e < REFINE_SUMS; e++) S[e] = 0.0;
        int behind = 0;
        for (int u = tid, k = 0; u < n_usable; u += nt, k++) {
            double X, Y, Z, g = 1.0;
            float2 kb;
            if (u < POSE_CHUNK) {
                X = c_x[u], Y = c_y[u], Z = c_z[u], kb = c_kb[u];
                if constexpr (WEIGHTED) g = (double)c_g[u];
            } else {
                const int slot = uslot[u];
                const PoseRow r = pose_row(pp, slot, cam);
                X = r.ax, Y = r.ay, Z = r.az, kb = r.kb;
                if constexpr (WEIGHTED) g = (double)weight[slot];
            }
            refine_terms<WEIGHTED>(trial, X, Y, Z, kb, cam, kx, ky, huber, (selected >> k) & 1u, g, S, behind);
        }
        pose_block_sum<REFINE_SUMS>(S, wsum, tid);
        behind = pose_block_count(behind, wcnt, tid);
        if (pass == 0) {
            c_in = S[0];
            if (tid == 0) cost_in[p] = c_in;
        } else {
            if (!(S[0] - S[0] == 0.0 && behind == 0 && S[0] < best[0])) break;      // uniform: every thread holds the same totals
            accepted++;
#pragma unroll
            for (int e = 0; e < 12; e++) cur[e] = trial[e];
        }
#pragma unroll
        for (int e = 0; e < REFINE_SUMS; e++) best[e] = S[e];
        if (pass == 0 && tid == 0) {
#pragma unroll
            for (int e = 0; e < 21; e++) info[e] = S[1 + e];                          // H at T_in: what stays unless a refined pose is returned
        }
        if (pass == n_iter) break;
        double delta[6];
        if (!refine_solve(best, delta)) break;
        refine_update(cur, delta, trial);
    }

    // ---- the keep rule: the refined pose over ALL usable rows; with fewer inliers than T_in has, T_in stays
    int st = accepted > 0 ? 0 : 1, final_n = 0;
    double sq[1] = {0.0};
#pragma unroll 1
    for (int attempt = 0; attempt < 2; attempt++) {
        const bool fin = pose_finite(cur);
        int n = 0;
        sq[0] = 0.0;
        for (int u = tid; u < n_usable; u += nt) {
            const int slot = uslot[u];
            double X, Y, Z, s;
            float2 kb;
            if (u < POSE_CHUNK) {
                X = c_x[u], Y = c_y[u], Z = c_z[u], kb = c_kb[u];
            } else {
                const PoseRow r = pose_row(pp, slot, cam);
                X = r.ax, Y = r.ay, Z = r.az, kb = r.kb;
            }
            const bool in = pose_inlier(cur, X, Y, Z, kb, cam, threshold, s) && fin;
            inlier_of_slot[slot] = in;
            n += in;
            sq[0] = sq[0] + (in ? s : 0.0);
        }
        final_n = pose_block_count(n, wcnt, tid);
        pose_block_sum<1>(sq, wsum, tid);
        if (accepted == 0 || attempt == 1 || final_n >= n_in) break;
        st = 2;                                          // steps were accepted, but the result loses inliers: T_in, bit for bit
#pragma unroll
        for (int e = 0; e < 12; e++) cur[e] = tin[e];
    }
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 12; e++) T_out[e] = cur[e];
        status[p] = st;
        iterations[p] = accepted;
        selected_count[p] = n_sel;
        usable_count[p] = n_usable;
        inlier_count_in[p] = n_in;
        inlier_count[p] = final_n;
        cost_out[p] = st == 0 ? best[0] : c_in;
        rms[p] = final_n > 0 ? __builtin_sqrt(sq[0] / (double)final_n) : 0.0;
        if constexpr (WEIGHTED) weight_sum[p] = gs[0];
        if (st == 0) {
#pragma unroll
            for (int e = 0; e < 21; e++) info[e] = best[1 + e];
        }
    }
}

}  // namespace
