// edge_terms.h - the per-edge arithmetic of include/sslam_graph.h (AN EDGE, JACOBIANS, UPDATE), shared by csrc_graph/pose_graph.hip and
// csrc_loop/loop.hip: one statement of it, so both libraries give the same bits.  Included inside an anonymous namespace, through
// gauss_newton.h (the driver that calls it).
#pragma once

constexpr int STAGE = 90;           // words staged per edge: BB 21, BA 36, AA 21, GB 6, GA 6
constexpr int S_BB = 0, S_BA = 21, S_AA = 57, S_GB = 78, S_GA = 84;

__device__ __forceinline__ bool fin(double v) { return v - v == 0.0; }

__device__ __forceinline__ constexpr int tri_upper(int i, int j) {      // H(i, j) in the 21 words of info, either triangle
    return i <= j ? 6 * i - (i * (i - 1)) / 2 + (j - i) : 6 * j - (j * (j - 1)) / 2 + (i - j);
}
__device__ __forceinline__ constexpr int tri_lower(int i, int j) { return (i * (i + 1)) / 2 + j; }      // i >= j

// out = A o B
__device__ __forceinline__ void compose(const double *A, const double *B, double *out) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[4 * i + j] = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j];
        out[4 * i + 3] = ((A[4 * i] * B[3] + A[4 * i + 1] * B[7]) + A[4 * i + 2] * B[11]) + A[4 * i + 3];
    }
}

__device__ __forceinline__ void inverse(const double *A, double *out) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[4 * i + j] = A[4 * j + i];
        out[4 * i + 3] = -((A[i] * A[3] + A[4 + i] * A[7]) + A[8 + i] * A[11]);
    }
}

__device__ __forceinline__ double sum6(const double (&x)[6]) { return ((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) + x[5]; }

struct Edge {
    double Tp[12], H[21], Hr[6], s, w, rho;
};

// the edge (Ca, Cb, Tm, info) at the poses: T_p, r, H r, s, w, rho
__device__ __forceinline__ void edge_eval(const double *Ca, const double *Cb, const double *Tm, const double *info, double chi, Edge &e) {
    double ca[12], cb[12], tm[12], ai[12], mi[12], D[12];
#pragma unroll
    for (int k = 0; k < 12; k++) ca[k] = Ca[k], cb[k] = Cb[k], tm[k] = Tm[k];
#pragma unroll
    for (int k = 0; k < 21; k++) e.H[k] = info[k];
    inverse(ca, ai);
    compose(cb, ai, e.Tp);
    inverse(tm, mi);
    compose(e.Tp, mi, D);
    const double r[6] = {D[3], D[7], D[11], 0.5 * (D[9] - D[6]), 0.5 * (D[2] - D[8]), 0.5 * (D[4] - D[1])};
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int k = 0; k < 6; k++) x[k] = e.H[tri_upper(i, k)] * r[k];
        e.Hr[i] = sum6(x);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) x[k] = r[k] * e.Hr[k];
    e.s = sum6(x);
    const bool quad = e.s <= chi * chi;                  // a NaN takes the linear branch and stays a NaN
    const double q = __builtin_sqrt(e.s);
    e.w = quad ? 1.0 : chi / q;
    e.rho = quad ? e.s : (2.0 * chi) * q - chi * chi;
}

// the 90 staged words of an edge from its evaluation
__device__ __forceinline__ void edge_stage(const Edge &e, double *st) {
    double Ad[6][6];
    const double *m = e.Tp;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Ad[i][j] = m[4 * i + j];
            Ad[3 + i][3 + j] = m[4 * i + j];
            Ad[3 + i][j] = 0.0;
        }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        Ad[0][3 + j] = m[7] * m[8 + j] - m[11] * m[4 + j];
        Ad[1][3 + j] = m[11] * m[j] - m[3] * m[8 + j];
        Ad[2][3 + j] = m[3] * m[4 + j] - m[7] * m[j];
    }
    double P[6][6], x[6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
#pragma unroll
            for (int k = 0; k < 6; k++) x[k] = e.H[tri_upper(i, k)] * Ad[k][j];
            P[i][j] = sum6(x);
            st[S_BA + 6 * i + j] = -(e.w * P[i][j]);
        }
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
#pragma unroll
            for (int k = 0; k < 6; k++) x[k] = Ad[k][i] * P[k][j];
            st[S_AA + tri_lower(i, j)] = e.w * sum6(x);
            st[S_BB + tri_lower(i, j)] = e.w * e.H[tri_upper(i, j)];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) x[k] = Ad[k][i] * e.Hr[k];
        st[S_GA + i] = -(e.w * sum6(x));
        st[S_GB + i] = e.w * e.Hr[i];
    }
}

// [R | t] <- [dR R | dR t + v] with dR from the unit quaternion of (1, wx / 2, wy / 2, wz / 2): sslam_pose_refine_pairs' update
__device__ __forceinline__ void pose_update(const double *m, const double *delta, double *out) {
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
