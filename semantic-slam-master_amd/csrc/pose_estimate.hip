// pose_estimate.hip - geometric verification: the relative pose of a frame pair from its match list and the depth under the keypoints.
//   sslam_pose_ransac_pairs  per listed pair: RANSAC over 3-point samples of the usable matches (both depths measured), every
//                            hypothesis solved by Horn's closed form (cyclic Jacobi on the 4 x 4 matrix, a fixed 8 sweeps), scored by
//                            reprojection into frame b, the best refitted over its inliers; the pose, the counts and the inlier mask.
// All arithmetic is float64 in the order include/sslam_hip.h states (-ffp-contract=off); the sampler is 64-bit integer arithmetic.
// One 256-thread workgroup per pair, one thread per hypothesis, 256 hypotheses at a time.  LDS: the slots of the usable rows in list order (8 KB), one chunk of
// POSE_CHUNK rows - X_a as three doubles and frame b's keypoint as a float2, 32 KB - that every hypothesis reads at one address
// per step (a broadcast), and the partials of the reductions.  No atomics, no scratch, no allocation, no host read: capturable.
#include "pose_common.h"

namespace {

constexpr int POSE_MAX_HYP = SSLAM_POSE_MAX_HYP;

// splitmix64's finalizer
__device__ __forceinline__ unsigned long long pose_mix(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
// draw `draw` (0, 1, 2) of hypothesis h from a range of n: a function of (seed, h, draw) alone
__device__ __forceinline__ int pose_draw(unsigned long long seed, int h, int draw, int n) {
    const unsigned long long x = pose_mix(seed + 0x9e3779b97f4a7c15ull * (unsigned long long)(3 * h + draw + 1));
    return (int)(((x >> 32) * (unsigned long long)n) >> 32);
}

// one Jacobi rotation on (P, Q) of the symmetric a (upper triangle kept) and the eigenvector matrix v, indices static
template <int P, int Q>
__device__ __forceinline__ void pose_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double at = __builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / at;
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    a[P][P] = a[P][P] - h;
    a[Q][Q] = a[Q][Q] + h;
    a[P][Q] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r != P && r != Q) {
            double &arp = r < P ? a[r][P] : a[P][r], &arq = r < Q ? a[r][Q] : a[Q][r];
            const double g = arp, k = arq;
            arp = c * g - s * k;
            arq = s * g + c * k;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const double g = v[r][P], k = v[r][Q];
        v[r][P] = c * g - s * k;
        v[r][Q] = s * g + c * k;
    }
}

// Horn's closed form from the centroids and the cross-covariance M[i][j] = sum (X_a - c_a)_i (X_b - c_b)_j: [R | t] with X_b = R X_a + t
__device__ __forceinline__ void pose_horn(const double *M, const double *ca, const double *cb, double *T) {
    const double Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
    double a[4][4], v[4][4];
    a[0][0] = (Sxx + Syy) + Szz;
    a[0][1] = Syz - Szy;
    a[0][2] = Szx - Sxz;
    a[0][3] = Sxy - Syx;
    a[1][1] = (Sxx - Syy) - Szz;
    a[1][2] = Sxy + Syx;
    a[1][3] = Szx + Sxz;
    a[2][2] = (Syy - Sxx) - Szz;
    a[2][3] = Syz + Szy;
    a[3][3] = (Szz - Sxx) - Syy;
    a[1][0] = a[2][0] = a[2][1] = a[3][0] = a[3][1] = a[3][2] = 0.0;      // never read
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) v[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 8; sweep++) {
        pose_rotate<0, 1>(a, v);
        pose_rotate<0, 2>(a, v);
        pose_rotate<0, 3>(a, v);
        pose_rotate<1, 2>(a, v);
        pose_rotate<1, 3>(a, v);
        pose_rotate<2, 3>(a, v);
    }
    // the column of the largest diagonal entry, the lowest index on equality
    double best = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (a[j][j] > best) {
            best = a[j][j];
            w = v[0][j];
            x = v[1][j];
            y = v[2][j];
            z = v[3][j];
        }
    const double nrm = __builtin_sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm;
    x = x / nrm;
    y = y / nrm;
    z = z / nrm;
    if (w < 0.0) {
        w = -w;
        x = -x;
        y = -y;
        z = -z;
    }
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
        T[4 * i] = R[3 * i];
        T[4 * i + 1] = R[3 * i + 1];
        T[4 * i + 2] = R[3 * i + 2];
        T[4 * i + 3] = cb[i] - ((R[3 * i] * ca[0] + R[3 * i + 1] * ca[1]) + R[3 * i + 2] * ca[2]);
    }
}


__global__ __launch_bounds__(POSE_THREADS) void pose_ransac_kernel(const float *__restrict__ kp_bank, const int *__restrict__ kp_depth_bank,
                                                            int n_bank, int K, const int *__restrict__ pair_first,
                                                            const int *__restrict__ pair_second, const long long *__restrict__ matches,
                                                            const int *__restrict__ count, int n1, PoseCamera cam, double threshold,
                                                            int n_hyp, unsigned long long seed, double *__restrict__ T_out,
                                                            int *__restrict__ inlier_count, int *__restrict__ usable_count,
                                                            int *__restrict__ best_hypothesis, int *__restrict__ refit_kept,
                                                            int *__restrict__ inlier_of_slot, double *__restrict__ rms) {
    __shared__ unsigned short uslot[POSE_MAX_N1];        // the slot of the u-th usable row
    __shared__ double c_x[POSE_CHUNK], c_y[POSE_CHUNK], c_z[POSE_CHUNK];
    __shared__ float2 c_kb[POSE_CHUNK];
    __shared__ double wsum[POSE_WAVES * 9];
    __shared__ double t_best[12];
    __shared__ unsigned long long wkey[POSE_WAVES];
    __shared__ int wcnt[POSE_WAVES];

    const int tid = threadIdx.x, nt = POSE_THREADS, lane = tid & 63, wave = tid >> 6;
    const long long p = blockIdx.x;
    inlier_of_slot += p * n1;
    T_out += p * 12;
    const PosePair pp = pose_pair(kp_bank, kp_depth_bank, n_bank, K, pair_first, pair_second, matches, count, n1, p);

    // ---- the usable rows in list order; every slot that is not usable gets its mask entry there, a usable one at the end
    const int n_usable = pose_list_usable(pp, n1, uslot, wcnt, inlier_of_slot, tid);

    if (n_usable < 3) {                                  // no pose (an absent pair has no usable row)
        for (int u = tid; u < n_usable; u += nt) inlier_of_slot[uslot[u]] = 0;
        if (tid < 12) T_out[tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
        if (tid == 0) {
            inlier_count[p] = 0;
            usable_count[p] = n_usable;
            best_hypothesis[p] = -1;
            refit_kept[p] = 0;
            rms[p] = 0.0;
        }
        return;
    }

    // ---- the hypotheses, POSE_THREADS at a time, one per thread: three distinct usable rows, Horn's closed form on them; then the
    // usable rows through LDS, a chunk at a time, every lane reading one address.  A thread keeps the best of its own hypotheses:
    // the most inliers, the lowest h on equality, as one 64-bit key
    unsigned long long key = 0ull;
    double mb[12];
#pragma unroll
    for (int e = 0; e < 12; e++) mb[e] = 0.0;
    const bool one_chunk = n_usable <= POSE_CHUNK;       // then the chunk is filled once and serves every round
    for (int h0 = 0; h0 < n_hyp; h0 += POSE_THREADS) {
        const int h = h0 + tid;
        const bool mine = h < n_hyp;
        double m[12];
        bool scored = false;
        if (mine) {
            const int i0 = pose_draw(seed, h, 0, n_usable);
            int i1 = pose_draw(seed, h, 1, n_usable - 1);
            i1 += i1 >= i0;
            const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
            int i2 = pose_draw(seed, h, 2, n_usable - 2);
            i2 += i2 >= lo;
            i2 += i2 >= hi;
            const PoseRow r0 = pose_row(pp, uslot[i0], cam), r1 = pose_row(pp, uslot[i1], cam), r2 = pose_row(pp, uslot[i2], cam);
            double ca[3], cb[3], M[9];
            ca[0] = (((0.0 + r0.ax) + r1.ax) + r2.ax) / 3.0;
            ca[1] = (((0.0 + r0.ay) + r1.ay) + r2.ay) / 3.0;
            ca[2] = (((0.0 + r0.az) + r1.az) + r2.az) / 3.0;
            cb[0] = (((0.0 + r0.bx) + r1.bx) + r2.bx) / 3.0;
            cb[1] = (((0.0 + r0.by) + r1.by) + r2.by) / 3.0;
            cb[2] = (((0.0 + r0.bz) + r1.bz) + r2.bz) / 3.0;
            const double A[3][3] = {{r0.ax - ca[0], r0.ay - ca[1], r0.az - ca[2]}, {r1.ax - ca[0], r1.ay - ca[1], r1.az - ca[2]},
                                    {r2.ax - ca[0], r2.ay - ca[1], r2.az - ca[2]}};
            const double B[3][3] = {{r0.bx - cb[0], r0.by - cb[1], r0.bz - cb[2]}, {r1.bx - cb[0], r1.by - cb[1], r1.bz - cb[2]},
                                    {r2.bx - cb[0], r2.by - cb[1], r2.bz - cb[2]}};
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) M[3 * i + j] = ((0.0 + A[0][i] * B[0][j]) + A[1][i] * B[1][j]) + A[2][i] * B[2][j];
            pose_horn(M, ca, cb, m);
            scored = pose_finite(m);                     // a hypothesis with a non-finite entry scores 0
        }
        int inl = 0;
        for (int s0 = 0; s0 < n_usable; s0 += POSE_CHUNK) {
            const int n = n_usable - s0 < POSE_CHUNK ? n_usable - s0 : POSE_CHUNK;
            if (!one_chunk || h0 == 0) {                 // uniform
                __syncthreads();                         // the chunk before is read
                for (int i = tid; i < n; i += POSE_THREADS) {
                    const PoseRow r = pose_row(pp, uslot[s0 + i], cam);
                    c_x[i] = r.ax;
                    c_y[i] = r.ay;
                    c_z[i] = r.az;
                    c_kb[i] = r.kb;
                }
                __syncthreads();
            }
            if (scored)
                for (int i = 0; i < n; i++) {
                    double s;
                    inl += pose_inlier(m, c_x[i], c_y[i], c_z[i], c_kb[i], cam, threshold, s);
                }
        }
        const unsigned long long k = ((unsigned long long)inl << 32) | (unsigned long long)(0xffffffffu - (unsigned)h);
        if (mine && k > key) {
            key = k;
#pragma unroll
            for (int e = 0; e < 12; e++) mb[e] = m[e];
        }
    }
    const unsigned long long own = key;
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if (lane == 0) wkey[wave] = key;
    __syncthreads();
    key = wkey[0];
    for (int w = 1; w < POSE_WAVES; w++) key = wkey[w] > key ? wkey[w] : key;
    const int best_h = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)), best_n = (int)(key >> 32);
    if (own == key) {                                    // keys are distinct: one thread
#pragma unroll
        for (int e = 0; e < 12; e++) t_best[e] = mb[e];
    }
    __syncthreads();
    double tb[12];
#pragma unroll
    for (int e = 0; e < 12; e++) tb[e] = t_best[e];

    // ---- the refit over the best hypothesis' inliers (with three at least): the same solver, the sums across threads
    int kept = 0, final_n = best_n;
    if (best_n >= 3) {                                   // uniform
        double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int u = tid; u < n_usable; u += POSE_THREADS) {
                const PoseRow r = pose_row(pp, uslot[u], cam);
                double s;
                const bool in = pose_inlier(tb, r.ax, r.ay, r.az, r.kb, cam, threshold, s);
                S[0] = S[0] + (in ? r.ax : 0.0);
                S[1] = S[1] + (in ? r.ay : 0.0);
                S[2] = S[2] + (in ? r.az : 0.0);
                S[3] = S[3] + (in ? r.bx : 0.0);
                S[4] = S[4] + (in ? r.by : 0.0);
                S[5] = S[5] + (in ? r.bz : 0.0);
            }
        pose_block_sum<6>(S, wsum, tid);
        const double nd = (double)best_n;
        const double ca[3] = {S[0] / nd, S[1] / nd, S[2] / nd}, cb[3] = {S[3] / nd, S[4] / nd, S[5] / nd};
        double M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int u = tid; u < n_usable; u += POSE_THREADS) {
                const PoseRow r = pose_row(pp, uslot[u], cam);
                double s;
                const bool in = pose_inlier(tb, r.ax, r.ay, r.az, r.kb, cam, threshold, s);
                const double A[3] = {r.ax - ca[0], r.ay - ca[1], r.az - ca[2]}, B[3] = {r.bx - cb[0], r.by - cb[1], r.bz - cb[2]};
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) M[3 * i + j] = M[3 * i + j] + (in ? A[i] * B[j] : 0.0);
            }
        pose_block_sum<9>(M, wsum, tid);
        double tr[12];
        pose_horn(M, ca, cb, tr);                        // every thread, from the same totals: the same bits
        int n_ref = 0;
        if (pose_finite(tr))
            for (int u = tid; u < n_usable; u += POSE_THREADS) {
                const PoseRow r = pose_row(pp, uslot[u], cam);
                double s;
                n_ref += pose_inlier(tr, r.ax, r.ay, r.az, r.kb, cam, threshold, s);
            }
        n_ref = pose_block_count(n_ref, wcnt, tid);
        if (n_ref >= best_n) {
            kept = 1;
            final_n = n_ref;
#pragma unroll
            for (int e = 0; e < 12; e++) tb[e] = tr[e];
        }
    }

    // ---- the mask of the usable rows and the root mean square under the pose that stays
    double sq[1] = {0.0};
    const bool fin = pose_finite(tb);
    for (int u = tid; u < n_usable; u += POSE_THREADS) {
            const int slot = uslot[u];
            const PoseRow r = pose_row(pp, slot, cam);
            double s;
            const bool in = pose_inlier(tb, r.ax, r.ay, r.az, r.kb, cam, threshold, s) && fin;
            inlier_of_slot[slot] = in;
            sq[0] = sq[0] + (in ? s : 0.0);
        }
    pose_block_sum<1>(sq, wsum, tid);
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 12; e++) T_out[e] = tb[e];
        inlier_count[p] = final_n;
        usable_count[p] = n_usable;
        best_hypothesis[p] = best_h;
        refit_kept[p] = kept;
        rms[p] = final_n > 0 ? __builtin_sqrt(sq[0] / (double)final_n) : 0.0;
    }
}

}  // namespace

extern "C" int sslam_pose_ransac_pairs(const float *kp_bank, const int32_t *kp_depth_bank, int n_bank, int K, const int32_t *pair_first,
                                       const int32_t *pair_second, int n_pairs, const int64_t *matches, const int32_t *count, int n1,
                                       double fx, double fy, double cx, double cy, double depth_scale, double scale_x, double scale_y,
                                       double view_w, double view_h, double threshold, int n_hyp, uint64_t seed, double *T,
                                       int32_t *inlier_count, int32_t *usable_count, int32_t *best_hypothesis, int32_t *refit_kept,
                                       int32_t *inlier_of_slot, double *rms, void *stream) {
    if (!pose_args_ok(kp_bank, kp_depth_bank, pair_first, pair_second, fx, fy, cx, cy, depth_scale, scale_x, scale_y, view_w, view_h,
                      threshold))
        return SSLAM_E_INVALID;
    if (!matches || !count || !T || !inlier_count || !usable_count || !best_hypothesis || !refit_kept || !inlier_of_slot || !rms)
        return SSLAM_E_INVALID;
    if (n_bank <= 0 || K <= 0 || n1 <= 0 || n_pairs <= 0 || n1 > K) return SSLAM_E_INVALID;
    if (n_hyp < 1 || n_hyp > POSE_MAX_HYP) return SSLAM_E_INVALID;
    if (sslam_misaligned(8, matches, T, rms) ||
        sslam_misaligned(4, count, inlier_count, usable_count, best_hypothesis, refit_kept, inlier_of_slot))
        return SSLAM_E_INVALID;
    if (K > POSE_MAX_N1) return SSLAM_E_UNSUPPORTED;
    const PoseCamera cam = {fx, fy, cx, cy, depth_scale, scale_x, scale_y};
    hipLaunchKernelGGL(pose_ransac_kernel, dim3((unsigned)n_pairs), dim3(POSE_THREADS), 0, (hipStream_t)stream, kp_bank, kp_depth_bank, n_bank,
                       K, pair_first, pair_second, (const long long *)matches, count, n1, cam, threshold, n_hyp,
                       (unsigned long long)seed, T, inlier_count, usable_count, best_hypothesis, refit_kept, inlier_of_slot, rms);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}
