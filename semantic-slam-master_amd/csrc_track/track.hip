// track.hip - libsslam_track.so: feature tracks and a landmark map (include/sslam_track.h states every rule and every floating-point
// operation; tests/track_ref.py restates them in numpy).
//   sslt_link_pairs   fill; a thread per row: atomicMin of the row index per frame; a workgroup per link row: lowest slots by atomicMin
//                     in LDS, the links; two passes that turn the per-frame row indices into frames.
//   sslt_track_ids    pointer jumping over (root, distance) pairs, ceil(log2 n_bank) rounds; a three-kernel exclusive scan of the
//                     root flags; ids, ages, lengths.
//   sslt_landmarks    fill; one thread per track walks its chain three times (float64, one order of sums).
//   sslt_track_step   one workgroup: the link-slot rule, inherited ids, new ids by a workgroup scan, the counters.
// All node indices n = frame * K + slot fit 31 bits (the entries refuse more); a grid's own index is formed in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sslam_track.h"

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;
constexpr int TILE = SSLT_SCAN_TILE;
constexpr int PER = TILE / NT;                           // nodes per thread of a scan tile, contiguous
constexpr int NONE = 0x7fffffff;

long long g_launches = 0;   // diagnostic launch counter (sslt_launch_count): relaxed atomic adds, the library's only mutable state

inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

__device__ __forceinline__ bool fin(double v) { return v - v == 0.0; }
__device__ __forceinline__ long long gid() { return (long long)blockIdx.x * NT + threadIdx.x; }

// ------------------------------------------------------------------------------------------------------------------- the links
__global__ __launch_bounds__(NT) void link_fill_kernel(int *__restrict__ prev, int *__restrict__ next, int *__restrict__ prev_frame,
                                                       int *__restrict__ next_frame, int n_bank, int N) {
    const long long n = gid();
    if (n < N) prev[n] = -1, next[n] = -1;
    if (n < n_bank) prev_frame[n] = NONE, next_frame[n] = NONE;
}

__device__ __forceinline__ bool row_valid(int a, int b, int n_bank) { return a >= 0 && a < b && b < n_bank; }

__global__ __launch_bounds__(NT) void link_rows_kernel(const int *__restrict__ first, const int *__restrict__ second, int n_pairs, int n_bank,
                                                       int *__restrict__ prev_frame, int *__restrict__ next_frame) {
    const long long p = gid();
    if (p >= n_pairs) return;
    const int a = first[p], b = second[p];
    if (!row_valid(a, b, n_bank)) return;
    atomicMin(&prev_frame[b], (int)p);
    atomicMin(&next_frame[a], (int)p);
}

__device__ __forceinline__ bool slot_valid(const long long *__restrict__ m, const int *__restrict__ mask, int j, int K, int &i1, int &i2) {
    const long long v1 = m[2 * (long long)j], v2 = m[2 * (long long)j + 1];
    if (v1 < 0 || v1 >= K || v2 < 0 || v2 >= K) return false;
    if (mask && mask[j] != 1) return false;
    i1 = (int)v1, i2 = (int)v2;
    return true;
}

// the lowest valid slot naming each idx1 (lo1) and each idx2 (lo2) of one row, NONE where there is none; ends with a barrier
__device__ __forceinline__ void lowest_slots(const long long *__restrict__ m, const int *__restrict__ mask, int cnt, int K, int *lo1, int *lo2) {
    for (int s = threadIdx.x; s < K; s += NT) lo1[s] = NONE, lo2[s] = NONE;
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += NT) {
        int i1, i2;
        if (slot_valid(m, mask, j, K, i1, i2)) atomicMin(&lo1[i1], j), atomicMin(&lo2[i2], j);
    }
    __syncthreads();
}

__device__ __forceinline__ int clamp_count(int c, int n1) { return c < 0 ? 0 : (c > n1 ? n1 : c); }

__global__ __launch_bounds__(NT) void link_slots_kernel(const int *__restrict__ first, const int *__restrict__ second,
                                                        const long long *__restrict__ matches, const int *__restrict__ count,
                                                        const int *__restrict__ mask, int n1, int n_bank, int K,
                                                        const int *__restrict__ prev_frame, const int *__restrict__ next_frame,
                                                        int *__restrict__ prev, int *__restrict__ next) {
    __shared__ int lo1[SSLT_MAX_K], lo2[SSLT_MAX_K];
    const int p = blockIdx.x;
    const int a = first[p], b = second[p];
    if (!row_valid(a, b, n_bank) || prev_frame[b] != p || next_frame[a] != p) return;      // uniform: no link row
    const long long *m = matches + (long long)p * n1 * 2;
    const int *mk = mask ? mask + (long long)p * n1 : nullptr;
    const int cnt = clamp_count(count[p], n1);
    lowest_slots(m, mk, cnt, K, lo1, lo2);
    for (int j = threadIdx.x; j < cnt; j += NT) {
        int i1, i2;
        if (slot_valid(m, mk, j, K, i1, i2) && lo1[i1] == j && lo2[i2] == j) next[a * K + i1] = i2, prev[b * K + i2] = i1;
    }
}

__global__ __launch_bounds__(NT) void link_prev_frame_kernel(const int *__restrict__ first, int n_bank, int *__restrict__ prev_frame,
                                                             const int *__restrict__ next_frame) {
    const long long f = gid();
    if (f >= n_bank) return;
    const int r = prev_frame[f];                          // the lowest valid row with second == f
    int v = -1;
    if (r != NONE) {
        const int a = first[r];
        if (next_frame[a] == r) v = a;
    }
    prev_frame[f] = v;
}

__global__ __launch_bounds__(NT) void link_next_frame_kernel(const int *__restrict__ second, int n_bank, const int *__restrict__ prev_frame,
                                                             int *__restrict__ next_frame) {
    const long long f = gid();
    if (f >= n_bank) return;
    const int r = next_frame[f];                          // the lowest valid row with first == f
    int v = -1;
    if (r != NONE) {
        const int b = second[r];
        if (prev_frame[b] == (int)f) v = b;               // prev_frame holds frames by now: that row is the link row (f, b)
    }
    next_frame[f] = v;
}

// ------------------------------------------------------------------------------------------------------------------- the tracks
__global__ __launch_bounds__(NT) void ids_init_kernel(const int *__restrict__ prev, const int *__restrict__ prev_frame, int K, int N,
                                                      int2 *__restrict__ rd, int *__restrict__ root_frame, int *__restrict__ root_slot,
                                                      int *__restrict__ length) {
    const long long g = gid();
    if (g >= N) return;
    const int n = (int)g, f = n / K;
    const int pf = prev_frame[f], ps = prev[n];
    const bool has = pf >= 0 && pf < f && ps >= 0 && ps < K;
    rd[n] = has ? make_int2(pf * K + ps, 1) : make_int2(n, 0);
    root_frame[n] = -1, root_slot[n] = -1, length[n] = 0;
}

__global__ __launch_bounds__(NT) void ids_jump_kernel(const int2 *__restrict__ src, int2 *__restrict__ dst, int N) {
    const long long g = gid();
    if (g >= N) return;
    const int2 me = src[g], up = src[me.x];
    dst[g] = make_int2(up.x, me.y + up.y);
}

// the sum of v over the workgroup's threads, and this thread's exclusive prefix; two barriers
__device__ __forceinline__ int block_exclusive(int v, int *wsum, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int i = 0; i < WAVES; i++) {
        if (i < w) base += wsum[i];
        total += wsum[i];
    }
    __syncthreads();                                     // wsum is written again
    return base + inc - v;
}

__global__ __launch_bounds__(NT) void ids_count_kernel(const int2 *__restrict__ rd, int N, int *__restrict__ tile_sum) {
    __shared__ int wsum[WAVES];
    const long long n0 = (long long)blockIdx.x * TILE + threadIdx.x * PER;
    int c = 0;
    for (int i = 0; i < PER; i++)
        if (n0 + i < N) c += rd[n0 + i].x == (int)(n0 + i);
    int total;
    block_exclusive(c, wsum, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum becomes its exclusive scan, n_tracks the total
__global__ __launch_bounds__(NT) void ids_scan_tiles_kernel(int *__restrict__ tile_sum, int n_tiles, int *__restrict__ n_tracks) {
    __shared__ int wsum[WAVES];
    int carry = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += NT) {
        const int i = t0 + threadIdx.x;
        const int v = i < n_tiles ? tile_sum[i] : 0;
        int total;
        const int ex = block_exclusive(v, wsum, total);
        if (i < n_tiles) tile_sum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) n_tracks[0] = carry;
}

__global__ __launch_bounds__(NT) void ids_number_kernel(const int2 *__restrict__ rd, const int *__restrict__ tile_sum, int K, int N,
                                                        int *__restrict__ id_of_root, int *__restrict__ root_frame, int *__restrict__ root_slot) {
    __shared__ int wsum[WAVES];
    const long long n0 = (long long)blockIdx.x * TILE + threadIdx.x * PER;
    bool root[PER];
    int c = 0;
    for (int i = 0; i < PER; i++) {
        root[i] = n0 + i < N && rd[n0 + i].x == (int)(n0 + i);
        c += root[i];
    }
    int total;
    int id = tile_sum[blockIdx.x] + block_exclusive(c, wsum, total);
    for (int i = 0; i < PER; i++)
        if (root[i]) {
            const int n = (int)(n0 + i), f = n / K;
            id_of_root[n] = id, root_frame[id] = f, root_slot[id] = n - f * K;
            id++;
        }
}

__global__ __launch_bounds__(NT) void ids_assign_kernel(const int2 *__restrict__ rd, const int *__restrict__ id_of_root, int N,
                                                        int *__restrict__ track_id, int *__restrict__ age, int *__restrict__ length) {
    const long long g = gid();
    if (g >= N) return;
    const int2 me = rd[g];
    const int id = id_of_root[me.x];
    track_id[g] = id, age[g] = me.y;
    atomicAdd(&length[id], 1);
}

// ---------------------------------------------------------------------------------------------------------------- the landmarks
struct Camera {
    double fx, fy, cx, cy, depth_scale, scale_x, scale_y;
};

__global__ __launch_bounds__(NT) void landmark_fill_kernel(double *__restrict__ residual, int *__restrict__ kept, int N) {
    const long long n = gid();
    if (n < N) residual[n] = -1.0, kept[n] = 0;
}

// member (f, s) as an observation: its weight, keypoint and C row -> true, with the world point.  Every load is made before any
// test - all of them are inside their arrays whatever the values - so that they travel together: the walk is one thread's chain of
// dependent loads, and its length in memory latencies is what the launch costs (tools/track_probe.py)
__device__ __forceinline__ bool observe(const float *__restrict__ kp, const int *__restrict__ depth, const double *__restrict__ C,
                                        const float *__restrict__ weight, const Camera &cam, int f, int n, double &g, double &x, double &y,
                                        double c[12], double Xw[3]) {
    const int d = depth[n];
    const float gf = weight ? weight[n] : 1.0f, xf = kp[2 * (long long)n], yf = kp[2 * (long long)n + 1];
    bool ok = true;
    for (int i = 0; i < 12; i++) c[i] = C[(long long)f * 12 + i], ok = ok && fin(c[i]);
    g = (double)gf, x = (double)xf, y = (double)yf;
    if (!(d > 0) || !(g > 0.0 && g - g == 0.0) || !ok) return false;
    const double u = x * cam.scale_x, v = y * cam.scale_y, z = (double)d / cam.depth_scale;
    const double X = ((u - cam.cx) * z) / cam.fx, Y = ((v - cam.cy) * z) / cam.fy;
    const double ex = X - c[3], ey = Y - c[7], ez = z - c[11];
    for (int j = 0; j < 3; j++) Xw[j] = (c[j] * ex + c[4 + j] * ey) + c[8 + j] * ez;
    return true;
}

__device__ __forceinline__ double score(const double c[12], const Camera &cam, const double L[3], double x, double y) {
    const double Xp = ((c[0] * L[0] + c[1] * L[1]) + c[2] * L[2]) + c[3];
    const double Yp = ((c[4] * L[0] + c[5] * L[1]) + c[6] * L[2]) + c[7];
    const double Zp = ((c[8] * L[0] + c[9] * L[1]) + c[10] * L[2]) + c[11];
    const double up = (cam.fx * Xp) / Zp + cam.cx, vp = (cam.fy * Yp) / Zp + cam.cy;
    const double dx = up / cam.scale_x - x, dy = vp / cam.scale_y - y;
    return Zp > 0.0 ? dx * dx + dy * dy : __builtin_huge_val();
}

// One track's chain and what an observation of it is judged by
struct Chain {
    const float *kp, *weight;
    const int *depth, *next, *next_frame;
    const double *C;
    Camera cam;
    int n_bank, K, root_frame, root_slot;
};

// The walk, the same in every pass: the members in ascending frame order, so it ends; body(n, g, x, y, c, Xw) on every member that is an
// observation.  The next member is asked for before this one is worked on.
template <typename Body>
__device__ __forceinline__ void walk(const Chain &t, Body body) {
    int f = t.root_frame, s = t.root_slot;
    if (!(f >= 0 && f < t.n_bank && s >= 0 && s < t.K)) return;
    double g, x, y, c[12], Xw[3];
    for (;;) {
        const int n = f * t.K + s;
        const int nf = t.next_frame[f], ns = t.next[n];
        if (observe(t.kp, t.depth, t.C, t.weight, t.cam, f, n, g, x, y, c, Xw)) body(n, g, x, y, c, Xw);
        if (!(nf > f && nf < t.n_bank && ns >= 0 && ns < t.K)) return;
        f = nf, s = ns;
    }
}

__global__ __launch_bounds__(NT) void landmark_kernel(const float *__restrict__ kp, const int *__restrict__ depth, const double *__restrict__ C,
                                                      int n_bank, int K, int N, Camera cam, double threshold, const int *__restrict__ next,
                                                      const int *__restrict__ next_frame, const int *__restrict__ root_frame,
                                                      const int *__restrict__ root_slot, const int *__restrict__ n_tracks_p,
                                                      const float *__restrict__ weight, int min_obs, double *__restrict__ xyz,
                                                      int *__restrict__ n_obs_o, int *__restrict__ n_kept_o, int *__restrict__ status_o,
                                                      double *__restrict__ weight_sum, double *__restrict__ rms, double *__restrict__ residual,
                                                      int *__restrict__ kept) {
    const long long gi = gid();
    if (gi >= N) return;
    const int i = (int)gi;
    int nt = n_tracks_p[0];
    nt = nt < 0 ? 0 : (nt > N ? N : nt);
    double L[3] = {0.0, 0.0, 0.0}, L0[3] = {0.0, 0.0, 0.0}, W = 0.0, ss = 0.0;
    int n_obs = 0, n_kept = 0, status = -1;
    if (i < nt) {
        const Chain t = {kp, weight, depth, next, next_frame, C, cam, n_bank, K, root_frame[i], root_slot[i]};
        double W0 = 0.0, S[3] = {0.0, 0.0, 0.0};
        walk(t, [&](int, double g, double, double, const double *, const double *Xw) {
            n_obs++;
            W0 = W0 + g;
            for (int j = 0; j < 3; j++) S[j] = S[j] + g * Xw[j];
        });
        status = 2;
        if (n_obs > 0) {
            for (int j = 0; j < 3; j++) L0[j] = S[j] / W0, S[j] = 0.0;
            walk(t, [&](int n, double g, double x, double y, const double *c, const double *Xw) {
                if (!(sqrt(score(c, cam, L0, x, y)) < threshold)) return;
                n_kept++;
                W = W + g;
                for (int j = 0; j < 3; j++) S[j] = S[j] + g * Xw[j];
                kept[n] = 1;
            });
            status = n_kept >= min_obs ? 0 : 1;
            for (int j = 0; j < 3; j++) L[j] = status == 0 ? S[j] / W : L0[j];
            walk(t, [&](int n, double, double x, double y, const double *c, const double *) {
                const double sc = score(c, cam, L, x, y);
                residual[n] = sqrt(sc);
                if (kept[n] == 1) ss = ss + sc;
            });
        }
    }
    for (int j = 0; j < 3; j++) xyz[3 * (long long)i + j] = L[j];
    n_obs_o[i] = n_obs, n_kept_o[i] = n_kept, status_o[i] = status;
    weight_sum[i] = W;
    rms[i] = n_kept > 0 ? sqrt(ss / (double)n_kept) : 0.0;
}

// ------------------------------------------------------------------------------------------------------------- the online step
__global__ __launch_bounds__(NT) void track_step_kernel(int *__restrict__ tp, int *__restrict__ next_id_p, int *__restrict__ prev,
                                                        int *__restrict__ next, int *__restrict__ prev_frame, int *__restrict__ next_frame,
                                                        int *__restrict__ track_id, int *__restrict__ age, const long long *__restrict__ matches,
                                                        const int *__restrict__ count, const int *__restrict__ mask,
                                                        const int *__restrict__ first, int n1, int K, int capacity,
                                                        int *__restrict__ out_track_id, int *__restrict__ out_age, int *__restrict__ n_new,
                                                        int *__restrict__ status) {
    __shared__ int lo1[SSLT_MAX_K], lo2[SSLT_MAX_K], pv[SSLT_MAX_K];
    __shared__ int wsum[WAVES];
    const int t = tp[0], id0 = next_id_p[0], tid = threadIdx.x;
    if (t < 0 || t >= capacity) {                        // uniform: the state is left alone
        for (int s = tid; s < K; s += NT) out_track_id[s] = -1, out_age[s] = -1;
        if (tid == 0) n_new[0] = 0, status[0] = 4;
        return;
    }
    const int a = first[0];
    const bool link_row = a >= 0 && a < t && next_frame[a] == -1;      // uniform
    for (int s = tid; s < K; s += NT) pv[s] = -1;
    if (link_row) {
        const int cnt = clamp_count(count[0], n1);
        lowest_slots(matches, mask, cnt, K, lo1, lo2);   // its first barrier also orders pv's fill before the stores below
        for (int j = tid; j < cnt; j += NT) {
            int i1, i2;
            if (slot_valid(matches, mask, j, K, i1, i2) && lo1[i1] == j && lo2[i2] == j) pv[i2] = i1, next[a * K + i1] = i2;
        }
    }
    __syncthreads();
    int carry = id0;
    for (int s0 = 0; s0 < K; s0 += NT) {                 // uniform trip count: the scan's barriers are met by every thread
        const int s = s0 + tid;
        const int p = s < K ? pv[s] : 0;
        const int fresh = s < K && p < 0;
        int total;
        const int ex = block_exclusive(fresh, wsum, total);
        if (s < K) {
            const int id = fresh ? carry + ex : track_id[a * K + p], ag = fresh ? 0 : age[a * K + p] + 1;
            const int n = t * K + s;
            prev[n] = p, next[n] = -1, track_id[n] = id, age[n] = ag;
            out_track_id[s] = id, out_age[s] = ag;
        }
        carry += total;
    }
    if (tid == 0) {
        prev_frame[t] = link_row ? a : -1, next_frame[t] = -1;
        if (link_row) next_frame[a] = t;
        n_new[0] = carry - id0, status[0] = 0;
        tp[0] = t + 1, next_id_p[0] = carry;             // every read of both counters and of next_frame[a] came before the barriers above
    }
}

inline int launched(void) {
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}

inline int bank_shape(int n_bank, int K) {
    if (n_bank <= 0 || K <= 0) return SSLAM_E_INVALID;
    return (long long)n_bank * K > 0x7fffffffLL ? SSLAM_E_UNSUPPORTED : SSLAM_OK;
}

inline unsigned groups(long long n) { return (unsigned)((n + NT - 1) / NT); }
inline bool positive(double v) { return v - v == 0.0 && v > 0.0; }

}  // namespace

extern "C" int sslt_version(void) { return 100; }
extern "C" const char *sslt_arch(void) { return "gfx950"; }
extern "C" long long sslt_launch_count(void) { return __atomic_load_n(&g_launches, __ATOMIC_RELAXED); }

extern "C" int sslt_link_pairs(const int32_t *pair_first, const int32_t *pair_second, int n_pairs, const int64_t *matches,
                               const int32_t *count, const int32_t *mask, int n1, int n_bank, int K, int32_t *prev, int32_t *next,
                               int32_t *prev_frame, int32_t *next_frame, void *stream) {
    for (const void *p : {(const void *)pair_first, (const void *)pair_second, (const void *)count, (const void *)prev, (const void *)next,
                          (const void *)prev_frame, (const void *)next_frame})
        if (!p || misaligned(p, 4)) return SSLAM_E_INVALID;
    if (!matches || misaligned(matches, 8) || misaligned(mask, 4)) return SSLAM_E_INVALID;
    if (n_pairs <= 0 || n1 <= 0 || n_bank <= 0 || K <= 0) return SSLAM_E_INVALID;
    if (K > SSLT_MAX_K || bank_shape(n_bank, K) != SSLAM_OK) return SSLAM_E_UNSUPPORTED;
    const int N = n_bank * K;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(link_fill_kernel, dim3(groups(N > n_bank ? N : n_bank)), dim3(NT), 0, st, (int *)prev, (int *)next, (int *)prev_frame,
                       (int *)next_frame, n_bank, N);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(link_rows_kernel, dim3(groups(n_pairs)), dim3(NT), 0, st, (const int *)pair_first, (const int *)pair_second, n_pairs,
                       n_bank, (int *)prev_frame, (int *)next_frame);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(link_slots_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, (const int *)pair_first, (const int *)pair_second,
                       (const long long *)matches, (const int *)count, (const int *)mask, n1, n_bank, K, (const int *)prev_frame,
                       (const int *)next_frame, (int *)prev, (int *)next);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(link_prev_frame_kernel, dim3(groups(n_bank)), dim3(NT), 0, st, (const int *)pair_first, n_bank, (int *)prev_frame,
                       (const int *)next_frame);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(link_next_frame_kernel, dim3(groups(n_bank)), dim3(NT), 0, st, (const int *)pair_second, n_bank,
                       (const int *)prev_frame, (int *)next_frame);
    return launched();
}

extern "C" size_t sslt_track_workspace_bytes(int n_bank, int K) {
    if (bank_shape(n_bank, K) != SSLAM_OK) return 0;
    const size_t N = (size_t)n_bank * (size_t)K;
    return 20 * N + 4 * ((N + TILE - 1) / TILE);
}

extern "C" int sslt_track_ids(const int32_t *prev, const int32_t *prev_frame, int n_bank, int K, void *workspace, int32_t *track_id,
                              int32_t *age, int32_t *n_tracks, int32_t *root_frame, int32_t *root_slot, int32_t *length, void *stream) {
    for (const void *p : {(const void *)prev, (const void *)prev_frame, (const void *)track_id, (const void *)age, (const void *)n_tracks,
                          (const void *)root_frame, (const void *)root_slot, (const void *)length})
        if (!p || misaligned(p, 4)) return SSLAM_E_INVALID;
    if (!workspace || misaligned(workspace, 8)) return SSLAM_E_INVALID;
    if (n_bank <= 0 || K <= 0) return SSLAM_E_INVALID;
    if (bank_shape(n_bank, K) != SSLAM_OK) return SSLAM_E_UNSUPPORTED;
    const int N = n_bank * K;
    const unsigned tiles = (unsigned)(((long long)N + TILE - 1) / TILE);
    int2 *rd[2] = {(int2 *)workspace, (int2 *)workspace + N};
    int *id_of_root = (int *)((int2 *)workspace + 2 * (size_t)N), *tile_sum = id_of_root + N;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ids_init_kernel, dim3(groups(N)), dim3(NT), 0, st, (const int *)prev, (const int *)prev_frame, K, N, rd[0],
                       (int *)root_frame, (int *)root_slot, (int *)length);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    int cur = 0;
    for (long long reach = 1; reach < n_bank; reach *= 2, cur ^= 1) {      // ceil(log2 n_bank) rounds: a chain has n_bank - 1 hops at most
        hipLaunchKernelGGL(ids_jump_kernel, dim3(groups(N)), dim3(NT), 0, st, (const int2 *)rd[cur], rd[cur ^ 1], N);
        if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    }
    hipLaunchKernelGGL(ids_count_kernel, dim3(tiles), dim3(NT), 0, st, (const int2 *)rd[cur], N, tile_sum);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(ids_scan_tiles_kernel, dim3(1), dim3(NT), 0, st, tile_sum, (int)tiles, (int *)n_tracks);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(ids_number_kernel, dim3(tiles), dim3(NT), 0, st, (const int2 *)rd[cur], (const int *)tile_sum, K, N, id_of_root,
                       (int *)root_frame, (int *)root_slot);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(ids_assign_kernel, dim3(groups(N)), dim3(NT), 0, st, (const int2 *)rd[cur], (const int *)id_of_root, N,
                       (int *)track_id, (int *)age, (int *)length);
    return launched();
}

extern "C" int sslt_landmarks(const float *kp_bank, const int32_t *kp_depth_bank, const double *C, int n_bank, int K, double fx, double fy,
                              double cx, double cy, double depth_scale, double scale_x, double scale_y, double view_w, double view_h,
                              double threshold, const int32_t *next, const int32_t *next_frame, const int32_t *root_frame,
                              const int32_t *root_slot, const int32_t *n_tracks, const float *weight, int min_obs, double *xyz,
                              int32_t *n_obs, int32_t *n_kept, int32_t *status, double *weight_sum, double *rms, double *residual,
                              int32_t *kept, void *stream) {
    for (const void *p : {(const void *)kp_bank, (const void *)kp_depth_bank, (const void *)next, (const void *)next_frame,
                          (const void *)root_frame, (const void *)root_slot, (const void *)n_tracks, (const void *)n_obs, (const void *)n_kept,
                          (const void *)status, (const void *)kept})
        if (!p || misaligned(p, 4)) return SSLAM_E_INVALID;
    for (const void *p : {(const void *)C, (const void *)xyz, (const void *)weight_sum, (const void *)rms, (const void *)residual})
        if (!p || misaligned(p, 8)) return SSLAM_E_INVALID;
    if (misaligned(weight, 4)) return SSLAM_E_INVALID;
    if (n_bank <= 0 || K <= 0 || min_obs < 2 || !(threshold - threshold == 0.0 && threshold >= 0.0)) return SSLAM_E_INVALID;
    if (!positive(fx) || !positive(fy) || !positive(depth_scale) || !positive(scale_x) || !positive(scale_y) || !positive(view_w) ||
        !positive(view_h) || !(cx - cx == 0.0) || !(cy - cy == 0.0))
        return SSLAM_E_INVALID;
    if (bank_shape(n_bank, K) != SSLAM_OK) return SSLAM_E_UNSUPPORTED;
    const int N = n_bank * K;
    const Camera cam = {fx, fy, cx, cy, depth_scale, scale_x, scale_y};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(landmark_fill_kernel, dim3(groups(N)), dim3(NT), 0, st, residual, (int *)kept, N);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(landmark_kernel, dim3(groups(N)), dim3(NT), 0, st, kp_bank, (const int *)kp_depth_bank, C, n_bank, K, N, cam, threshold,
                       (const int *)next, (const int *)next_frame, (const int *)root_frame, (const int *)root_slot, (const int *)n_tracks, weight,
                       min_obs, xyz, (int *)n_obs, (int *)n_kept, (int *)status, weight_sum, rms, residual, (int *)kept);
    return launched();
}

extern "C" int sslt_track_step(int32_t *t, int32_t *next_id, int32_t *prev, int32_t *next, int32_t *prev_frame, int32_t *next_frame,
                               int32_t *track_id, int32_t *age, const int64_t *matches, const int32_t *count, const int32_t *mask,
                               const int32_t *first, int n1, int K, int capacity, int32_t *out_track_id, int32_t *out_age, int32_t *n_new,
                               int32_t *status, void *stream) {
    for (const void *p : {(const void *)t, (const void *)next_id, (const void *)prev, (const void *)next, (const void *)prev_frame,
                          (const void *)next_frame, (const void *)track_id, (const void *)age, (const void *)count, (const void *)first,
                          (const void *)out_track_id, (const void *)out_age, (const void *)n_new, (const void *)status})
        if (!p || misaligned(p, 4)) return SSLAM_E_INVALID;
    if (!matches || misaligned(matches, 8) || misaligned(mask, 4)) return SSLAM_E_INVALID;
    if (n1 <= 0 || K <= 0 || capacity <= 0) return SSLAM_E_INVALID;
    if (K > SSLT_MAX_K || bank_shape(capacity, K) != SSLAM_OK) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(track_step_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (int *)t, (int *)next_id, (int *)prev, (int *)next,
                       (int *)prev_frame, (int *)next_frame, (int *)track_id, (int *)age, (const long long *)matches, (const int *)count,
                       (const int *)mask, (const int *)first, n1, K, capacity, (int *)out_track_id, (int *)out_age, (int *)n_new,
                       (int *)status);
    return launched();
}
