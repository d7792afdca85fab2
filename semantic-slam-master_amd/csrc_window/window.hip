// window.hip - libsslam_window.so: the online sliding-window estimator (include/sslam_window.h states the step; tests/window_ref.py
// restates it in numpy float64 on top of tests/pose_graph_ref.py).
//   sslw_window_step   one 256-thread workgroup per window: the frame's S refined pairs are admitted into the ring, the new pose is
//                      predicted from the nearest admitted one, and the window's poses are optimised by csrc_graph/gauss_newton.h's
//                      driver - the one sslg_pose_graph and ssll_pose_graph_sparse run - on this file's solve, DenseSolver::step.
// A step of the solve, n = 6 (n_nodes - 1) <= 186 rows:
//   assembly       pose_graph.hip's, the walk being csrc_graph/edge_walk.h's, shared: the (at most 256) slots are STAGED once, one thread per slot, into the workspace, then WALKED in
//                  slot order by four groups of 63 threads, a thread owning one entry position of the nodes n with n % 4 == its group,
//                  so every word of A and g has one writer and takes its terms in ascending slot order.  A and g are LDS.
//   factorisation  right-looking, in place on the whole lower triangle in LDS (row i at i (i + 1) / 2): column j is divided by the
//                  pivot by one thread per row, a barrier, the 256 threads as 16 x 16 subtract (L_ij L_kj) D_j from the triangle
//                  behind it, a barrier.  An element takes its updates in ascending k, as in the left-looking statement of
//                  sslam_graph.h at band >= n / 6, so the bits are those.  The forward substitution rides along.
//   backward       by rows, in one wave, as pose_graph.hip's: lane t holds delta_{i+1+t+64q} in registers, the products with row
//                  i's column of L (from LDS) are formed in parallel and subtracted in ascending k by every lane.
// No column of the factor goes through global memory, which is what BandedSolver pays per column.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sslam_window.h"

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;

#include "../csrc_graph/gauss_newton.h"      // the driver and, through it, edge_terms.h

#include "../csrc_graph/edge_walk.h"        // WALK, GROUPS, walk_staged: pose_graph.hip's walk; lane_value

constexpr int ROWS_MAX = 6 * (SSLW_MAX_WINDOW - 1);
constexpr int QB = (ROWS_MAX + 63) / 64;      // 64-lane groups of a row of the backward substitution: 3
static_assert(SSLW_MAX_WINDOW * SSLW_MAX_SPACINGS <= NT, "the slots are staged in one pass, one thread per slot");
static_assert(ROWS_MAX <= NT, "one thread per row divides a column by its pivot");

long long g_launches = 0;   // diagnostic launch counter (sslw_launch_count): relaxed atomic adds, the library's only mutable state

// the dense solve: A (the lower triangle by rows), g, y and delta in LDS, the staged terms in the workspace
struct DenseSolver {
    const Graph &g;
    const double *C;
    double chi, damping;
    double *stage, *A;
    int *sa, *sb;                                        // the staged slots' nodes; sb < 0: not used
    int n;

    __device__ __forceinline__ void prepare() {}

    __device__ __forceinline__ int step(int, const double *&delta) {
        const int tid = threadIdx.x, n_edges = g.n_edges, ntri = (n * (n + 1)) / 2;
        double *gv = A + ntri, *yv = gv + n, *dv = yv + n;
        // ---- assembly at the current poses
        for (int k = tid; k < ntri + n; k += NT) A[k] = 0.0;      // A and g
        {
            int a = -1, b = -1;
            if (tid < n_edges && edge_used(g, tid, a, b)) {
                Edge ed;
                edge_eval(C + a * 12, C + b * 12, g.T + tid * 12, g.info + tid * 21, chi, ed);
                edge_stage(ed, stage + tid * STAGE);
            } else {
                b = -1;
            }
            sa[tid] = a;
            sb[tid] = b;
        }
        __syncthreads();
        {
            double *const tri = A;
            walk_staged(sa, sb, stage, n_edges, tid, [=](int r, int c) { return tri + tri_lower(r, c); }, gv);
        }
        __syncthreads();
        for (int i = tid; i < n; i += NT) {
            double *p = A + tri_lower(i, i);
            *p = *p + damping;
            yv[i] = -gv[i];
        }

        // ---- the factorisation and the forward substitution, column by column
        const int tx = tid & 15, ty = tid >> 4;
        int fail = -1;
#pragma unroll 1
        for (int j = 0; j < n; j++) {
            __syncthreads();                             // the trailing block holds the updates of the columns before j
            const double d = A[tri_lower(j, j)], yj = yv[j];
            if (!(d > 0.0 && fin(d))) {                  // uniform
                fail = j;
                break;
            }
            const int m = n - 1 - j;
            if (tid >= 1 && tid <= m) {
                const int at = tri_lower(j + tid, j);
                const double l = A[at] / d;
                A[at] = l;
                yv[j + tid] = yv[j + tid] - l * yj;
            }
            __syncthreads();
            for (int ri = 1 + ty; ri <= m; ri += 16) {   // entry (j + ri, j + rk), rk <= ri
                const int rowb = tri_lower(j + ri, 0) + j;
                const double li = A[rowb];
                for (int rk = 1 + tx; rk <= ri; rk += 16) A[rowb + rk] = A[rowb + rk] - (li * A[tri_lower(j + rk, j)]) * d;
            }
        }
        if (fail >= 0) return fail;
        __syncthreads();

        // ---- backward, by rows, in the first wave alone: lane t holds delta_{i+1+t+64q} in registers, the products are formed in
        // parallel, every lane subtracts them in ascending k (a slot past the row's end holds +0.0, and x - (+0.0) is x), the deltas
        // move up one lane, delta_i enters at lane 0.  No barrier inside.
        if (tid < 64) {
            double dl[QB];
#pragma unroll
            for (int q = 0; q < QB; q++) dl[q] = 0.0;
#pragma unroll 1
            for (int i = n - 1; i >= 0; i--) {
                const int cnt = n - 1 - i;
                double pr[QB];
#pragma unroll
                for (int q = 0; q < QB; q++) pr[q] = tid + 64 * q < cnt ? A[tri_lower(i + 1 + tid + 64 * q, i)] * dl[q] : 0.0;
                double v = yv[i] / A[tri_lower(i, i)];
#pragma unroll
                for (int q = 0; q < QB; q++) {
                    if (64 * q < cnt) {                  // uniform
#pragma unroll
                        for (int t = 0; t < 64; t++) v = v - lane_value(pr[q], t);
                    }
                }
                if (tid == 0) dv[i] = v;
#pragma unroll
                for (int q = QB - 1; q >= 0; q--) {
                    const double carry = q > 0 ? lane_value(dl[q > 0 ? q - 1 : 0], 63) : v;
                    const double up = __shfl_up(dl[q], 1);
                    dl[q] = tid == 0 ? carry : up;
                }
            }
        }
        __syncthreads();
        delta = dv;
        return -1;
    }
};

struct WindowArgs {
    int *t, *ring_first, *ring_second;
    double *ring_T, *ring_info, *ring_C, *trajectory;
    const int *spacings;
    const double *new_T, *new_info;
    const int *new_status, *new_inliers;
    const double *C_start;
    int W, S, min_inliers, n_iter;
    double chi, damping;
    long long capacity, ws_words;
    double *workspace, *C_window;
    int *base, *n_nodes, *admitted, *predicted_from, *lost, *status, *iterations, *used_edges, *dropped_edges, *failed_row;
    double *cost_in, *cost, *edge_chi2;
};

__global__ __launch_bounds__(NT) void window_kernel(const WindowArgs p) {
    extern __shared__ double dyn[];                      // A, g, y, delta of the solve
    __shared__ double wsum[WAVES];
    __shared__ int wcnt[WAVES];
    __shared__ int sa[NT], sb[NT];
    __shared__ int adm[SSLW_MAX_SPACINGS];

    const long long wi = blockIdx.x;
    const int tid = threadIdx.x, W = p.W, S = p.S, WS = W * S;
    const int t = p.t[wi];
    if (t < 0 || t > SSLW_MAX_FRAME) {                   // uniform
        if (tid == 0) p.status[wi] = 4;
        return;
    }
    const int base = t - W + 1 > 0 ? t - W + 1 : 0, nn = t - base + 1, row = t % W;
    int *rf = p.ring_first + wi * WS, *rs = p.ring_second + wi * WS;
    double *rT = p.ring_T + wi * WS * 12, *rI = p.ring_info + wi * WS * 21, *rC = p.ring_C + wi * W * 12;

    // ---- admission: thread k judges pair k and writes its ring slot
    if (tid < S) {
        const long long a = (long long)t - p.spacings[tid];
        const double *nt = p.new_T + (wi * S + tid) * 12, *ni = p.new_info + (wi * S + tid) * 21;
        bool ok = a >= base && a < t && p.new_status[wi * S + tid] != 3 && p.new_inliers[wi * S + tid] >= p.min_inliers;
        for (int k = 0; k < 12; k++) ok = ok && fin(nt[k]);
        for (int k = 0; k < 21; k++) ok = ok && fin(ni[k]);
        adm[tid] = ok;
        p.admitted[wi * S + tid] = ok;
        const int slot = row * S + tid;
        rf[slot] = ok ? (int)a : -1;
        rs[slot] = t;
        for (int k = 0; k < 12; k++) rT[slot * 12 + k] = ok ? nt[k] : 0.0;
        for (int k = 0; k < 21; k++) rI[slot * 21 + k] = ok ? ni[k] : 0.0;
    }
    __syncthreads();

    // ---- prediction: frame t's pose into its row of ring_C
    if (tid == 0) {
        double cur[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        int ks = -1, sp = 0;
        if (t == 0) {
            if (p.C_start) {
#pragma unroll
                for (int k = 0; k < 12; k++) cur[k] = p.C_start[wi * 12 + k];
            }
        } else {
            for (int k = 0; k < S; k++) {
                const int s = p.spacings[k];
                if (adm[k] && (ks < 0 || s < sp)) {
                    ks = k;
                    sp = s;
                }
            }
            const double *src = rC + ((t - (ks >= 0 ? sp : 1)) % W) * 12;
            double from[12], tm[12];
#pragma unroll
            for (int k = 0; k < 12; k++) from[k] = src[k];
            if (ks >= 0) {
#pragma unroll
                for (int k = 0; k < 12; k++) tm[k] = p.new_T[(wi * S + ks) * 12 + k];
                compose(tm, from, cur);
            } else {
#pragma unroll
                for (int k = 0; k < 12; k++) cur[k] = from[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 12; k++) rC[row * 12 + k] = cur[k];
        p.predicted_from[wi] = ks;
        p.lost[wi] = t > 0 && ks < 0;
        p.base[wi] = base;
        p.n_nodes[wi] = nn;
    }
    __syncthreads();

    // ---- the window as one graph: the slots' local nodes and C_in
    double *Cin = p.workspace + wi * p.ws_words, *trial = Cin + 12 * W, *stage = trial + 12 * W;
    int *lf = reinterpret_cast<int *>(stage + NT * STAGE), *ls = lf + WS;
    for (int e = tid; e < WS; e += NT) {
        const int f = rf[e];
        lf[e] = f == -1 ? -1 : (f < base ? -2 : f - base);
        ls[e] = (int)((unsigned)rs[e] - (unsigned)base);
    }
    for (int k = tid; k < nn * 12; k += NT) {
        const int i = k / 12;
        Cin[k] = rC[((base + i) % W) * 12 + (k - 12 * i)];
    }
    __syncthreads();

    Graph g;
    g.first = lf;
    g.second = ls;
    g.T = rT;
    g.info = rI;
    g.n_nodes = nn;
    g.n_edges = WS;
    g.band = W - 1;
    double *Cw = p.C_window + wi * W * 12;
    DenseSolver solver{g, Cw, p.chi, p.damping, stage, dyn, sa, sb, 6 * (nn - 1)};
    gauss_newton(solver, g, Cin, Cw, trial, p.chi, p.n_iter, wsum, wcnt,
                 GraphOut{p.status, p.iterations, p.used_edges, p.dropped_edges, p.failed_row, p.cost_in, p.cost, p.edge_chi2 + wi * WS}, wi);
    __syncthreads();

    // ---- write-back
    double *traj = p.trajectory + wi * p.capacity * 12;
    for (int k = tid; k < W * 12; k += NT) {
        const int i = k / 12, c = k - 12 * i;
        if (i < nn) {
            const double v = Cw[k];
            const long long j = (long long)base + i;
            rC[(j % W) * 12 + c] = v;
            if (j < p.capacity) traj[j * 12 + c] = v;
        } else {
            Cw[k] = 0.0;
        }
    }
    if (tid == 0) p.t[wi] = t + 1;
}

inline long long workspace_words(int window, int n_spacings) {      // per window
    return 24LL * window + (long long)NT * STAGE + (long long)window * n_spacings;
}

inline int window_shape(int n_windows, int window, int n_spacings) {
    if (n_windows <= 0 || window < 2 || n_spacings <= 0) return SSLAM_E_INVALID;
    if (window > SSLW_MAX_WINDOW || n_spacings > SSLW_MAX_SPACINGS || n_windows > SSLW_MAX_WINDOWS) return SSLAM_E_UNSUPPORTED;
    return SSLAM_OK;
}

}  // namespace

extern "C" int sslw_version(void) { return 100; }
extern "C" const char *sslw_arch(void) { return "gfx950"; }
extern "C" long long sslw_launch_count(void) { return __atomic_load_n(&g_launches, __ATOMIC_RELAXED); }

extern "C" size_t sslw_window_workspace_bytes(int n_windows, int window, int n_spacings) {
    if (window_shape(n_windows, window, n_spacings) != SSLAM_OK) return 0;
    return (size_t)n_windows * (size_t)workspace_words(window, n_spacings) * sizeof(double);
}

extern "C" int sslw_window_step(int32_t *t, int32_t *ring_first, int32_t *ring_second, double *ring_T, double *ring_info, double *ring_C,
                                double *trajectory, const int32_t *spacings, const double *new_T, const double *new_info,
                                const int32_t *new_status, const int32_t *new_inliers, const double *C_start, int n_windows, int window,
                                int n_spacings, int min_inliers, double huber_chi, double damping, int n_iter, long long capacity,
                                void *workspace, double *C_window, int32_t *base, int32_t *n_nodes, int32_t *admitted,
                                int32_t *predicted_from, int32_t *lost, int32_t *status, int32_t *iterations, int32_t *used_edges,
                                int32_t *dropped_edges, int32_t *failed_row, double *cost_in, double *cost, double *edge_chi2, void *stream) {
    for (const void *p : {(const void *)ring_T, (const void *)ring_info, (const void *)ring_C, (const void *)trajectory, (const void *)new_T,
                          (const void *)new_info, (const void *)workspace, (const void *)C_window, (const void *)cost_in, (const void *)cost,
                          (const void *)edge_chi2})
        if (!p || misaligned(p, 8)) return SSLAM_E_INVALID;
    for (const void *p : {(const void *)t, (const void *)ring_first, (const void *)ring_second, (const void *)spacings, (const void *)new_status,
                          (const void *)new_inliers, (const void *)base, (const void *)n_nodes, (const void *)admitted,
                          (const void *)predicted_from, (const void *)lost, (const void *)status, (const void *)iterations,
                          (const void *)used_edges, (const void *)dropped_edges, (const void *)failed_row})
        if (!p || misaligned(p, 4)) return SSLAM_E_INVALID;
    if (misaligned(C_start, 8)) return SSLAM_E_INVALID;
    if (!finite_positive(huber_chi) || !finite_nonnegative(damping) || n_iter < 0 || n_iter > SSLG_GRAPH_MAX_ITER || min_inliers < 0 ||
        capacity <= 0 || window_shape(n_windows, window, n_spacings) == SSLAM_E_INVALID)
        return SSLAM_E_INVALID;
    if (window_shape(n_windows, window, n_spacings) != SSLAM_OK || capacity > 0x7fffffffffffffffLL / 96 / n_windows) return SSLAM_E_UNSUPPORTED;
    const int n = 6 * (window - 1);
    const size_t lds = ((size_t)n * (n + 1) / 2 + 3 * (size_t)n) * sizeof(double);      // 143 592 bytes at window 32
    // past 60 KB the kernel's allowance is raised, always to the largest window's size: the value never depends on the caller, so
    // host threads that step windows of different sizes set the same thing (not a stream operation: legal inside a capture)
    constexpr int LDS_MAX = (ROWS_MAX * (ROWS_MAX + 1) / 2 + 3 * ROWS_MAX) * (int)sizeof(double);
    if (lds > 60 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(window_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX) != hipSuccess)
        return SSLAM_E_LAUNCH;
    WindowArgs a;
    a.t = (int *)t, a.ring_first = (int *)ring_first, a.ring_second = (int *)ring_second;
    a.ring_T = ring_T, a.ring_info = ring_info, a.ring_C = ring_C, a.trajectory = trajectory;
    a.spacings = (const int *)spacings, a.new_T = new_T, a.new_info = new_info;
    a.new_status = (const int *)new_status, a.new_inliers = (const int *)new_inliers, a.C_start = C_start;
    a.W = window, a.S = n_spacings, a.min_inliers = min_inliers, a.n_iter = n_iter;
    a.chi = huber_chi, a.damping = damping, a.capacity = capacity, a.ws_words = workspace_words(window, n_spacings);
    a.workspace = (double *)workspace, a.C_window = C_window;
    a.base = (int *)base, a.n_nodes = (int *)n_nodes, a.admitted = (int *)admitted, a.predicted_from = (int *)predicted_from;
    a.lost = (int *)lost, a.status = (int *)status, a.iterations = (int *)iterations, a.used_edges = (int *)used_edges;
    a.dropped_edges = (int *)dropped_edges, a.failed_row = (int *)failed_row;
    a.cost_in = cost_in, a.cost = cost, a.edge_chi2 = edge_chi2;
    hipLaunchKernelGGL(window_kernel, dim3((unsigned)n_windows), dim3(NT), lds, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}
