// pose_graph.hip - libsslam_graph.so: the pose graph over relative poses and their information matrices (include/sslam_graph.h
// states the arithmetic operation by operation; tests/pose_graph_ref.py restates it in numpy float64).
//   sslg_chain_poses   world -> camera poses from consecutive transforms, one thread per chain: the initial guess.
//   sslg_pose_graph    one 256-thread workgroup per graph: Gauss-Newton with a Huber weight per edge, node 0 the anchor.  The
//                      driver (the slot counts, the costs, the trial poses, the accept rule, the status words) is gauss_newton.h's,
//                      shared with csrc_loop/loop.hip; this file is the banded solve it calls, BandedSolver::step.
// A step of sslg_pose_graph:
//   assembly       256 edges at a time are STAGED, one thread per edge (the residual, w, and the 90 products w H, -(w H Ad),
//                  w Ad^T H Ad, w H r, -(w Ad^T H r)), then WALKED (edge_walk.h) in slot order by four groups of 63 threads: a thread owns one entry
//                  position (21 of a diagonal block's lower triangle, 36 of an off-diagonal block, 6 of g) of the nodes n with
//                  n % 4 == its group, so every word of A and g has one writer and takes its terms in ascending slot order.
//   factorisation  right-looking on a sliding window in LDS: the lower triangle of the trailing (bw + 1) x (bw + 1) block, 64 KB at
//                  band 20, 158 KB at band 32.  Column j: one thread per row divides by the pivot, a barrier, the 256 threads
//                  subtract (L_ij L_kj) D_j from the triangle behind it (about (bw / 16)^2 / 2 entries each), a barrier, row
//                  j + bw + 1 of A enters where column j was.  An element takes its updates in ascending k, as in the left-looking
//                  statement of the header, so the bits are those.  The forward substitution rides along (y_i takes L_ij y_j as y_j
//                  becomes final).  L leaves the window column by column, into the workspace where row j of A was.
//   backward       by rows, in one wave: the deltas and the row's column of L (contiguous) in registers, the products in parallel, then
//                  subtracted in ascending k by every lane; the next row's column is fetched meanwhile.
// The window's slots: entry (i, k) of the trailing block lies at the unordered pair (i mod M, k mod M), M = bw + 1, of a packed
// triangle - the M rows in flight have distinct residues, so the map is one to one, and the row that enters takes exactly the slots
// of the column that left.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sslam_graph.h"

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;

#include "gauss_newton.h"         // the driver: block_sum, block_count, Graph, edge_used, graph_cost, gauss_newton, graph_operands; edge_terms.h

#include "edge_walk.h"           // WALK, GROUPS, walk_staged: the assembly's walk, shared with csrc_window/window.hip; lane_value

constexpr int TQ = (6 * SSLG_MAX_BAND + 5 + 15) / 16;      // columns of the trailing block a thread of the 16 x 16 tiling takes: 13

long long g_launches = 0;   // diagnostic launch counter (sslg_launch_count): relaxed atomic adds, the library's only mutable state

// the banded solve: the normal equations of one graph in the workspace (A by rows of W words, then g, y, delta), the window and
// the ring in LDS
struct BandedSolver {
    const Graph &g;
    const double *C;
    double chi, damping;
    double *Ab, *gv, *yv, *dv, *stage, *win, *ring;
    int *sa, *sb;                                        // the staged edges' nodes; sb < 0: not used
    int n, bw, W, M;

    __device__ __forceinline__ void prepare() {}

    __device__ __forceinline__ int step(int, const double *&delta) {
        const int tid = threadIdx.x, n_edges = g.n_edges;
        // ---- assembly at the current poses
        for (long long k = tid; k < (long long)n * W + n; k += NT) Ab[k] = 0.0;      // A and g
        __syncthreads();
#pragma unroll 1
        for (int base = 0; base < n_edges; base += NT) {
            const int e = base + tid;
            int a = -1, b = -1;
            if (e < n_edges && edge_used(g, e, a, b)) {
                Edge ed;
                edge_eval(C + (long long)a * 12, C + (long long)b * 12, g.T + (long long)e * 12, g.info + (long long)e * 21, chi, ed);
                edge_stage(ed, stage + tid * STAGE);
            } else {
                b = -1;
            }
            sa[tid] = a;
            sb[tid] = b;
            __syncthreads();
            {
                double *const band = Ab;
                const int Wl = W, bwl = bw;
                walk_staged(sa, sb, stage, n_edges - base < NT ? n_edges - base : NT, tid,
                            [=](int r, int c) { return band + (long long)r * Wl + (c - r + bwl); }, gv);
            }
            __syncthreads();
        }
        for (int i = tid; i < n; i += NT) {
            double *p = Ab + (long long)i * W + bw;
            *p = *p + damping;
        }
        __syncthreads();

        // ---- the factorisation and the forward substitution, column by column on the window
        const int rows0 = n < M ? n : M;
        for (int i = tid >> 4; i < rows0; i += 16)
            for (int k = tid & 15; k <= i; k += 16) win[tri_lower(i, k)] = Ab[(long long)i * W + (k - i + bw)];
        for (int i = tid; i < rows0; i += NT) ring[i] = -gv[i];
        int fail = -1, jm = 0;                           // jm = j mod M
#pragma unroll 1
        for (int j = 0; j < n; j++) {
            __syncthreads();                             // the window holds rows j .. j + bw of the trailing block
            const double d = win[tri_lower(jm, jm)], yj = ring[jm];
            if (!(d > 0.0 && fin(d))) {                  // uniform
                fail = j;
                break;
            }
            const int m = n - 1 - j < bw ? n - 1 - j : bw, inew = j + bw + 1;
            double vnew = 0.0, gnew = 0.0;               // row inew of A, fetched now, stored when column j is dead
            if (inew < n && tid <= bw) vnew = Ab[(long long)inew * W + tid];
            if (inew < n && tid == 0) gnew = gv[inew];
            if (tid >= 1 && tid <= m) {
                int a = jm + tid;
                a = a >= M ? a - M : a;
                const int at = a >= jm ? tri_lower(a, jm) : tri_lower(jm, a);
                const double l = win[at] / d;
                win[at] = l;
                Ab[(long long)j * W + tid] = l;          // column j of L, where row j of A was
                ring[a] = ring[a] - l * yj;
            }
            if (tid == 0) {
                Ab[(long long)j * W] = d;
                yv[j] = yj;
            }
            __syncthreads();
            // thread (ty, tx) of 16 x 16 takes the entries (j + ri, j + rk), ri = 1 + ty + 16 p, rk = 1 + tx + 16 q <= ri; its L_kj
            // stay in registers for the column, and a row's reads are issued before its writes
            // (a slot's row base a (a + 1) / 2 is computed once per column or row: the entry's index is then an add and a select)
            const int tx = tid & 15, ty = tid >> 4, qn = (m + 15) >> 4, jmb = tri_lower(jm, 0);
            double lkq[TQ];
            int akq[TQ], kbq[TQ];
#pragma unroll
            for (int q = 0; q < TQ; q++) {
                if (q < qn) {                            // uniform
                    const int rk = 1 + tx + 16 * q;
                    int ak = jm + rk;
                    ak = ak >= M ? ak - M : ak;
                    akq[q] = ak;
                    kbq[q] = tri_lower(ak, 0);
                    lkq[q] = rk <= m ? win[ak >= jm ? kbq[q] + jm : jmb + ak] : 0.0;
                }
            }
            for (int p = 0, ri = 1 + ty; ri <= m; p++, ri += 16) {      // row ri takes the column groups q <= p, the last one up to tx <= ty
                int ai = jm + ri;
                ai = ai >= M ? ai - M : ai;
                const int ib = tri_lower(ai, 0);
                const double li = win[ai >= jm ? ib + jm : jmb + ai];
                double cur[TQ];
                int at[TQ];
#pragma unroll
                for (int q = 0; q < TQ; q++) {
                    if (q <= p && (q < p || tx <= ty)) {
                        at[q] = ai >= akq[q] ? ib + akq[q] : kbq[q] + ai;
                        cur[q] = win[at[q]];
                    }
                }
#pragma unroll
                for (int q = 0; q < TQ; q++)
                    if (q <= p && (q < p || tx <= ty)) win[at[q]] = cur[q] - (li * lkq[q]) * d;
            }
            __syncthreads();
            if (inew < n && tid <= bw) {                 // entry (inew, j + 1 + tid): inew's residue is jm
                int ak = jm + 1 + tid;
                ak = ak >= M ? ak - M : ak;
                win[ak >= jm ? tri_lower(ak, jm) : tri_lower(jm, ak)] = vnew;
                if (tid == 0) ring[jm] = -gnew;
            }
            jm = jm + 1 == M ? 0 : jm + 1;
        }
        if (fail >= 0) return fail;

        // ---- backward, by rows, in the first wave alone: lane t holds delta_{i+1+t+64q} and L_{i+1+t+64q, i} (q < 4: bw < 256) in
        // registers, the products are formed in parallel, every lane subtracts them in ascending k (a lane's product read by
        // v_readlane; a slot past the row's end holds +0.0, and x - (+0.0) is x), the deltas move up one lane, delta_i enters at
        // lane 0.  No barrier, no LDS; the next row's column of L is fetched while this one is summed.
        if (tid < 64) {
            double dl[4] = {0.0, 0.0, 0.0, 0.0}, lc[4] = {0.0, 0.0, 0.0, 0.0};
            double ycur = yv[n - 1], dcur = Ab[(long long)(n - 1) * W];
#pragma unroll 1
            for (int i = n - 1; i >= 0; i--) {
                const int cnt = n - 1 - i < bw ? n - 1 - i : bw;
                double pr[4], ln[4] = {0.0, 0.0, 0.0, 0.0}, ynext = 0.0, dnext = 1.0;
#pragma unroll
                for (int q = 0; q < 4; q++) pr[q] = tid + 64 * q < cnt ? lc[q] * dl[q] : 0.0;
                if (i > 0) {
                    const int cn = n - i < bw ? n - i : bw;
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (tid + 64 * q < cn) ln[q] = Ab[(long long)(i - 1) * W + 1 + tid + 64 * q];
                    ynext = yv[i - 1];
                    dnext = Ab[(long long)(i - 1) * W];
                }
                double v = ycur / dcur;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (64 * q < cnt) {                  // uniform
#pragma unroll
                        for (int t = 0; t < 64; t++) v = v - lane_value(pr[q], t);
                    }
                }
                if (tid == 0) dv[i] = v;
#pragma unroll
                for (int q = 3; q >= 0; q--) {
                    const double carry = q > 0 ? lane_value(dl[q - 1], 63) : v;
                    const double up = __shfl_up(dl[q], 1);
                    dl[q] = tid == 0 ? carry : up;
                    lc[q] = ln[q];
                }
                ycur = ynext;
                dcur = dnext;
            }
        }
        __syncthreads();
        delta = dv;
        return -1;
    }
};

__global__ __launch_bounds__(NT) void pose_graph_kernel(const int *__restrict__ edge_first, const int *__restrict__ edge_second,
                                                        const double *__restrict__ edge_T, const double *__restrict__ edge_info,
                                                        int n_nodes, int n_edges, const double *__restrict__ C_in, int band, double chi,
                                                        double damping, int n_iter, double *workspace, long long ws_words, double *C,
                                                        int *__restrict__ status, int *__restrict__ iterations,
                                                        int *__restrict__ used_edges, int *__restrict__ skipped_edges,
                                                        int *__restrict__ failed_row, double *__restrict__ cost_in,
                                                        double *__restrict__ cost_out, double *__restrict__ edge_chi2) {
    extern __shared__ double dyn[];                      // win: M (M + 1) / 2 words, then ring: M words (y, later delta)
    __shared__ double wsum[WAVES];
    __shared__ int wcnt[WAVES];
    __shared__ int sa[NT], sb[NT];

    const long long gi = blockIdx.x;
    const Graph g = graph_of(edge_first, edge_second, edge_T, edge_info, n_nodes, n_edges, band, gi);
    C += gi * n_nodes * 12;

    const int n = 6 * (n_nodes - 1), bw = 6 * band + 5, W = bw + 1, M = W;
    double *Ab = workspace + gi * ws_words;
    double *gv = Ab + (long long)n * W, *yv = gv + n, *dv = yv + n;
    double *trial = dv + n;
    BandedSolver solver{g, C, chi, damping, Ab, gv, yv, dv, trial + (long long)n_nodes * 12, dyn, dyn + (M * (M + 1)) / 2, sa, sb, n, bw, W, M};
    gauss_newton(solver, g, C_in + gi * n_nodes * 12, C, trial, chi, n_iter, wsum, wcnt,
                 GraphOut{status, iterations, used_edges, skipped_edges, failed_row, cost_in, cost_out, edge_chi2 + gi * n_edges}, gi);
}

__global__ __launch_bounds__(NT) void chain_kernel(const double *__restrict__ T, const double *__restrict__ C_start, int n_graphs,
                                                   int n_nodes, double *__restrict__ C) {
    const long long gi = (long long)blockIdx.x * NT + threadIdx.x;
    if (gi >= n_graphs) return;
    double cur[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (C_start) {
#pragma unroll
        for (int k = 0; k < 12; k++) cur[k] = C_start[gi * 12 + k];
    }
    double *out = C + gi * n_nodes * 12;
    const double *t = T + gi * (n_nodes - 1) * 12;
#pragma unroll
    for (int k = 0; k < 12; k++) out[k] = cur[k];
#pragma unroll 1
    for (int i = 0; i + 1 < n_nodes; i++) {
        double ti[12], nxt[12];
#pragma unroll
        for (int k = 0; k < 12; k++) ti[k] = t[(long long)i * 12 + k];
        compose(ti, cur, nxt);
#pragma unroll
        for (int k = 0; k < 12; k++) out[(long long)(i + 1) * 12 + k] = cur[k] = nxt[k];
    }
}

inline long long workspace_words(int n_nodes, int band) {      // per graph
    const long long n = 6LL * (n_nodes - 1), W = 6LL * band + 6;
    return n * W + 3 * n + 12LL * n_nodes + (long long)NT * STAGE;
}

inline int graph_shape(int n_graphs, int n_nodes, int band) {
    if (n_graphs <= 0 || n_nodes <= 0 || band <= 0) return SSLAM_E_INVALID;
    if (band > SSLG_MAX_BAND || n_nodes > SSLG_MAX_NODES || n_graphs > SSLG_MAX_GRAPHS) return SSLAM_E_UNSUPPORTED;
    return SSLAM_OK;
}

}  // namespace

extern "C" int sslg_version(void) { return 100; }
extern "C" const char *sslg_arch(void) { return "gfx950"; }
extern "C" long long sslg_launch_count(void) { return __atomic_load_n(&g_launches, __ATOMIC_RELAXED); }

extern "C" int sslg_chain_poses(const double *T, const double *C_start, int n_graphs, int n_nodes, double *C, void *stream) {
    if (!C || n_graphs <= 0 || n_nodes <= 0 || (!T && n_nodes > 1) || C == C_start) return SSLAM_E_INVALID;
    if (misaligned(T, 8) || misaligned(C_start, 8) || misaligned(C, 8)) return SSLAM_E_INVALID;
    if (n_graphs > 0x7fffffff / NT || n_nodes > SSLG_MAX_NODES) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(chain_kernel, dim3((unsigned)((n_graphs + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, T, C_start, n_graphs,
                       n_nodes, C);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}

extern "C" size_t sslg_pose_graph_workspace_bytes(int n_graphs, int n_nodes, int band) {
    if (graph_shape(n_graphs, n_nodes, band) != SSLAM_OK) return 0;
    return (size_t)n_graphs * (size_t)workspace_words(n_nodes, band) * sizeof(double);
}

extern "C" int sslg_pose_graph(const int32_t *edge_first, const int32_t *edge_second, const double *edge_T, const double *edge_info,
                               int n_graphs, int n_nodes, int n_edges, const double *C_in, int band, double huber_chi, double damping,
                               int n_iter, void *workspace, double *C, int32_t *status, int32_t *iterations, int32_t *used_edges,
                               int32_t *skipped_edges, int32_t *failed_row, double *cost_in, double *cost, double *edge_chi2,
                               void *stream) {
    if (graph_operands(edge_first, edge_second, edge_T, edge_info, C_in, huber_chi, damping, n_iter, SSLG_GRAPH_MAX_ITER, workspace, C,
                       status, iterations, used_edges, skipped_edges, failed_row, cost_in, cost, edge_chi2) != SSLAM_OK)
        return SSLAM_E_INVALID;
    if (n_edges <= 0 || graph_shape(n_graphs, n_nodes, band) == SSLAM_E_INVALID) return SSLAM_E_INVALID;
    if (graph_shape(n_graphs, n_nodes, band) != SSLAM_OK || n_edges > SSLG_MAX_EDGES) return SSLAM_E_UNSUPPORTED;
    const int M = 6 * band + 6;
    const size_t lds = ((size_t)M * (M + 1) / 2 + M) * sizeof(double);      // the window and the ring: 159 192 bytes at band 32
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(pose_graph_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return SSLAM_E_LAUNCH;
    hipLaunchKernelGGL(pose_graph_kernel, dim3((unsigned)n_graphs), dim3(NT), lds, (hipStream_t)stream, (const int *)edge_first,
                       (const int *)edge_second, edge_T, edge_info, n_nodes, n_edges, C_in, band, huber_chi, damping, n_iter,
                       (double *)workspace, workspace_words(n_nodes, band), C, (int *)status, (int *)iterations, (int *)used_edges,
                       (int *)skipped_edges, (int *)failed_row, cost_in, cost, edge_chi2);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}
