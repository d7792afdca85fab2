// loop.hip - libsslam_loop.so: loop closures (include/sslam_loop.h states the arithmetic operation by operation; tests/loop_ref.py
// restates it in numpy).
//   ssll_frame_signatures    two kernels: the score-weighted column sums of every frame (one workgroup per frame, thread c one
//                            column, one fmaf chain over the keypoints), then the sequence's mean, the centring and the norm (one
//                            workgroup per 32 frames; each forms the mean anew, in frame order, so no workgroup waits for another).
//   ssll_loop_candidates     one 256-thread workgroup per frame i: S_ij of the older frames into LDS, thread t the frames t, t + 256,
//                            ..., each one fmaf chain; then per_frame block-wide arg-max picks with suppression around each.
//   ssll_pose_graph_sparse   one 256-thread workgroup per graph: sslg_pose_graph's Gauss-Newton driver itself
//                            (csrc_graph/gauss_newton.h), the step (SparseSolver::step) by block-Jacobi preconditioned
//                            conjugate gradients.  Per launch (SparseSolver::prepare) the incidence lists (node -> its used slots, ascending);
//                            per step every used slot's 90 words are STAGED (csrc_graph/edge_terms.h: the same code as the banded
//                            kernel), a thread per (node, entry) adds a node's terms in list order, a thread per node factorises
//                            its block; a CG iteration is a thread per row for q = A p and the products, a thread per node for
//                            x, r, z = M^-1 r, a thread per row for p.  Every reduction is block_sum's fixed tree.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sslam_loop.h"

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;
constexpr int NODE_WORDS = 27;      // entry positions of a node: 21 of D_m's lower triangle, 6 of g_m
constexpr int NO_ROW = 0x7fffffff;

#include "../csrc_graph/gauss_newton.h"         // the driver and, through it, edge_terms.h: the same code as the banded kernel

long long g_launches = 0;   // diagnostic launch counter (ssll_launch_count): relaxed atomic adds, the library's only mutable state

inline bool width_ok(int d) { return d == 128 || d == 256; }

// ------------------------------------------------------------------------------------------------------------ signatures
__global__ __launch_bounds__(NT) void raw_kernel(const float *__restrict__ desc, const float *__restrict__ scores, int k, int d,
                                                 float *__restrict__ raw) {
    const long long f = blockIdx.x;
    const int c = threadIdx.x;
    const float *dp = desc + f * k * d + c, *sp = scores + f * k;
    float acc = 0.0f;
    for (int kk = 0; kk < k; kk++) acc = fmaf(sp[kk], dp[(long long)kk * d], acc);
    raw[f * d + c] = acc;
}

__global__ __launch_bounds__(NT) void sig_kernel(const float *__restrict__ raw, int n, int d, float *__restrict__ sig) {
    __shared__ float wsum[WAVES];
    const int c = threadIdx.x;
    float mean = 0.0f;
    for (int i = 0; i < n; i++) mean = mean + raw[i * d + c];
    mean = mean / (float)n;
    const int f0 = blockIdx.x * SSLL_FRAMES_PER_GROUP, f1 = f0 + SSLL_FRAMES_PER_GROUP < n ? f0 + SSLL_FRAMES_PER_GROUP : n;
    for (int f = f0; f < f1; f++) {
        const float cv = raw[f * d + c] - mean;
        float p = cv * cv;
        for (int o = 32; o >= 1; o >>= 1) p = p + __shfl_xor(p, o);
        if ((c & 63) == 0) wsum[c >> 6] = p;
        __syncthreads();
        float ss = wsum[0] + wsum[1];
        if (d == 256) ss = (ss + wsum[2]) + wsum[3];
        __syncthreads();                                     // wsum is written again
        sig[f * d + c] = cv / fmaxf(sqrtf(ss), 1e-12f);
    }
}

// ------------------------------------------------------------------------------------------------------------ candidates
// is (ov, oj) ahead of (bv, bj)?  value descending, then frame ascending; a negative frame is no candidate
__device__ __forceinline__ bool ahead(float ov, int oj, float bv, int bj) { return oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj)); }

__global__ __launch_bounds__(NT) void candidates_kernel(const float *__restrict__ sig, int n, int d, int min_gap, float min_sim,
                                                        int per_frame, int suppress, int *__restrict__ first,
                                                        int *__restrict__ second, float *__restrict__ sim, int *__restrict__ count) {
    __shared__ float S[SSLL_MAX_FRAMES];                   // S_ij, -inf where j is not (or no longer) eligible
    __shared__ float si[NT];
    __shared__ float wv[WAVES];
    __shared__ int wj[WAVES];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int m = i - min_gap + 1;                         // the frames 0 .. m - 1 are old enough (none if m <= 0)
    const float none = -__builtin_huge_valf();
    if (tid < d) si[tid] = sig[i * d + tid];
    __syncthreads();
    for (int j = tid; j < m; j += NT) {
        const float4 *row = reinterpret_cast<const float4 *>(sig + j * d);
        float acc = 0.0f;
        for (int q = 0; q < d / 4; q++) {
            const float4 v = row[q];
            acc = fmaf(si[4 * q], v.x, acc);
            acc = fmaf(si[4 * q + 1], v.y, acc);
            acc = fmaf(si[4 * q + 2], v.z, acc);
            acc = fmaf(si[4 * q + 3], v.w, acc);
        }
        S[j] = acc >= min_sim ? acc : none;
    }
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
        if (tid == 0) {
            first[i * per_frame + s] = bj;
            second[i * per_frame + s] = i;
            sim[i * per_frame + s] = bv;
        }
        cnt++;
        const int reach = suppress < n ? suppress : n;
        const int lo = bj - reach > 0 ? bj - reach : 0, hi = bj + reach < m - 1 ? bj + reach : m - 1;
        for (int j = lo + tid; j <= hi; j += NT) S[j] = none;
        __syncthreads();
    }
    if (tid == 0) {
        for (int s = cnt; s < per_frame; s++) {
            first[i * per_frame + s] = -1;
            second[i * per_frame + s] = -1;
            sim[i * per_frame + s] = 0.0f;
        }
        count[i] = cnt;
    }
}

// ------------------------------------------------------------------------------------------------------------ the sparse graph
__device__ __forceinline__ int block_min(int n, int *wcnt, int tid) {
    for (int o = 32; o >= 1; o >>= 1) {
        const int v = __shfl_xor(n, o);
        n = v < n ? v : n;
    }
    if ((tid & 63) == 0) wcnt[tid >> 6] = n;
    __syncthreads();
    for (int w = 0; w < WAVES; w++) n = wcnt[w] < n ? wcnt[w] : n;
    __syncthreads();
    return n;
}

// u . v over the n rows, in the cost's order
__device__ __forceinline__ double dot(const double *u, const double *v, int n, double *wsum, int tid) {
    double part = 0.0;
    for (int i = tid; i < n; i += NT) part = part + u[i] * v[i];
    return block_sum(part, wsum, tid);
}

// z = M^-1 v for one node: f holds L below the diagonal and the pivots on it (tri_lower)
__device__ __forceinline__ void block_solve(const double *f, const double (&v)[6], double (&z)[6]) {
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        y[i] = v[i];
#pragma unroll
        for (int k = 0; k < i; k++) y[i] = y[i] - f[tri_lower(i, k)] * y[k];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        z[i] = y[i] / f[tri_lower(i, i)];
#pragma unroll
        for (int k = i + 1; k < 6; k++) z[i] = z[i] - f[tri_lower(k, i)] * z[k];
    }
}

inline long long workspace_words(int n_nodes, int n_edges) {      // per graph
    const long long N = n_nodes, nn = N - 1, E = n_edges;
    return 90 * E + 78 * nn + 12 * N + (N + 1 + 2 * E + 1) / 2;
}

// the sparse solve: one graph's staged terms, blocks, CG vectors and incidence lists in the workspace, the list cursors in LDS
struct SparseSolver {
    const Graph &g;
    const double *C;
    double chi, damping, tol2;
    int cg_iterations;
    double *stage, *Dl, *Lf, *gv, *xv, *rv, *zv, *pv, *qv;
    int *off, *list;
    double *wsum;
    int *wcnt, *sa, *sb, *cur, *seg, *steps_of;          // sa, sb: a chunk's nodes while the lists are filled; -1: not used

    __device__ __forceinline__ void prepare() {
        const int tid = threadIdx.x, n_nodes = g.n_nodes, n_edges = g.n_edges;
        // ---- the incidence lists: counts, an exclusive scan, then the slots a chunk at a time, in slot order
        for (int m = tid; m <= n_nodes; m += NT) cur[m] = 0;
        __syncthreads();
        for (int e = tid; e < n_edges; e += NT) {
            int a, b;
            if (edge_used(g, e, a, b)) {
                atomicAdd(&cur[b], 1);
                if (a >= 1) atomicAdd(&cur[a], 1);
            }
        }
        __syncthreads();
        {
            const int per = (n_nodes + NT - 1) / NT, m0 = tid * per, m1 = m0 + per < n_nodes ? m0 + per : n_nodes;
            int sum = 0;
            for (int m = m0; m < m1; m++) sum += cur[m];
            seg[tid] = sum;
            __syncthreads();
            int run = 0;
            for (int t = 0; t < tid; t++) run += seg[t];
            for (int m = m0; m < m1; m++) {
                const int c = cur[m];
                off[m] = run;
                cur[m] = run;
                run += c;
            }
            if (tid == NT - 1) off[n_nodes] = run;           // the last thread's segment ends the nodes (or is empty, after them)
        }
        __syncthreads();
#pragma unroll 1
        for (int base = 0; base < n_edges; base += NT) {
            const int e = base + tid;
            int a = -1, b = -1;
            const bool u = e < n_edges && edge_used(g, e, a, b);
            sa[tid] = u ? a : -1;
            sb[tid] = u ? b : -1;
            __syncthreads();
            int rank_a = 0, tot_a = 0, rank_b = 0, tot_b = 0;
            if (u) {
                const int cnt = n_edges - base < NT ? n_edges - base : NT;
                for (int c = 0; c < cnt; c++) {
                    const int ca = sa[c], cb = sb[c];
                    const int ha = (ca == a) + (cb == a), hb = (ca == b) + (cb == b);
                    tot_a += ha;
                    tot_b += hb;
                    rank_a += c < tid ? ha : 0;
                    rank_b += c < tid ? hb : 0;
                }
                list[cur[b] + rank_b] = 2 * e;
                if (a >= 1) list[cur[a] + rank_a] = 2 * e + 1;
            }
            __syncthreads();
            if (u) {                                             // the last of a node's entries in the chunk moves its cursor
                if (rank_b + 1 == tot_b) cur[b] += tot_b;
                if (a >= 1 && rank_a + 1 == tot_a) cur[a] += tot_a;
            }
            __syncthreads();
        }
    }

    __device__ __forceinline__ int step(int it, const double *&delta) {
        const int tid = threadIdx.x, n_edges = g.n_edges, nn = g.n_nodes - 1, n = 6 * nn;
        // ---- every used slot's terms at the current poses
#pragma unroll 1
        for (int e = tid; e < n_edges; e += NT) {
            int a, b;
            if (edge_used(g, e, a, b)) {
                Edge ed;
                edge_eval(C + (long long)a * 12, C + (long long)b * 12, g.T + (long long)e * 12, g.info + (long long)e * 21, chi, ed);
                edge_stage(ed, stage + (long long)e * STAGE);
            }
        }
        __syncthreads();
        // ---- D_m and g_m: a thread per (node, entry), the node's list in order
        for (int idx = tid; idx < nn * NODE_WORDS; idx += NT) {
            const int mi = idx / NODE_WORDS, pos = idx - mi * NODE_WORDS;
            double acc = 0.0;
            for (int q = off[mi + 1]; q < off[mi + 2]; q++) {
                const int ent = list[q], as_a = ent & 1;
                const double *st = stage + (long long)(ent >> 1) * STAGE;
                acc = acc + (pos < 21 ? st[(as_a ? S_AA : S_BB) + pos] : st[(as_a ? S_GA : S_GB) + pos - 21]);
            }
            if (pos < 21) {
                const bool diag = pos == 0 || pos == 2 || pos == 5 || pos == 9 || pos == 14 || pos == 20;
                Dl[mi * 21 + pos] = diag ? acc + damping : acc;
            } else {
                gv[mi * 6 + pos - 21] = acc;
            }
        }
        __syncthreads();
        // ---- the preconditioner: every block's LDL^T; x = 0, r = -g, z = M^-1 r, p = z
        int fail = NO_ROW;
        for (int mi = tid; mi < nn; mi += NT) {
            double f[21];
#pragma unroll
            for (int k = 0; k < 21; k++) f[k] = Dl[mi * 21 + k];
            int badj = -1;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double d = f[tri_lower(j, j)];
#pragma unroll
                for (int k = 0; k < j; k++) d = d - (f[tri_lower(j, k)] * f[tri_lower(j, k)]) * f[tri_lower(k, k)];
                f[tri_lower(j, j)] = d;
                if (badj < 0 && !(d > 0.0 && fin(d))) badj = j;
#pragma unroll
                for (int i = j + 1; i < 6; i++) {
                    double l = f[tri_lower(i, j)];
#pragma unroll
                    for (int k = 0; k < j; k++) l = l - (f[tri_lower(i, k)] * f[tri_lower(j, k)]) * f[tri_lower(k, k)];
                    f[tri_lower(i, j)] = l / d;
                }
            }
            if (badj >= 0) fail = 6 * mi + badj < fail ? 6 * mi + badj : fail;
            double r[6], z[6];
#pragma unroll
            for (int k = 0; k < 6; k++) r[k] = -gv[mi * 6 + k];
            block_solve(f, r, z);
#pragma unroll
            for (int k = 0; k < 21; k++) Lf[mi * 21 + k] = f[k];
#pragma unroll
            for (int k = 0; k < 6; k++) {
                xv[mi * 6 + k] = 0.0;
                rv[mi * 6 + k] = r[k];
                zv[mi * 6 + k] = z[k];
                pv[mi * 6 + k] = z[k];
            }
        }
        fail = block_min(fail, wcnt, tid);                   // its barriers also publish r, z, p
        if (fail != NO_ROW) return fail;                     // uniform

        // ---- conjugate gradients
        double rz = dot(rv, zv, n, wsum, tid);
        const double rz0 = rz;
        int steps = 0;
#pragma unroll 1
        for (int cg = 0; cg < cg_iterations; cg++) {
            double part = 0.0;
            for (int row = tid; row < n; row += NT) {
                const int mi = row / 6, i = row - 6 * mi;
                double x[6];
#pragma unroll
                for (int k = 0; k < 6; k++) x[k] = Dl[mi * 21 + (i >= k ? tri_lower(i, k) : tri_lower(k, i))] * pv[mi * 6 + k];
                double q = sum6(x);
                for (int t = off[mi + 1]; t < off[mi + 2]; t++) {
                    const int ent = list[t], e = ent >> 1, as_a = ent & 1;
                    const int a = g.first[e];
                    if (a < 1) continue;
                    const double *B = stage + (long long)e * STAGE + S_BA;
                    const double *po = pv + (as_a ? g.second[e] - 1 : a - 1) * 6;
#pragma unroll
                    for (int k = 0; k < 6; k++) x[k] = (as_a ? B[6 * k + i] : B[6 * i + k]) * po[k];
                    q = q + sum6(x);
                }
                qv[row] = q;
                part = part + pv[row] * q;
            }
            const double pq = block_sum(part, wsum, tid);
            if (!(pq > 0.0 && fin(pq))) break;               // uniform
            const double alpha = rz / pq;
            for (int mi = tid; mi < nn; mi += NT) {
                double f[21], r[6], z[6];
#pragma unroll
                for (int k = 0; k < 21; k++) f[k] = Lf[mi * 21 + k];
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    xv[mi * 6 + k] = xv[mi * 6 + k] + alpha * pv[mi * 6 + k];
                    r[k] = rv[mi * 6 + k] - alpha * qv[mi * 6 + k];
                    rv[mi * 6 + k] = r[k];
                }
                block_solve(f, r, z);
#pragma unroll
                for (int k = 0; k < 6; k++) zv[mi * 6 + k] = z[k];
            }
            __syncthreads();
            const double rz1 = dot(rv, zv, n, wsum, tid);
            steps++;
            if (rz1 <= tol2 * rz0) break;
            const double beta = rz1 / rz;
            for (int row = tid; row < n; row += NT) pv[row] = zv[row] + beta * pv[row];
            rz = rz1;
            __syncthreads();
        }
        if (tid == 0) steps_of[it] = steps;
        __syncthreads();                                     // x is read next by other threads than wrote it
        delta = xv;
        return -1;
    }
};

__global__ __launch_bounds__(NT) void sparse_kernel(const int *__restrict__ edge_first, const int *__restrict__ edge_second,
                                                    const double *__restrict__ edge_T, const double *__restrict__ edge_info,
                                                    int n_nodes, int n_edges, const double *__restrict__ C_in, double chi, double damping,
                                                    int n_iter, int cg_iterations, double cg_tol, double *workspace, long long ws_words,
                                                    double *C, int *__restrict__ status, int *__restrict__ iterations,
                                                    int *__restrict__ used_edges, int *__restrict__ skipped_edges,
                                                    int *__restrict__ failed_row, double *__restrict__ cost_in,
                                                    double *__restrict__ cost_out, double *__restrict__ edge_chi2,
                                                    int *__restrict__ cg_steps) {
    __shared__ double wsum[WAVES];
    __shared__ int wcnt[WAVES];
    __shared__ int sa[NT], sb[NT];
    __shared__ int cur[SSLL_MAX_NODES + 1];              // per node: its count, then the cursor into its list
    __shared__ int seg[NT];
    __shared__ int steps_of[SSLL_GRAPH_MAX_ITER];

    const int tid = threadIdx.x;
    const long long gi = blockIdx.x;
    const Graph g = graph_of(edge_first, edge_second, edge_T, edge_info, n_nodes, n_edges, n_nodes, gi);      // no band: b - a < n_nodes
    C += gi * n_nodes * 12;

    const int nn = n_nodes - 1, n = 6 * nn;
    double *stage = workspace + gi * ws_words;
    double *Dl = stage + (long long)STAGE * n_edges, *Lf = Dl + 21 * nn;
    double *gv = Lf + 21 * nn, *xv = gv + n, *rv = xv + n, *zv = rv + n, *pv = zv + n, *qv = pv + n;
    double *trial = qv + n;
    int *off = reinterpret_cast<int *>(trial + (long long)n_nodes * 12), *list = off + n_nodes + 1;

    if (tid < SSLL_GRAPH_MAX_ITER) steps_of[tid] = 0;    // the driver's first barriers publish it
    SparseSolver solver{g, C, chi, damping, cg_tol * cg_tol, cg_iterations, stage, Dl, Lf, gv, xv, rv, zv, pv, qv, off, list,
                        wsum, wcnt, sa, sb, cur, seg, steps_of};
    gauss_newton(solver, g, C_in + gi * n_nodes * 12, C, trial, chi, n_iter, wsum, wcnt,
                 GraphOut{status, iterations, used_edges, skipped_edges, failed_row, cost_in, cost_out, edge_chi2 + gi * n_edges}, gi);
    // attempted or not, the driver's last barriers came after the last write of steps_of: zeros where no step was taken
    if (tid < SSLL_GRAPH_MAX_ITER) cg_steps[gi * SSLL_GRAPH_MAX_ITER + tid] = steps_of[tid];
}

inline int sparse_shape(int n_graphs, int n_nodes, int n_edges) {
    if (n_graphs <= 0 || n_nodes <= 0 || n_edges <= 0) return SSLAM_E_INVALID;
    if (n_nodes > SSLL_MAX_NODES || n_edges > SSLL_MAX_EDGES || n_graphs > SSLL_MAX_GRAPHS) return SSLAM_E_UNSUPPORTED;
    return SSLAM_OK;
}

inline int launched(void) {
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}

}  // namespace

extern "C" int ssll_version(void) { return 100; }
extern "C" const char *ssll_arch(void) { return "gfx950"; }
extern "C" long long ssll_launch_count(void) { return __atomic_load_n(&g_launches, __ATOMIC_RELAXED); }

extern "C" int ssll_frame_signatures(const float *desc, const float *scores, int n_frames, int k, int d, void *workspace, float *sig,
                                     void *stream) {
    if (!desc || !scores || !workspace || !sig || n_frames <= 0 || k <= 0 || d <= 0) return SSLAM_E_INVALID;
    if (misaligned(desc, 4) || misaligned(scores, 4) || misaligned(workspace, 4) || misaligned(sig, 4)) return SSLAM_E_INVALID;
    if (n_frames > SSLL_MAX_FRAMES || k > SSLL_MAX_K || !width_ok(d)) return SSLAM_E_UNSUPPORTED;
    float *raw = (float *)workspace;
    hipLaunchKernelGGL(raw_kernel, dim3((unsigned)n_frames), dim3((unsigned)d), 0, (hipStream_t)stream, desc, scores, k, d, raw);
    if (launched() != SSLAM_OK) return SSLAM_E_LAUNCH;
    const int groups = (n_frames + SSLL_FRAMES_PER_GROUP - 1) / SSLL_FRAMES_PER_GROUP;
    hipLaunchKernelGGL(sig_kernel, dim3((unsigned)groups), dim3((unsigned)d), 0, (hipStream_t)stream, (const float *)raw, n_frames, d, sig);
    return launched();
}

extern "C" int ssll_loop_candidates(const float *sig, int n_frames, int d, int min_gap, float min_sim, int per_frame, int suppress,
                                    int32_t *first, int32_t *second, float *sim, int32_t *count, void *stream) {
    if (!sig || !first || !second || !sim || !count || n_frames <= 0 || d <= 0) return SSLAM_E_INVALID;
    if (min_gap < 1 || per_frame < 1 || suppress < 0 || !(min_sim - min_sim == 0.0f)) return SSLAM_E_INVALID;
    if (misaligned(sig, 16) || misaligned(first, 4) || misaligned(second, 4) || misaligned(sim, 4) || misaligned(count, 4)) return SSLAM_E_INVALID;
    if (n_frames > SSLL_MAX_FRAMES || !width_ok(d) || per_frame > SSLL_MAX_PER_FRAME) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(candidates_kernel, dim3((unsigned)n_frames), dim3(NT), 0, (hipStream_t)stream, sig, n_frames, d, min_gap, min_sim,
                       per_frame, suppress, (int *)first, (int *)second, sim, (int *)count);
    return launched();
}

extern "C" size_t ssll_pose_graph_sparse_workspace_bytes(int n_graphs, int n_nodes, int n_edges) {
    if (sparse_shape(n_graphs, n_nodes, n_edges) != SSLAM_OK) return 0;
    return (size_t)n_graphs * (size_t)workspace_words(n_nodes, n_edges) * sizeof(double);
}

extern "C" int ssll_pose_graph_sparse(const int32_t *edge_first, const int32_t *edge_second, const double *edge_T, const double *edge_info,
                                      int n_graphs, int n_nodes, int n_edges, const double *C_in, double huber_chi, double damping,
                                      int n_iter, int cg_iterations, double cg_tol, void *workspace, double *C, int32_t *status,
                                      int32_t *iterations, int32_t *used_edges, int32_t *skipped_edges, int32_t *failed_row,
                                      double *cost_in, double *cost, double *edge_chi2, int32_t *cg_steps, void *stream) {
    if (graph_operands(edge_first, edge_second, edge_T, edge_info, C_in, huber_chi, damping, n_iter, SSLL_GRAPH_MAX_ITER, workspace, C,
                       status, iterations, used_edges, skipped_edges, failed_row, cost_in, cost, edge_chi2) != SSLAM_OK)
        return SSLAM_E_INVALID;
    if (!cg_steps || misaligned(cg_steps, 4) || !finite_nonnegative(cg_tol) || cg_iterations <= 0) return SSLAM_E_INVALID;
    if (sparse_shape(n_graphs, n_nodes, n_edges) == SSLAM_E_INVALID) return SSLAM_E_INVALID;
    if (sparse_shape(n_graphs, n_nodes, n_edges) != SSLAM_OK || cg_iterations > SSLL_MAX_CG) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(sparse_kernel, dim3((unsigned)n_graphs), dim3(NT), 0, (hipStream_t)stream, (const int *)edge_first,
                       (const int *)edge_second, edge_T, edge_info, n_nodes, n_edges, C_in, huber_chi, damping, n_iter, cg_iterations,
                       cg_tol, (double *)workspace, workspace_words(n_nodes, n_edges), C, (int *)status, (int *)iterations,
                       (int *)used_edges, (int *)skipped_edges, (int *)failed_row, cost_in, cost, edge_chi2, (int *)cg_steps);
    return launched();
}
