// gauss_newton.h - the Gauss-Newton driver of include/sslam_graph.h (THE PASS, THE ITERATION), shared by csrc_graph/pose_graph.hip
// (the banded solve) and csrc_loop/loop.hip (the sparse solve): one statement of the slot rules, the accept rule and the status
// codes, so both libraries give the same bits.  Included inside an anonymous namespace that defines NT = 256 and WAVES = 4.
//   gauss_newton<Solver>   C <- C_in and the slot counts, the not-attempted exit, cost_in, the steps (the solver's delta, the trial
//                          poses, accept or stop), the final edge_chi2 pass, the status words.  A Solver supplies
//                            void prepare()                         once per launch, after the exit, every thread
//                            int step(int it, const double *&delta) one linear solve at the poses C: -1 and the 6 (n_nodes - 1)
//                                                                   deltas, published by a barrier, or the first failed row
//   graph_operands         what the two host entries judge alike, before anything is launched
#pragma once

#include "edge_terms.h"           // STAGE, S_*: the words staged per edge; fin, the pose products, Edge, edge_eval, edge_stage, pose_update

static_assert(NT == 256 && WAVES == 4, "block_sum and block_count add four waves' words in a fixed order");

inline bool finite_positive(double v) { return v > 0.0 && v - v == 0.0; }
inline bool finite_nonnegative(double v) { return v >= 0.0 && v - v == 0.0; }
inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// the operands of sslg_pose_graph and ssll_pose_graph_sparse that are judged alike: SSLAM_E_INVALID or SSLAM_OK (each entry's size
// limits, which give SSLAM_E_UNSUPPORTED, come after it)
inline int graph_operands(const int32_t *edge_first, const int32_t *edge_second, const double *edge_T, const double *edge_info,
                          const double *C_in, double huber_chi, double damping, int n_iter, int max_iter, const void *workspace,
                          const double *C, const int32_t *status, const int32_t *iterations, const int32_t *used_edges,
                          const int32_t *skipped_edges, const int32_t *failed_row, const double *cost_in, const double *cost,
                          const double *edge_chi2) {
    for (const void *p : {(const void *)edge_T, (const void *)edge_info, (const void *)C_in, workspace, (const void *)C,
                          (const void *)cost_in, (const void *)cost, (const void *)edge_chi2})
        if (!p || misaligned(p, 8)) return SSLAM_E_INVALID;
    for (const void *p : {(const void *)edge_first, (const void *)edge_second, (const void *)status, (const void *)iterations,
                          (const void *)used_edges, (const void *)skipped_edges, (const void *)failed_row})
        if (!p || misaligned(p, 4)) return SSLAM_E_INVALID;
    if (!finite_positive(huber_chi) || !finite_nonnegative(damping) || n_iter < 0 || n_iter > max_iter || C == C_in) return SSLAM_E_INVALID;
    return SSLAM_OK;
}

__device__ __forceinline__ double block_sum(double p, double *wsum, int tid) {
    p = p + __shfl_xor(p, 32);
    p = p + __shfl_xor(p, 16);
    p = p + __shfl_xor(p, 8);
    p = p + __shfl_xor(p, 4);
    p = p + __shfl_xor(p, 2);
    p = p + __shfl_xor(p, 1);
    if ((tid & 63) == 0) wsum[tid >> 6] = p;
    __syncthreads();
    p = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __syncthreads();                                     // wsum may be written again
    return p;
}

__device__ __forceinline__ int block_count(int n, int *wcnt, int tid) {
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
    if ((tid & 63) == 0) wcnt[tid >> 6] = n;
    __syncthreads();
    n = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
    __syncthreads();
    return n;
}

struct Graph {                      // one graph of the launch; band = n_nodes where the solver has none
    const int *first, *second;
    const double *T, *info;
    int n_nodes, n_edges, band;
};

__device__ __forceinline__ Graph graph_of(const int *edge_first, const int *edge_second, const double *edge_T, const double *edge_info,
                                          int n_nodes, int n_edges, int band, long long gi) {
    Graph g;
    g.first = edge_first + gi * n_edges;
    g.second = edge_second + gi * n_edges;
    g.T = edge_T + gi * n_edges * 12;
    g.info = edge_info + gi * n_edges * 21;
    g.n_nodes = n_nodes;
    g.n_edges = n_edges;
    g.band = band;
    return g;
}

__device__ __forceinline__ bool edge_used(const Graph &g, int e, int &a, int &b) {
    a = g.first[e];
    b = g.second[e];
    if (!(0 <= a && a < b && b < g.n_nodes && b - a <= g.band)) return false;
    bool ok = true;
    const double *t = g.T + (long long)e * 12, *h = g.info + (long long)e * 21;
    for (int k = 0; k < 12; k++) ok = ok && fin(t[k]);
    for (int k = 0; k < 21; k++) ok = ok && fin(h[k]);
    return ok;
}

// the cost at the poses X, in the pass' order; with chi2, s of every used edge (+0.0 elsewhere) is written there
__device__ __forceinline__ double graph_cost(const Graph &g, const double *X, double chi, double *chi2, double *wsum, int tid) {
    double part = 0.0;
    for (int e = tid; e < g.n_edges; e += NT) {
        int a, b;
        double rho = 0.0, s = 0.0;
        if (edge_used(g, e, a, b)) {
            Edge ed;
            edge_eval(X + (long long)a * 12, X + (long long)b * 12, g.T + (long long)e * 12, g.info + (long long)e * 21, chi, ed);
            rho = ed.rho;
            s = ed.s;
        }
        part = part + rho;
        if (chi2) chi2[e] = s;
    }
    return block_sum(part, wsum, tid);
}

// the per-graph output words of a launch, and graph gi's edge_chi2
struct GraphOut {
    int *status, *iterations, *used_edges, *skipped_edges, *failed_row;
    double *cost_in, *cost, *edge_chi2;
};

// One graph, by the 256 threads of its workgroup.  C_in, C and trial are the graph's own poses; wsum and wcnt are WAVES words of
// LDS each.
template <class Solver>
__device__ __forceinline__ void gauss_newton(Solver &solver, const Graph &g, const double *C_in, double *C, double *trial, double chi,
                                             int n_iter, double *wsum, int *wcnt, const GraphOut &out, long long gi) {
    const int tid = threadIdx.x, n_nodes = g.n_nodes, n_edges = g.n_edges;

    // ---- C <- C_in; the edge counts; whether anything is attempted
    int bad = 0, used = 0, skipped = 0;
    for (int k = tid; k < n_nodes * 12; k += NT) {
        const double v = C_in[k];
        C[k] = v;
        bad += !fin(v);
    }
    for (int e = tid; e < n_edges; e += NT) {
        int a, b;
        const bool u = edge_used(g, e, a, b);
        used += u;
        skipped += !u && a != -1;
    }
    bad = block_count(bad, wcnt, tid);
    used = block_count(used, wcnt, tid);
    skipped = block_count(skipped, wcnt, tid);
    if (tid == 0) {
        out.used_edges[gi] = used;
        out.skipped_edges[gi] = skipped;
    }
    if (bad != 0 || used == 0) {                         // not attempted (uniform)
        for (int e = tid; e < n_edges; e += NT) out.edge_chi2[e] = 0.0;
        if (tid == 0) {
            out.status[gi] = 3;
            out.iterations[gi] = 0;
            out.failed_row[gi] = -1;
            out.cost_in[gi] = 0.0;
            out.cost[gi] = 0.0;
        }
        return;
    }
    __syncthreads();                                     // C is read below by other threads than wrote it
    solver.prepare();

    const double c_in = graph_cost(g, C, chi, nullptr, wsum, tid);
    double cur_cost = c_in;
    int accepted = 0, failed = -1;
    bool first_failed = false;

#pragma unroll 1
    for (int it = 0; it < n_iter; it++) {
        const double *dv;
        const int fail = solver.step(it, dv);
        if (fail >= 0) {                                 // uniform
            failed = fail;
            first_failed = it == 0;
            break;
        }

        // ---- the trial poses and their cost
        for (int m = tid; m < n_nodes; m += NT) {
            double cm[12], to[12];
#pragma unroll
            for (int k = 0; k < 12; k++) cm[k] = C[(long long)m * 12 + k];
            if (m == 0) {
#pragma unroll
                for (int k = 0; k < 12; k++) to[k] = cm[k];
            } else {
                double delta[6];
#pragma unroll
                for (int k = 0; k < 6; k++) delta[k] = dv[6 * (m - 1) + k];
                pose_update(cm, delta, to);
            }
#pragma unroll
            for (int k = 0; k < 12; k++) trial[(long long)m * 12 + k] = to[k];
        }
        __syncthreads();
        const double c_trial = graph_cost(g, trial, chi, nullptr, wsum, tid);
        if (!(fin(c_trial) && c_trial < cur_cost)) break;      // uniform: every thread holds the same total
        cur_cost = c_trial;
        accepted++;
        for (int k = tid; k < n_nodes * 12; k += NT) C[k] = trial[k];
        __syncthreads();
    }

    graph_cost(g, C, chi, out.edge_chi2, wsum, tid);
    if (tid == 0) {
        out.status[gi] = accepted > 0 ? 0 : (first_failed ? 2 : 1);
        out.iterations[gi] = accepted;
        out.failed_row[gi] = failed;
        out.cost_in[gi] = c_in;
        out.cost[gi] = cur_cost;
    }
}
