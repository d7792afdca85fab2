/*
 * sslam_graph.h - C ABI of libsslam_graph.so: the third native library of the project (gfx950), the pose graph over the relative
 * poses and information matrices that libsslam_hip.so (sslam_hip.h: sslam_pose_refine_pairs) produced.  Same conventions as there:
 * every pointer is a CALLER-OWNED DEVICE pointer, the library never allocates, frees, synchronises or reads back; `stream` is a
 * hipStream_t passed as void*; the return value is SSLAM_OK or a negative SSLAM_E_* code of sslam_hip.h; results are written with
 * ordinary vector stores, there are no atomics: every entry can be captured in a graph.  All floating point is IEEE float64,
 * + - * / sqrt only, every operation named below rounded once, in the order written (built with -ffp-contract=off), no
 * transcendental function: a result is the same bits as tests/pose_graph_ref.py.  The entries carry the prefix sslg_.
 */
#ifndef SSLAM_GRAPH_H
#define SSLAM_GRAPH_H

#include <stddef.h>
#include <stdint.h>

#include "sslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ALIGNMENT, every entry that takes device pointers: the LEAST alignment in bytes of each pointer argument - the widest access
 * the entry's kernel makes to it (4 an int32 word, 8 a float64).  A pointer that misses its alignment: SSLAM_E_INVALID before
 * anything is launched, nothing written.  A result is a function of the operands' values, not of their addresses
 * (tests/test_gpu_pose_graph.py runs every pointer at its least alignment, just past and just before a 256-byte boundary).
 * No entry takes a stride.
 *   sslg_chain_poses: T 8, C_start 8, C 8
 *   sslg_pose_graph: edge_first 4, edge_second 4, edge_T 8, edge_info 8, C_in 8, workspace 8, C 8, status 4, iterations 4, used_edges 4, skipped_edges 4, failed_row 4, cost_in 8, cost 8, edge_chi2 8
 */

/* ---- SIZE LIMITS: the expressions the dispatch code tests, the code returned where one is false, and the widths in bits of the
 * kernel's index expressions (tests/graph_table.py restates them, tests/test_pose_graph_cpu.py holds one past each to its code).
 *   sslg_chain_poses: n_graphs <= 0x7fffffff / 256 and n_nodes <= 4096, else SSLAM_E_UNSUPPORTED. offsets: graph * n_nodes * 12 64
 *   sslg_pose_graph: band <= 32, else SSLAM_E_UNSUPPORTED; n_nodes <= 4096, else SSLAM_E_UNSUPPORTED; n_edges <= 1048576, else SSLAM_E_UNSUPPORTED; n_graphs <= 65535, else SSLAM_E_UNSUPPORTED. offsets: graph * n_edges * 21 64, graph * workspace doubles 64, row * (6 * band + 6) 31
 */

int sslg_version(void);
const char *sslg_arch(void);          /* "gfx950" */
long long sslg_launch_count(void);    /* kernels this library has launched in this process - a launch that returned
                                         SSLAM_E_LAUNCH is not counted (diagnostic; relaxed atomic) */

#define SSLG_MAX_BAND 32
#define SSLG_MAX_NODES 4096
#define SSLG_MAX_EDGES 1048576
#define SSLG_MAX_GRAPHS 65535
#define SSLG_GRAPH_MAX_ITER 16

/* A pose is [R | t], 12 float64 row-major (m[4 * i + j], the translation at j = 3).  Two operations on poses, used by both entries:
 *   A o B (first B, then A):   R_ij = (A_i0 * B_0j + A_i1 * B_1j) + A_i2 * B_2j;
 *                              t_i  = ((A_i0 * B_03 + A_i1 * B_13) + A_i2 * B_23) + A_i3
 *                              - the row-by-row product of sslam_pose_refine_pairs' update;
 *   inv(A):                    R_ij = A_ji;   t_i = -((A_0i * A_03 + A_1i * A_13) + A_2i * A_23).
 *
 * Chained world -> camera poses: n_graphs independent chains of n_nodes poses from the n_nodes - 1 transforms camera i -> camera
 * i + 1 of each.
 *   T (n_graphs, n_nodes - 1, 12); may be NULL when n_nodes is 1.   C_start (n_graphs, 12) or NULL: C_0, [I | 0] if NULL.
 *   C (n_graphs, n_nodes, 12):  C_0 = the start pose bit for bit, C_{i+1} = T_i o C_i.
 * Launch: one kernel, one thread per chain, 256-thread workgroups.  Every element of C is written; nothing else is.
 * SSLAM_E_INVALID: a NULL C, a NULL T with n_nodes > 1, n_graphs or n_nodes <= 0, a pointer that misses its alignment, C equal to
 * C_start.  SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
int sslg_chain_poses(const double *T, const double *C_start, int n_graphs, int n_nodes, double *C, void *stream);

/* ---- The pose graph: robust Gauss-Newton over the world -> camera poses C_0 .. C_{n_nodes-1} of each of n_graphs independent
 * graphs, on n_edges edge slots each; node 0 is the anchor.  One launch, one 256-thread workgroup per graph.
 *   edge_first, edge_second (n_graphs, n_edges) int32: the nodes a, b of every slot; a == -1: an absent slot.
 *   edge_T (n_graphs, n_edges, 12): the measured [R | t], camera a -> camera b, as sslam_pose_refine_pairs writes T.
 *   edge_info (n_graphs, n_edges, 21): the upper triangle, row-major, of the measurement's 6 x 6 information matrix H as that entry
 *     writes info: left perturbation in camera b, parameters (vx, vy, vz, wx, wy, wz).  H is read as symmetric.
 *   C_in (n_graphs, n_nodes, 12): the initial poses.   band: 1 .. SSLG_MAX_BAND.   huber_chi: finite, > 0.   damping: finite, >= 0.
 *   n_iter: 0 .. SSLG_GRAPH_MAX_ITER.   workspace: sslg_pose_graph_workspace_bytes(n_graphs, n_nodes, band) bytes, 8-byte aligned;
 *     nothing is expected in it and nothing useful left in it.
 * USED EDGES: a slot is used iff 0 <= a < b < n_nodes, b - a <= band, and every entry of its T and its info is finite.  Every
 *   other slot is skipped; skipped_edges counts the skipped slots whose a is not -1.  Duplicates of one (a, b) are all used.
 * AN EDGE at poses C:
 *     T_p = C_b o inv(C_a);   D = T_p o inv(T_meas);
 *     r = (D_03, D_13, D_23, 0.5 * (D_21 - D_12), 0.5 * (D_02 - D_20), 0.5 * (D_10 - D_01));
 *     Hr_i = ((((H_i0 * r_0 + H_i1 * r_1) + H_i2 * r_2) + H_i3 * r_3) + H_i4 * r_4) + H_i5 * r_5;
 *     s = ((((r_0 * Hr_0 + r_1 * Hr_1) + r_2 * Hr_2) + r_3 * Hr_3) + r_4 * Hr_4) + r_5 * Hr_5;
 *     if s <= huber_chi * huber_chi:  w = 1, rho = s;   otherwise (a NaN included):  q = sqrt(s), w = huber_chi / q,
 *     rho = (2 * huber_chi) * q - huber_chi * huber_chi.
 *   The cost at C is the sum of rho over the slots in the order of sslam_pose_refine_pairs' pass: thread t of 256 adds, from +0.0,
 *   the terms of the slots t, t + 256, ... ascending, a slot that is not used adding +0.0; lanes by xor 32 .. 1; the four waves
 *   ((w0 + w1) + w2) + w3.
 * JACOBIANS for the left perturbations C_i <- exp(xi_i) C_i:  J_b = I;  J_a = -Ad, with [R | t] = T_p,
 *     B_0j = t_1 * R_2j - t_2 * R_1j;   B_1j = t_2 * R_0j - t_0 * R_2j;   B_2j = t_0 * R_1j - t_1 * R_0j      ([t]x R);
 *     Ad = [[R, B], [0, R]], 6 x 6, the zero block +0.0 and multiplied like any other entry.
 *   With sum6_k x_k = ((((x_0 + x_1) + x_2) + x_3) + x_4) + x_5:
 *     P_ij = sum6_k H_ik * Ad_kj;    Q_ij = sum6_k Ad_ki * P_kj;    ga_i = sum6_k Ad_ki * Hr_k.
 * NORMAL EQUATIONS A delta = -g over the nodes 1 .. n_nodes - 1, six rows each, row 6 * (node - 1) + i; node 0's rows and columns
 *   are dropped.  Only the lower triangle of A is formed.  Every entry of A and g starts at +0.0 and takes, in ascending slot order
 *   over the used edges, per edge and in this order where one entry takes two terms of one edge (it never does: a < b):
 *     block (b, b), i >= j:  + w * H_ij;          g of b:  + w * Hr_i;
 *     and, when a >= 1:  block (b, a), all i, j:  + (-(w * P_ij));     block (a, a), i >= j:  + w * Q_ij;     g of a:  + (-(w * ga_i)).
 *   Then A_ii = A_ii + damping for every row.
 * SOLVE with n = 6 * (n_nodes - 1) and bw = 6 * band + 5, an unpivoted banded LDL^T written as the 6 x 6 one of sslam_hip.h:
 *     for j = 0 .. n-1:   D_j = A_jj, then for k = max(0, j - bw) .. j-1 ascending  D_j = D_j - (L_jk * L_jk) * D_k;
 *         for i = j+1 .. min(n-1, j + bw):  L_ij = A_ij, then for k ascending from max(0, i - bw) to j-1
 *                                           L_ij = L_ij - (L_ik * L_jk) * D_k;   L_ij = L_ij / D_j;
 *     y_i = -g_i, then for k ascending from max(0, i - bw) to i-1  y_i = y_i - L_ik * y_k                       (i = 0 .. n-1);
 *     delta_i = y_i / D_i, then for k = i+1 .. min(n-1, i + bw) ascending  delta_i = delta_i - L_ki * delta_k   (i = n-1 .. 0).
 *   The first pivot D_j that is not finite and > 0 ENDS the iteration; nothing past it is computed; failed_row = j.
 * UPDATE of node m >= 1 with delta = rows 6 * (m - 1) .. + 5 = (vx, vy, vz, wx, wy, wz): sslam_pose_refine_pairs' quaternion update
 *   of C_m (w = 1, x = 0.5 * wx, ... each divided by sqrt(((w*w + x*x) + y*y) + z*z); C_m <- [dR R | dR t + v]).  Node 0 is copied.
 * ITERATION.  cost_in = the cost at C_in.  Up to n_iter times: the normal equations at the current poses, the solve, the trial
 *   poses, the cost at the trial; the trial is ACCEPTED - becomes the current poses - iff its cost is finite and < the current
 *   cost.  The first trial that is not accepted, or a failed pivot, ends the iteration.
 * Outputs per graph (every element is written; nothing else is, outside the workspace):
 *     C (n_graphs, n_nodes, 12)           the current poses at the end; C_0 = C_in's bit for bit;
 *     status (n_graphs) int32             0 optimised (a step was accepted); 1 no step accepted (n_iter 0, a minimum already, the
 *                                         first trial rejected); 2 a failed pivot at the first step; 3 not attempted: no used edge,
 *                                         or a non-finite entry in C_in;
 *     iterations (n_graphs) int32         the accepted steps;
 *     used_edges, skipped_edges (n_graphs) int32;
 *     failed_row (n_graphs) int32         the row of the pivot that ended the iteration, at any step, else -1; its node is
 *                                         failed_row / 6 + 1;
 *     cost_in, cost (n_graphs) float64    the cost at C_in and at C;
 *     edge_chi2 (n_graphs, n_edges)       s of every used edge at C, +0.0 for every other slot.
 *   Under status 1, 2 and 3 C = C_in bit for bit and cost = cost_in; under status 3 both costs and all of edge_chi2 are +0.0,
 *   iterations 0, failed_row -1, and the two edge counts are still what they are.  A graph's outputs are a function of that
 *   graph's operands and the scalars alone.  C and C_in are different arrays.
 * WHERE THINGS LIVE.  LDS, M = bw + 1: the lower triangle of the trailing M x M block of the factorisation, M (M + 1) / 2 words,
 *   and a ring of M words (y, then delta) - 64 KB at band 20, 159 192 bytes at band 32 - beside 2 KB for the staged edges' node
 *   numbers and the wave partial sums.  The factorisation runs right-looking on that window; every element takes its updates in
 *   ascending k, so the bits are those of the statement above.  Workspace, per graph, in float64 words: the band of A row-major,
 *   n * M words, entry (i, j) at i * M + (j - i + bw), overwritten column by column by the factor (D_j at j * M, L_ij at
 *   j * M + (i - j)); g, y and delta, 3 * n; the trial poses, 12 * n_nodes; the staged terms of 256 edges, 256 * 90.
 * SSLAM_E_INVALID: a NULL pointer; n_graphs, n_nodes, n_edges or band <= 0; huber_chi not finite and > 0; damping not finite and
 * >= 0; n_iter outside 0 .. SSLG_GRAPH_MAX_ITER; a pointer that misses its alignment; C equal to C_in.  SSLAM_E_UNSUPPORTED: SIZE
 * LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
size_t sslg_pose_graph_workspace_bytes(int n_graphs, int n_nodes, int band);      /* 0 for arguments the entry refuses */
int sslg_pose_graph(const int32_t *edge_first, const int32_t *edge_second, const double *edge_T, const double *edge_info, int n_graphs,
                    int n_nodes, int n_edges, const double *C_in, int band, double huber_chi, double damping, int n_iter,
                    void *workspace, double *C, int32_t *status, int32_t *iterations, int32_t *used_edges, int32_t *skipped_edges,
                    int32_t *failed_row, double *cost_in, double *cost, double *edge_chi2, void *stream);

#ifdef __cplusplus
}
#endif
#endif
