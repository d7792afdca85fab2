/*
 * sslam_loop.h - C ABI of libsslam_loop.so: the fourth native library of the project (gfx950), loop closures - a place signature
 * per frame, far pairs proposed from the signatures, and a pose graph whose solve does not depend on where its edges lie.  Same
 * conventions as sslam_graph.h: every pointer is a CALLER-OWNED DEVICE pointer, the library never allocates, frees, synchronises
 * or reads back; `stream` is a hipStream_t passed as void*; the return value is SSLAM_OK or a negative SSLAM_E_* code of
 * sslam_hip.h; results are written with ordinary vector stores and there are no floating-point atomics: every entry can be
 * captured in a graph.  Built with -ffp-contract=off: every operation named below is rounded once, in the order written, and a
 * fused multiply-add happens exactly where fmaf is written: a result is the same bits as tests/loop_ref.py.  The entries carry
 * the prefix ssll_.
 */
#ifndef SSLAM_LOOP_H
#define SSLAM_LOOP_H

#include <stddef.h>
#include <stdint.h>

#include "sslam_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ALIGNMENT, every entry that takes device pointers: the LEAST alignment in bytes of each pointer argument - the widest access
 * the entry's kernels make to it (4 an int32 or float32 word, 8 a float64, 16 four float32).  A pointer that misses its alignment:
 * SSLAM_E_INVALID before anything is launched, nothing written.  A result is a function of the operands' values, not of their
 * addresses (tests/test_gpu_loop.py runs every pointer at its least alignment, just past and just before a 256-byte boundary).
 * No entry takes a stride.
 *   ssll_frame_signatures: desc 4, scores 4, workspace 4, sig 4
 *   ssll_loop_candidates: sig 16, first 4, second 4, sim 4, count 4
 *   ssll_pose_graph_sparse: edge_first 4, edge_second 4, edge_T 8, edge_info 8, C_in 8, workspace 8, C 8, status 4, iterations 4, used_edges 4, skipped_edges 4, failed_row 4, cost_in 8, cost 8, edge_chi2 8, cg_steps 4
 */

/* ---- SIZE LIMITS: the expressions the dispatch code tests, the code returned where one is false, and the widths in bits of the
 * kernels' index expressions (tests/loop_table.py restates them, tests/test_loop_cpu.py holds one past each to its code).
 *   ssll_frame_signatures: n_frames <= 4096, else SSLAM_E_UNSUPPORTED; k <= 4096, else SSLAM_E_UNSUPPORTED; d == 128 or d == 256, else SSLAM_E_UNSUPPORTED. offsets: frame * k * d 64
 *   ssll_loop_candidates: n_frames <= 4096, else SSLAM_E_UNSUPPORTED; d == 128 or d == 256, else SSLAM_E_UNSUPPORTED; per_frame <= 8, else SSLAM_E_UNSUPPORTED. offsets: frame * d 31, frame * per_frame 31
 *   ssll_pose_graph_sparse: n_nodes <= 4096, else SSLAM_E_UNSUPPORTED; n_edges <= 65536, else SSLAM_E_UNSUPPORTED; n_graphs <= 65535, else SSLAM_E_UNSUPPORTED; cg_iterations <= 4096, else SSLAM_E_UNSUPPORTED. offsets: graph * n_edges * 21 64, graph * workspace doubles 64, slot * 90 31
 */

int ssll_version(void);
const char *ssll_arch(void);          /* "gfx950" */
long long ssll_launch_count(void);    /* kernels this library has launched in this process - a launch that returned
                                         SSLAM_E_LAUNCH is not counted (diagnostic; relaxed atomic) */

#define SSLL_MAX_FRAMES 4096
#define SSLL_MAX_K 4096
#define SSLL_MAX_PER_FRAME 8
#define SSLL_MAX_NODES 4096
#define SSLL_MAX_EDGES 65536
#define SSLL_MAX_GRAPHS 65535
#define SSLL_GRAPH_MAX_ITER 16
#define SSLL_MAX_CG 4096
#define SSLL_FRAMES_PER_GROUP 32

/* ---- Frame signatures: one unit float32 vector per frame from the banks the extraction returns, centred on the sequence.
 *   desc (n_frames, k, d) float32, d = 128 or 256;   scores (n_frames, k) float32;
 *   workspace: n_frames * d * 4 bytes (the raw sums); nothing is expected in it.      sig (n_frames, d) float32.
 *     raw_i[c]  = acc after acc = +0.0f; for kk = 0 .. k-1 ascending: acc = fmaf(scores[i][kk], desc[i][kk][c], acc);
 *     mean[c]   = (sum over the frames i = 0 .. n_frames-1 ascending, from +0.0f, one float32 add each, of raw_i[c]) / (float)n_frames;
 *     c_i[c]    = raw_i[c] - mean[c];
 *     ss_i      = the sum of c_i[c] * c_i[c] (a product, then adds) over c in this order: thread c of d holds its product; within
 *                 each wave of 64 (threads 64 v .. 64 v + 63) lanes are added by xor 32, 16, 8, 4, 2, 1; then the waves
 *                 ascending from wave 0: (w0 + w1) at d = 128, ((w0 + w1) + w2) + w3 at d = 256;
 *     sig_i[c]  = c_i[c] / fmaxf(sqrtf(ss_i), 1e-12f)      (sqrtf and / correctly rounded).
 *   A frame whose c_i is all zero - n_frames = 1 always - has a signature of zeros (of c_i's signs).
 *   WHY CENTRED: a frame's raw sum is dominated by what every frame of a sequence shares; the raw sums of different places have
 *   cosines above 0.99.  Taking the sequence's mean away leaves what tells places apart.
 * Launches: two.  (1) one workgroup of d threads per frame, thread c one column: raw into the workspace.  (2) one workgroup of d
 * threads per SSLL_FRAMES_PER_GROUP consecutive frames: the mean (every workgroup forms it anew, in the order above), then its
 * frames.  Every element of sig is written; nothing else is, outside the workspace.
 * SSLAM_E_INVALID: a NULL pointer; n_frames, k or d <= 0; a pointer that misses its alignment.  SSLAM_E_UNSUPPORTED: SIZE LIMITS
 * above.  Every refusal comes before anything is launched and writes nothing. */
int ssll_frame_signatures(const float *desc, const float *scores, int n_frames, int k, int d, void *workspace, float *sig,
                          void *stream);

/* ---- Loop candidates: for every frame i the most similar OLDER frames, in match_pairs' pair-list form.
 *   sig (n_frames, d) float32, d = 128 or 256.   min_gap >= 1.   min_sim finite.   per_frame 1 .. SSLL_MAX_PER_FRAME.
 *   suppress >= 0.
 *     S_ij = acc after acc = +0.0f; for c = 0 .. d-1 ascending: acc = fmaf(sig[i][c], sig[j][c], acc)
 *            - ONE chain, the similarity contract of the matcher (the oracle's sim_matrix(sig, sig)).
 *   Frame j is ELIGIBLE for i iff 0 <= j <= i - min_gap and S_ij >= min_sim (a NaN is not).  Up to per_frame times: pick among
 *   the eligible frames the one of greatest S_ij, of equal values (as == compares: -0.0 equals +0.0) the lowest j; then every j'
 *   with |j' - j| <= suppress stops being eligible.  Slot s of frame i is the s-th pick:
 *     first (n_frames * per_frame) int32    the older frame j; -1 in an empty slot;
 *     second (n_frames * per_frame) int32   i; -1 in an empty slot (so first < second in every filled slot);
 *     sim (n_frames * per_frame) float32    S_ij; +0.0 in an empty slot;
 *     count (n_frames) int32                the filled slots of frame i, which come first.
 * Launch: one kernel, one 256-thread workgroup per frame; thread t forms S_ij of j = t, t + 256, ... into LDS (16 KB at 4096
 * frames), the picks are block-wide arg-max reductions by (value descending, j ascending) - a total order, so the tree's shape
 * does not matter.  Every element of the four outputs is written; nothing else is.
 * SSLAM_E_INVALID: a NULL pointer; n_frames or d <= 0; min_gap < 1; per_frame < 1; suppress < 0; min_sim not finite; a pointer that
 * misses its alignment.  SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
int ssll_loop_candidates(const float *sig, int n_frames, int d, int min_gap, float min_sim, int per_frame, int suppress,
                         int32_t *first, int32_t *second, float *sim, int32_t *count, void *stream);

/* ---- The sparse pose graph: sslg_pose_graph (sslam_graph.h) with edges anywhere.  Operands as there, without `band`, with
 * cg_iterations (1 .. SSLL_MAX_CG) and cg_tol (finite, >= 0).  IEEE float64, + - * / sqrt only.  One launch, one 256-thread
 * workgroup per graph; no workgroup waits for another.
 * USED EDGES: a slot is used iff 0 <= a < b < n_nodes and every entry of its T and its info is finite - there is no band test.
 * The following are sslam_graph.h's, bit for bit, by its paragraphs: AN EDGE (T_p, r, Hr, s, w, rho and the cost's summation
 * order), JACOBIANS (Ad, P, Q, ga, sum6), UPDATE, ITERATION (the accept rule), and the outputs C, status (0 - 3), iterations,
 * used_edges, skipped_edges, failed_row, cost_in, cost, edge_chi2 with everything said there of status 1, 2 and 3.
 * What differs is how A delta = -g is solved: by preconditioned conjugate gradients on blocks.
 * BLOCKS.  Per node m >= 1: D_m (6 x 6, the lower triangle i >= j formed, read as symmetric) and g_m (6) start at +0.0 and take,
 *   in ascending slot order over the used edges incident to m:  as the edge's b:  D_m += w * H_ij,  g_m += w * Hr_i;
 *   as its a:  D_m += w * Q_ij,  g_m += -(w * ga_i).  Then damping is added to the six diagonal entries of D_m.
 *   Per used edge e with a >= 1:  B_e = -(w * P_ij), 6 x 6, block (b, a) of A; block (a, b) is its transpose.
 * PRECONDITIONER M = diag(D_m): the unpivoted 6 x 6 LDL^T of every D_m in the order of sslam_hip.h's STEP (D_j = H_jj, then
 *   k ascending D_j -= (L_jk * L_jk) * D_k; L_ij = H_ij, then k ascending L_ij -= (L_ik * L_jk) * D_k; L_ij /= D_j).  A node's
 *   factorisation stops at its first pivot that is not finite and > 0; the LOWEST such row 6 * (m - 1) + j over all nodes ENDS the
 *   iteration: failed_row = that row, status 2 at the first step.   z = M^-1 v per node is that STEP's two substitutions with
 *   y_i = v_i:  y_i -= L_ik * y_k (k ascending), z_i = y_i / D_i, then z_i -= L_ki * z_k (k = i+1 .. 5 ascending; i = 5 .. 0).
 * A DOT PRODUCT u . v over the n = 6 * (n_nodes - 1) rows, in the cost's order: thread t of 256 adds, from +0.0, the products
 *   u_i * v_i of the rows i = t, t + 256, ... ascending; lanes by xor 32 .. 1; the four waves ((w0 + w1) + w2) + w3.
 * PCG from x = 0:   r = -g;  z = M^-1 r;  p = z;  rz0 = rz = r . z;  steps = 0.   Up to cg_iterations times:
 *     q_m = D_m p_m:  q_i = sum6_k D_ik * p_k;  then per edge incident to m, in ascending slot order, when its a >= 1:
 *         m is its b:  q_i = q_i + sum6_k B_ik * (p_a)_k;       m is its a:  q_i = q_i + sum6_k B_ki * (p_b)_k;
 *     pq = p . q;  if pq is not finite and > 0: stop, x as it stands;
 *     alpha = rz / pq;  x_i = x_i + alpha * p_i;  r_i = r_i - alpha * q_i;  z = M^-1 r;  rz1 = r . z;  steps = steps + 1;
 *     if rz1 <= (cg_tol * cg_tol) * rz0: stop;
 *     beta = rz1 / rz;  p_i = z_i + beta * p_i;  rz = rz1.
 *   Running out of iterations uses x as it stands.  delta = x.
 * New output:  cg_steps (n_graphs, SSLL_GRAPH_MAX_ITER) int32: `steps` of every Gauss-Newton step whose solve began (a step
 *   ended by a failed pivot counts 0), 0 past the last; all 0 under status 3.
 * WHERE THINGS LIVE.  LDS: the per-node counts and cursors of the incidence lists (4097 int32), 2 KB for a chunk's node numbers and
 *   the wave partial sums.  Workspace, per graph, in float64 words, with N = n_nodes, nn = N - 1, E = n_edges: the staged terms
 *   of every slot, 90 * E (sslam_graph.h's 90 words: BB 21, BA 36, AA 21, GB 6, GA 6; B_e is BA); D_m's lower triangles, 21 * nn;
 *   their factors, 21 * nn; g, x, r, z, p, q, 36 * nn; the trial poses, 12 * N; then int32: the lists' offsets, N + 1, and the
 *   lists, 2 * E (entry = 2 * slot + (1 if the node is the slot's a)), rounded up to whole words:
 *   90 * E + 78 * nn + 12 * N + (N + 1 + 2 * E + 1) / 2.
 *   The incidence lists are built anew in every launch, without atomics on floating point and in a fixed order: counts by integer
 *   LDS atomics, an exclusive scan, then the slots 256 at a time, a slot's place in a node's list its rank among the chunk's.
 * SSLAM_E_INVALID: a NULL pointer; n_graphs, n_nodes, n_edges or cg_iterations <= 0; huber_chi not finite and > 0; damping or
 * cg_tol not finite and >= 0; n_iter outside 0 .. SSLL_GRAPH_MAX_ITER; a pointer that misses its alignment; C equal to C_in.
 * SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
size_t ssll_pose_graph_sparse_workspace_bytes(int n_graphs, int n_nodes, int n_edges);      /* 0 for arguments the entry refuses */
int ssll_pose_graph_sparse(const int32_t *edge_first, const int32_t *edge_second, const double *edge_T, const double *edge_info,
                           int n_graphs, int n_nodes, int n_edges, const double *C_in, double huber_chi, double damping, int n_iter,
                           int cg_iterations, double cg_tol, void *workspace, double *C, int32_t *status, int32_t *iterations,
                           int32_t *used_edges, int32_t *skipped_edges, int32_t *failed_row, double *cost_in, double *cost,
                           double *edge_chi2, int32_t *cg_steps, void *stream);

#ifdef __cplusplus
}
#endif
#endif
