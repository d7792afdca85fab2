/*
 * sslam_window.h - C ABI of libsslam_window.so: the fifth native library of the project (gfx950), the ONLINE estimator over the
 * relative poses and information matrices that libsslam_hip.so (sslam_hip.h: sslam_pose_refine_pairs) writes for the S pairs of one
 * frame of a multi-spacing step: a ring of the last `window` frames' edges and poses, and one Gauss-Newton solve over them per
 * frame.  Same conventions as sslam_graph.h: every pointer is a CALLER-OWNED DEVICE pointer, the library never allocates, frees,
 * synchronises or reads back; `stream` is a hipStream_t passed as void*; the return value is SSLAM_OK or a negative SSLAM_E_* code
 * of sslam_hip.h; results are written with ordinary vector stores, there are no atomics: the entry can be captured in a graph, and
 * no host value that changes between frames enters it - the frame counter is device memory.  All floating point is IEEE float64,
 * + - * / sqrt only, every operation rounded once, in the order written (built with -ffp-contract=off): a result is the same bits
 * as tests/window_ref.py.  The entries carry the prefix sslw_.
 */
#ifndef SSLAM_WINDOW_H
#define SSLAM_WINDOW_H

#include <stddef.h>
#include <stdint.h>

#include "sslam_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ALIGNMENT, every entry that takes device pointers: the LEAST alignment in bytes of each pointer argument - the widest access
 * the entry's kernel makes to it (4 an int32 word, 8 a float64).  A pointer that misses its alignment: SSLAM_E_INVALID before
 * anything is launched, nothing written.  A result is a function of the operands' values, not of their addresses
 * (tests/test_gpu_window.py runs every pointer at its least alignment, just past and just before a 256-byte boundary).
 * No entry takes a stride.
 *   sslw_window_step: t 4, ring_first 4, ring_second 4, ring_T 8, ring_info 8, ring_C 8, trajectory 8, spacings 4, new_T 8, new_info 8, new_status 4, new_inliers 4, C_start 8, workspace 8, C_window 8, base 4, n_nodes 4, admitted 4, predicted_from 4, lost 4, status 4, iterations 4, used_edges 4, dropped_edges 4, failed_row 4, cost_in 8, cost 8, edge_chi2 8
 */

/* ---- SIZE LIMITS: the expressions the dispatch code tests, the code returned where one is false, and the widths in bits of the
 * kernel's index expressions (tests/window_table.py restates them, tests/test_window_cpu.py holds one past each to its code).
 *   sslw_window_step: window <= 32, else SSLAM_E_UNSUPPORTED; n_spacings <= 8, else SSLAM_E_UNSUPPORTED; n_windows <= 65535, else SSLAM_E_UNSUPPORTED; capacity <= 0x7fffffffffffffff / 96 / n_windows, else SSLAM_E_UNSUPPORTED. offsets: window * capacity * 12 64, window * workspace doubles 64, frame * 12 64, row * (row + 1) / 2 31
 */

int sslw_version(void);
const char *sslw_arch(void);          /* "gfx950" */
long long sslw_launch_count(void);    /* kernels this library has launched in this process - a launch that returned
                                         SSLAM_E_LAUNCH is not counted (diagnostic; relaxed atomic) */

#define SSLW_MAX_WINDOW 32
#define SSLW_MAX_SPACINGS 8
#define SSLW_MAX_WINDOWS 65535
#define SSLW_MAX_FRAME 2147483646      /* the largest frame counter a step takes: 2^31 - 2 */

/* ---- One frame of n_windows independent sliding windows: one launch, one 256-thread workgroup per window.  W = window (2 ..
 * SSLW_MAX_WINDOW), S = n_spacings (1 .. SSLW_MAX_SPACINGS).  Poses, `o`, inv(), edges, the cost, the normal equations, the solve,
 * the update, the iteration and the status codes 0 .. 3 are sslam_graph.h's, word for word; this header states what surrounds them.
 *
 * PERSISTENT STATE, the caller's, read and written by every step (leading axis n_windows on every array):
 *   t (n_windows) int32                     the frames stepped so far: this step's frame index;
 *   ring_first, ring_second (n_windows, W * S) int32   GLOBAL frame indices a, b of every edge slot; ring_first -1: an absent slot;
 *   ring_T (n_windows, W * S, 12), ring_info (n_windows, W * S, 21)   the slots' measured poses and information, as edge_T, edge_info;
 *   ring_C (n_windows, W, 12)               world -> camera pose of frame j at row j mod W, for the frames of the window;
 *   trajectory (n_windows, capacity, 12)    the last pose every frame j < capacity took while it was in the window.
 *   A fresh state is t = 0 and ring_first = -1 everywhere; nothing else of it is read before it is written.
 * STEP INPUTS, as sslam_pose_refine_pairs wrote them for this frame's S pairs (k = 0 .. S - 1, pair k = frames t - spacings[k], t):
 *   spacings (S) int32, shared by the windows;   new_T (n_windows, S, 12);   new_info (n_windows, S, 21);
 *   new_status, new_inliers (n_windows, S) int32: that entry's status and inlier_count;
 *   C_start (n_windows, 12) or NULL: the pose of frame 0, [I | 0] if NULL; read at t = 0 only.
 * SCALARS: min_inliers >= 0;  huber_chi finite, > 0;  damping finite, >= 0;  n_iter 0 .. SSLG_GRAPH_MAX_ITER;  capacity >= 1;
 *   workspace: sslw_window_workspace_bytes(n_windows, window, n_spacings) bytes, 8-byte aligned; nothing is expected in it and
 *   nothing useful left in it.
 *
 * THE STEP of one window, t its counter as read:
 * 0. COUNTER.  t outside 0 .. SSLW_MAX_FRAME: status = 4 is written and NOTHING else, state included.
 * 1. WINDOW.  base = max(0, t - W + 1); the nodes are the frames base .. t, frame j the local node j - base; n_nodes = t - base + 1.
 * 2. ADMISSION of k, with a = t - spacings[k] (64-bit):  admitted[k] = 1 iff  base <= a < t,  new_status[k] != 3,
 *    new_inliers[k] >= min_inliers, and all 33 numbers of new_T[k] and new_info[k] are finite;  else 0.
 *    Ring slot (t mod W) * S + k takes (a, t, new_T[k], new_info[k]) when admitted, else first -1, second t and +0.0 in all 33
 *    words: the state is a function of the inputs alone.  (The slots of row t mod W held the edges that END at frame t - W, which
 *    has left the window.)
 * 3. PREDICTION.  t = 0: C_0 = C_start bit for bit, predicted_from = -1, lost = 0.  Otherwise, with k* the admitted k of the
 *    smallest spacing (the lowest k among equals):  C_t = new_T[k*] o C_{t - spacings[k*]},  predicted_from = k*, lost = 0;  with
 *    no k admitted  C_t = C_{t-1} bit for bit, predicted_from = -1, lost = 1.  C_j is ring_C's row j mod W.
 * 4. SOLVE.  sslg_pose_graph's statement on one graph of n_nodes nodes and W * S edge slots in ascending slot order, band = W - 1:
 *    slot e has the local nodes  (-1, ring_second - base)  where ring_first is -1,  (-2, ring_second - base)  where ring_first <
 *    base (a DROPPED slot: its first frame has left the window; it is not used and dropped_edges counts it as sslg_pose_graph
 *    counts skipped_edges),  else (ring_first - base, ring_second - base);  edge_T = ring_T, edge_info = ring_info;  C_in = the
 *    window's poses C_base .. C_t with the prediction in its last row;  huber_chi, damping, n_iter as given.  Node 0, the OLDEST
 *    frame of the window, is the anchor: it stays at its current estimate (conditioning, not marginalisation).  At band W - 1 the
 *    banded LDL^T is the plain dense one: n = 6 * (n_nodes - 1) <= 6 * W - 6 < bw = 6 * W - 1.  With one node, no used edge or a
 *    non-finite pose the status is 3 as there, and the poses are C_in's.
 * 5. WRITE-BACK.  The solve's C goes to ring_C (frame j to row j mod W) and to trajectory[j] for every window frame j < capacity;
 *    a frame that left the window keeps its last value.  Then t <- t + 1.
 * Outputs per window (every element is written - except under status 4 - and nothing else is, outside state and workspace):
 *     C_window (n_windows, W, 12)         the solve's C in node order; rows past n_nodes +0.0;
 *     base, n_nodes (n_windows) int32;    admitted (n_windows, S) int32;    predicted_from, lost (n_windows) int32;
 *     status (n_windows) int32            sslg_pose_graph's 0 .. 3, or 4: the counter was out of range;
 *     iterations, used_edges, dropped_edges, failed_row (n_windows) int32;    cost_in, cost (n_windows) float64;
 *     edge_chi2 (n_windows, W * S)        s of every used slot at C, +0.0 for every other slot;   all as sslg_pose_graph states them.
 *   A window's outputs and next state are a function of that window's state, its inputs and the scalars alone.
 * WHERE THINGS LIVE.  LDS, n = 6 * (W - 1): the whole lower triangle of A by rows, entry (i, j) at i * (i + 1) / 2 + j, overwritten
 *   by the factor (D on the diagonal, L below), then g, y and delta: n * (n + 1) / 2 + 3 * n words - 143 592 bytes at W = 32, 60 960
 *   at W = 21 - beside 2 KB for the staged edges' nodes and the wave partial sums.  A call that needs more than 60 KB (W >= 22) first
 *   raises the kernel's LDS allowance, always to the largest window's 143 592 bytes, so the value does not depend on the caller; it
 *   is a host call, no stream operation, and is made inside a capture too (tests/test_gpu_window.py captures at W = 24).  Assembly is sslg_pose_graph's (one staging pass:
 *   W * S <= 256 slots), the factorisation right-looking in place - every element takes its updates in ascending k, so the bits
 *   are the statement's -, the forward substitution rides along, the backward substitution runs by rows in one wave.  Nothing of
 *   the solve goes through global memory but the staged terms.  Workspace, per window, in float64 words: C_in and the trial
 *   poses, 24 * W; the staged terms, 256 * 90; the local nodes of the slots, W * S (two int32 each).
 * SSLAM_E_INVALID: a NULL pointer other than C_start; n_windows, n_spacings or capacity <= 0; window < 2; min_inliers < 0; huber_chi
 * not finite and > 0; damping not finite and >= 0; n_iter outside 0 .. SSLG_GRAPH_MAX_ITER; a pointer that misses its alignment.
 * SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
size_t sslw_window_workspace_bytes(int n_windows, int window, int n_spacings);      /* 0 for arguments the entry refuses */
int sslw_window_step(int32_t *t, int32_t *ring_first, int32_t *ring_second, double *ring_T, double *ring_info, double *ring_C,
                     double *trajectory, const int32_t *spacings, const double *new_T, const double *new_info, const int32_t *new_status,
                     const int32_t *new_inliers, const double *C_start, int n_windows, int window, int n_spacings, int min_inliers,
                     double huber_chi, double damping, int n_iter, long long capacity, void *workspace, double *C_window, int32_t *base,
                     int32_t *n_nodes, int32_t *admitted, int32_t *predicted_from, int32_t *lost, int32_t *status, int32_t *iterations,
                     int32_t *used_edges, int32_t *dropped_edges, int32_t *failed_row, double *cost_in, double *cost, double *edge_chi2,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif
