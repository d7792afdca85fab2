/*
 * sslam_place.h - C ABI of libsslam_place.so: the sixth native library of the project (gfx950), loop closures WHILE the sequence
 * runs - a place bank that grows by one frame per step and answers, inside the step, which older frames this one resembles; and an
 * append-only log of the step's verified edges, which ssll_pose_graph_sparse (sslam_loop.h) reads whenever the caller asks for a
 * corrected trajectory.  Same conventions as sslam_loop.h: every pointer is a CALLER-OWNED DEVICE pointer, the library never
 * allocates, frees, synchronises or reads back; `stream` is a hipStream_t passed as void*; the return value is SSLAM_OK or a
 * negative SSLAM_E_* code of sslam_hip.h; results are written with ordinary vector stores and there are no floating-point atomics:
 * every entry can be captured in a graph, and no host value that changes between frames enters a step - the frame counters are
 * device memory.  Built with -ffp-contract=off: every operation named below is rounded once, in the order written, and a fused
 * multiply-add happens exactly where fmaf is written: a result is the same bits as tests/place_ref.py.  The entries carry the
 * prefix sslp_.
 */
#ifndef SSLAM_PLACE_H
#define SSLAM_PLACE_H

#include <stddef.h>
#include <stdint.h>

#include "sslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ALIGNMENT, every entry that takes device pointers: the LEAST alignment in bytes of each pointer argument - the widest access
 * the entry's kernels make to it (4 an int32 or float32 word, 8 a float64).  A pointer that misses its alignment:
 * SSLAM_E_INVALID before anything is launched, nothing written.  A result is a function of the operands' values, not of their
 * addresses (tests/test_gpu_place.py runs every pointer at its least alignment, just past and just before a 256-byte boundary).
 * No entry takes a stride.
 *   sslp_place_step: t 4, raw 4, sum 4, desc 4, scores 4, workspace 4, first 4, second 4, sim 4, count 4, status 4, sig 4
 *   sslp_edge_log_step: t 4, log_first 4, log_second 4, log_T 8, log_info 8, slot_first 4, new_T 8, new_info 8, new_status 4, new_inliers 4, logged 4, status 4
 */

/* ---- SIZE LIMITS: the expressions the dispatch code tests, the code returned where one is false, and the widths in bits of the
 * kernels' index expressions (tests/place_table.py restates them, tests/test_place_cpu.py holds one past each to its code).
 *   sslp_place_step: capacity <= 4096, else SSLAM_E_UNSUPPORTED; k <= 4096, else SSLAM_E_UNSUPPORTED; d == 128 or d == 256, else SSLAM_E_UNSUPPORTED; per_frame <= 8, else SSLAM_E_UNSUPPORTED. offsets: frame * d 31, keypoint * d 31
 *   sslp_edge_log_step: n_slots <= 16, else SSLAM_E_UNSUPPORTED; capacity <= 0x7fffffffffffffff / 168 / n_slots, else SSLAM_E_UNSUPPORTED. offsets: (frame * n_slots + slot) * 21 64
 */

int sslp_version(void);
const char *sslp_arch(void);          /* "gfx950" */
long long sslp_launch_count(void);    /* kernels this library has launched in this process - a launch that returned
                                         SSLAM_E_LAUNCH is not counted (diagnostic; relaxed atomic) */

#define SSLP_MAX_CAPACITY 4096
#define SSLP_MAX_K 4096
#define SSLP_MAX_PER_FRAME 8
#define SSLP_MAX_SLOTS 16
#define SSLP_FRAMES_PER_GROUP 32

/* ---- One frame of a growing place bank: this frame's signature, and the most similar OLDER frames in match_pairs' pair-list form.
 * PERSISTENT STATE, the caller's, read and written by every step:
 *   t (1) int32                 the frames stepped so far: this step's frame index;
 *   raw (capacity, d) float32   the raw sums of the frames 0 .. t - 1;        sum (d) float32   their column sums.
 *   A fresh state is t = 0; nothing else of it is read before it is written.
 * STEP INPUTS: desc (k, d) float32 and scores (k) float32 of this frame, as the extraction returns them, d = 128 or 256.
 * SCALARS: capacity 1 .. SSLP_MAX_CAPACITY;  k 1 .. SSLP_MAX_K;  min_gap >= 1;  min_sim finite;  per_frame 1 .. SSLP_MAX_PER_FRAME;
 *   suppress >= 0;  workspace: sslp_place_workspace_bytes(capacity) bytes (capacity float32: this step's similarities); nothing is
 *   expected in it and nothing useful left in it.
 * THE STEP, t the counter as read.  The arithmetic is sslam_loop.h's, by its names:
 * 0. COUNTER.  t outside 0 .. capacity - 1: status = 4, first and second all -1, sim all +0.0, count 0, sig all +0.0, and the
 *    STATE IS UNTOUCHED: a pair list built from first / second reads "absent" also when the bank is full.
 * 1. raw[t][c] = ssll_frame_signatures' raw_i[c] of this frame: acc = +0.0f; for kk = 0 .. k-1 ascending: acc = fmaf(scores[kk],
 *    desc[kk][c], acc).   Then  sum[c] = (t == 0 ? +0.0f : sum[c]) + raw[t][c]   (one float32 add).
 * 2. mean[c] = sum[c] / (float)(t + 1): the bits of ssll_frame_signatures' mean over the frames 0 .. t, whose sum is formed in
 *    the same order.  For j = t and every j <= t - min_gap:  c_j[c] = raw[j][c] - mean[c];  ss_j = the sum of c_j[c] * c_j[c] in
 *    that entry's order (thread c of d holds its product; lanes of each wave of 64 by xor 32, 16, 8, 4, 2, 1; then the waves
 *    ascending, (w0 + w1) at d = 128, ((w0 + w1) + w2) + w3 at d = 256);  sig_j[c] = c_j[c] / fmaxf(sqrtf(ss_j), 1e-12f).
 * 3. S_tj = ssll_loop_candidates' ONE chain: acc = +0.0f; for c = 0 .. d-1 ascending: acc = fmaf(sig_t[c], sig_j[c], acc).
 *    The picks are that entry's rule for the row i = t: frame j is ELIGIBLE iff 0 <= j <= t - min_gap and S_tj >= min_sim (a NaN
 *    is not); up to per_frame times: the eligible frame of greatest S_tj, of equal values (as == compares) the lowest j; then
 *    every j' with |j' - j| <= suppress stops being eligible.
 * 4. t <- t + 1.
 * Outputs (every element is written, nothing else is outside state and workspace):
 *     first, second (per_frame) int32   slot s: the older frame j of the s-th pick and t - GLOBAL frame indices; -1, -1 in an empty slot;
 *     sim (per_frame) float32           S_tj; +0.0 in an empty slot;       count (1) int32   the filled slots, which come first;
 *     status (1) int32                  0, or 4: the counter was out of range;
 *     sig (d) float32                   sig_t AS OF THIS STEP (a later step centres the frame on a later mean).
 * THE CONTRACT: first / second / sim / count of step t are row t of ssll_loop_candidates over ssll_frame_signatures of the frames
 * 0 .. t, bit for bit, and sig is row t of those signatures (tests/test_gpu_place.py runs both on the device).
 * Launches: three, on `stream`; no workgroup waits for another.  (a) one workgroup of d threads: raw[t] and sum.  (b) one workgroup
 * of d threads per SSLP_FRAMES_PER_GROUP bank frames, the grid fixed by capacity; a group wholly past t - min_gap leaves at once
 * (group 0 stays and writes sig); each forms the mean and sig_t anew, its frames' signatures go to LDS (a row every d + 1 words,
 * 33 KB at d = 256), thread f of the first 32 runs frame f's chain and writes S_tj to the workspace, -inf where it is below
 * min_sim or a NaN.  (c) one 256-thread workgroup: the similarities into LDS (16 KB at capacity 4096), ssll_loop_candidates'
 * block-wide arg-max picks, the outputs, the counter.
 * SSLAM_E_INVALID: a NULL pointer; capacity, k or d <= 0; min_gap < 1; per_frame < 1; suppress < 0; min_sim not finite; a pointer that
 * misses its alignment.  SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
size_t sslp_place_workspace_bytes(int capacity);      /* 0 for arguments the entry refuses */
int sslp_place_step(int32_t *t, float *raw, float *sum, const float *desc, const float *scores, int capacity, int k, int d, int min_gap,
                    float min_sim, int per_frame, int suppress, void *workspace, int32_t *first, int32_t *second, float *sim,
                    int32_t *count, int32_t *status, float *sig, void *stream);

/* ---- The append-only edge list ssll_pose_graph_sparse will read: one frame's E = n_slots (1 .. SSLP_MAX_SLOTS) pairs.
 * PERSISTENT STATE, the caller's:
 *   t (1) int32                                        the frames logged so far - a counter of its own;
 *   log_first, log_second (capacity * E) int32         GLOBAL frame indices a, b of every slot; log_first -1: an absent slot;
 *   log_T (capacity * E, 12), log_info (capacity * E, 21) float64   the slots' measured poses and information, as edge_T, edge_info.
 *   A fresh state is t = 0; the rows of the frames 0 .. t - 1 are written, nothing past them is read by the step.
 * STEP INPUTS, as sslam_pose_refine_pairs wrote them for this frame's E pairs:
 *   slot_first (E) int32: the GLOBAL index of each slot's older frame, -1 for none;   new_T (E, 12);   new_info (E, 21);
 *   new_status, new_inliers (E) int32: that entry's status and inlier_count.
 * SCALARS: n_odometry 0 .. E: the slots before it are odometry pairs, the others loop candidates;  min_inliers >= 0;
 *   loop_min_inliers >= 0;  capacity >= 1.
 * THE STEP, t the counter as read:
 * 0. COUNTER.  t outside 0 .. capacity - 1: status = 4, logged all 0, and NOTHING else is written, state included.
 * 1. Slot e, with m = min_inliers if e < n_odometry else loop_min_inliers, is LOGGED iff  0 <= slot_first[e] < t,
 *    new_status[e] != 3,  new_inliers[e] >= m,  and all 33 numbers of new_T[e] and new_info[e] are finite.
 *    Row t * E + e takes (slot_first[e], t, new_T[e], new_info[e]) when logged, else first -1, second t and +0.0 in all 33 words:
 *    the state is a function of the inputs alone.
 * 2. t <- t + 1.
 * Outputs: logged (E) int32: 1 or 0;   status (1) int32: 0, or 4.
 * For e < n_odometry and slot_first[e] = t - s with a spacing s below the window, logged[e] equals sslw_window_step's admitted[e]
 * (sslam_window.h, ADMISSION) at the same min_inliers: the same four tests, base <= a being implied by s < W.
 * The first n * E rows are the operands edge_first, edge_second, edge_T, edge_info of ssll_pose_graph_sparse over the n frames logged.
 * Launch: one kernel, one workgroup of 64 * E threads, one wave per slot: lane l < 33 holds word l of the slot's 33, a wave vote
 * decides, lanes 0 .. 35 write one word each; row offsets are 64-bit.
 * SSLAM_E_INVALID: a NULL pointer; n_slots or capacity <= 0; n_odometry outside 0 .. n_slots; min_inliers or loop_min_inliers < 0; a
 * pointer that misses its alignment.  SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and
 * writes nothing. */
int sslp_edge_log_step(int32_t *t, int32_t *log_first, int32_t *log_second, double *log_T, double *log_info, const int32_t *slot_first,
                       const double *new_T, const double *new_info, const int32_t *new_status, const int32_t *new_inliers, int n_slots,
                       int n_odometry, int min_inliers, int loop_min_inliers, long long capacity, int32_t *logged, int32_t *status,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif
