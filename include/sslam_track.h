/*
 * sslam_track.h - C ABI of libsslam_track.so: the ninth native library of the project (gfx950), feature tracks and a landmark map.
 * Every geometric stage before it is pairwise; this one records that keypoint 17 of frame 3, keypoint 40 of frame 4 and keypoint 9
 * of frame 5 are the same scene point: match lists become links, links become tracks, tracks become map points under the graphs'
 * poses - in batch, and one frame at a time inside a captured step.  Same conventions as sslam_place.h: every pointer is a
 * CALLER-OWNED DEVICE pointer, the library never allocates, frees, synchronises or reads back; `stream` is a hipStream_t passed as
 * void*; the return value is SSLAM_OK or a negative SSLAM_E_* code of sslam_hip.h; results are written with ordinary vector stores
 * and there are no floating-point atomics: every entry can be captured in a graph, and no host value that changes between frames
 * enters a step.  Index arithmetic is integer; the integer atomics are named where they are used (their results do not depend on
 * the order in which they happen).  Everything floating point is float64, built with -ffp-contract=off and the correctly rounded
 * divide and sqrt: every operation named below is rounded once, in the order written: a result is the same bits as
 * tests/track_ref.py.  The entries carry the prefix sslt_.
 */
#ifndef SSLAM_TRACK_H
#define SSLAM_TRACK_H

#include <stddef.h>
#include <stdint.h>

#include "sslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ALIGNMENT, every entry that takes device pointers: the LEAST alignment in bytes of each pointer argument - the widest access
 * the entry's kernels make to it (4 an int32 or float32 word, 8 an int64, a float64 or the workspace's (root, distance) pairs).  A
 * pointer that misses its alignment: SSLAM_E_INVALID before anything is launched, nothing written.  A result is a function of the
 * operands' values, not of their addresses (tests/test_gpu_tracks.py runs every pointer at its least alignment, just past and just
 * before a 256-byte boundary).  No entry takes a stride.  kp_bank is read a float32 at a time.
 *   sslt_link_pairs: pair_first 4, pair_second 4, matches 8, count 4, mask 4, prev 4, next 4, prev_frame 4, next_frame 4
 *   sslt_track_ids: prev 4, prev_frame 4, workspace 8, track_id 4, age 4, n_tracks 4, root_frame 4, root_slot 4, length 4
 *   sslt_landmarks: kp_bank 4, kp_depth_bank 4, C 8, next 4, next_frame 4, root_frame 4, root_slot 4, n_tracks 4, weight 4, xyz 8, n_obs 4, n_kept 4, status 4, weight_sum 8, rms 8, residual 8, kept 4
 *   sslt_track_step: t 4, next_id 4, prev 4, next 4, prev_frame 4, next_frame 4, track_id 4, age 4, matches 8, count 4, mask 4, first 4, out_track_id 4, out_age 4, n_new 4, status 4
 */

/* ---- SIZE LIMITS: the expressions the dispatch code tests, the code returned where one is false, and the widths in bits of the
 * kernels' index expressions (tests/track_table.py restates them, tests/test_tracks_cpu.py holds one past each to its code).
 *   sslt_link_pairs: K <= 4096, else SSLAM_E_UNSUPPORTED; n_bank * K <= 0x7fffffff, else SSLAM_E_UNSUPPORTED. offsets: frame * K + slot 31, (pair * n1 + slot) * 2 64
 *   sslt_track_ids: n_bank * K <= 0x7fffffff, else SSLAM_E_UNSUPPORTED. offsets: frame * K + slot 31, workspace words 64
 *   sslt_landmarks: n_bank * K <= 0x7fffffff, else SSLAM_E_UNSUPPORTED. offsets: frame * K + slot 31, (frame * K + slot) * 2 64, frame * 12 64, track * 3 64
 *   sslt_track_step: K <= 4096, else SSLAM_E_UNSUPPORTED; capacity * K <= 0x7fffffff, else SSLAM_E_UNSUPPORTED. offsets: frame * K + slot 31
 */

int sslt_version(void);
const char *sslt_arch(void);          /* "gfx950" */
long long sslt_launch_count(void);    /* kernels this library has launched in this process - a launch that returned
                                         SSLAM_E_LAUNCH is not counted (diagnostic; relaxed atomic) */

#define SSLT_MAX_K 4096
#define SSLT_SCAN_TILE 1024

/* ---- Match lists to links.
 *   pair_first, pair_second (n_pairs) int32: the frames a < b of every row, as match_pairs takes them;  matches (n_pairs, n1, 2)
 *   int64 and count (n_pairs) int32: the lists a finalize entry or sslam_match_rank wrote, rows (idx1 in frame a, idx2 in frame b),
 *   count[p] clamped to [0, n1];  mask (n_pairs, n1) int32 or NULL: where given, only slots with mask == 1 count - RANSAC's or the
 *   refinement's inlier_of_slot;  n_bank frames of K keypoint slots.
 * LINK ROW.  Row p is VALID iff 0 <= first[p] < second[p] < n_bank.  It is a LINK ROW iff it is valid, it is the lowest valid row
 *   with that `second` and it is the lowest valid row with that `first`.
 * LINK SLOT.  Slot j of a link row is VALID iff j < count (clamped), 0 <= idx1 < K, 0 <= idx2 < K (judged on the int64 values) and
 *   the mask passes.  It is a LINK iff it is valid, it is the lowest valid slot of the row naming its idx1 and the lowest valid slot
 *   naming its idx2.  Under the mutual rules (M1, M4) every valid slot is a link; under M2 and M5 the rule decides - no sequential
 *   greedy pass: a slot that loses on one side does not free its other side.
 * So every keypoint has at most one predecessor and one successor, always in an earlier and a later frame: a track is a chain in
 * ascending frame order.  Frames need not be consecutive: a row (3, 5) bridges a dropped frame.
 * Outputs, EVERY element written, -1 meaning none:
 *   prev, next (n_bank, K) int32: for a link (idx1, idx2) of the link row (a, b): next[a][idx1] = idx2, prev[b][idx2] = idx1;
 *   prev_frame, next_frame (n_bank) int32: for a link row (a, b): next_frame[a] = b, prev_frame[b] = a.
 * Launches: five, on `stream`.  (a) fill: prev, next -1; prev_frame, next_frame INT32_MAX.  (b) a thread per row: integer atomicMin
 * of the row index into prev_frame[second] and next_frame[first] of a valid row.  (c) a 256-thread workgroup per row; a row that is
 * no link row leaves at once; lowest slots by integer atomicMin in LDS (two arrays of K words, 32 KB at K = 4096), then the links'
 * stores.  (d) a thread per frame: prev_frame from a row index to a frame, -1 unless that row is a link row.  (e) the same for
 * next_frame: the lowest row r naming f first is a link row iff prev_frame[second[r]], as (d) left it, is f.
 * SSLAM_E_INVALID: a NULL pointer (mask apart); n_pairs, n1, n_bank or K <= 0; a pointer that misses its alignment.
 * SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
int sslt_link_pairs(const int32_t *pair_first, const int32_t *pair_second, int n_pairs, const int64_t *matches, const int32_t *count,
                    const int32_t *mask, int n1, int n_bank, int K, int32_t *prev, int32_t *next, int32_t *prev_frame,
                    int32_t *next_frame, void *stream);

/* ---- Links to tracks.  Node (f, s) is keypoint slot s of frame f, n = f * K + s.  It HAS A PREDECESSOR iff 0 <= prev_frame[f] < f and
 * 0 <= prev[f][s] < K: the node (prev_frame[f], prev[f][s]); anything else reads as none, so any input ends.  A ROOT has none.
 * Every node belongs to exactly one track, its root's; a keypoint with no link is a track of length 1.
 * NUMBERING.  Roots are numbered 0, 1, ... in ascending (frame, slot) order - the order an online stepper meets them in.
 * Outputs, every element written:
 *   track_id (n_bank, K) int32: the number of the node's root;   age (n_bank, K) int32: the number of predecessors up to the root;
 *   n_tracks (1) int32;   root_frame, root_slot, length (n_bank * K) int32: row i < n_tracks the root's frame and slot and the
 *   number of nodes of track i; rows past n_tracks are -1, -1, 0.
 * METHOD.  Pointer jumping over double-buffered (root, distance) int32 pairs in the workspace, ceil(log2 n_bank) rounds: the round
 * count comes from the host scalar n_bank (a chain has at most n_bank - 1 hops), so the sequence of launches is fixed.  The numbering
 * is a device-wide exclusive scan of the root flags: per tile of SSLT_SCAN_TILE nodes a count, one workgroup scans the tile counts,
 * per tile a local scan.  length is an integer atomicAdd of 1 per node.  Launches: 5 + ceil(log2 n_bank), a thread per node but for
 * the tile scans.
 * workspace: sslt_track_workspace_bytes(n_bank, K) bytes = 20 * n_bank * K + 4 * ceil(n_bank * K / SSLT_SCAN_TILE); nothing is
 * expected in it and nothing useful left in it.
 * SSLAM_E_INVALID: a NULL pointer; n_bank or K <= 0; a pointer that misses its alignment.  SSLAM_E_UNSUPPORTED: SIZE LIMITS above.
 * Every refusal comes before anything is launched and writes nothing. */
size_t sslt_track_workspace_bytes(int n_bank, int K);      /* 0 for arguments the entry refuses */
int sslt_track_ids(const int32_t *prev, const int32_t *prev_frame, int n_bank, int K, void *workspace, int32_t *track_id, int32_t *age,
                   int32_t *n_tracks, int32_t *root_frame, int32_t *root_slot, int32_t *length, void *stream);

/* ---- Tracks to map points.
 *   kp_bank (n_bank, K, 2) fp32, kp_depth_bank (n_bank, K) int32: as sslam_pose_refine_pairs takes them;  C (n_bank, 12) float64:
 *   world -> camera [R | t] row-major of every frame, the graphs' C;  fx .. view_h: the camera scalars of sslam_pose_refine_pairs
 *   (view_w and view_h are checked and otherwise take no part);  threshold in keypoint units;  min_obs >= 2;
 *   next (n_bank, K), next_frame (n_bank): sslt_link_pairs';  root_frame, root_slot (n_bank * K), n_tracks (1): sslt_track_ids';
 *   weight (n_bank, K) fp32 or NULL: NULL means 1 for every keypoint.
 * MEMBERS of track i < n_tracks (n_tracks clamped to [0, n_bank * K]): the root (root_frame[i], root_slot[i]) if 0 <= frame < n_bank
 *   and 0 <= slot < K, then from member (f, s) the member (next_frame[f], next[f][s]) while f < next_frame[f] < n_bank and
 *   0 <= next[f][s] < K: ascending frames, so any input ends.
 * OBSERVATION.  A member is an observation iff its raw depth d is > 0, all 12 entries of its frame's C row are finite, and its
 *   weight g (as a double; 1.0 under NULL) satisfies g > 0 && g - g == 0, the weighted refinement's own rule.
 * CAMERA AND WORLD POINT of an observation (x, y), the back-projection of sslam_pose_ransac_pairs:
 *     u = x*scale_x, v = y*scale_y, z = d / depth_scale;  X = ((u - cx) * z) / fx, Y = ((v - cy) * z) / fy, Z = z;
 *     ex = X - t0, ey = Y - t1, ez = Z - t2;   Xw_j = (r0j * ex + r1j * ey) + r2j * ez   (j = 0, 1, 2):   Xw = R^T (Xc - t).
 * SCORE of a point L in an observation's frame, that entry's formulas:
 *     X' = ((r00*L0 + r01*L1) + r02*L2) + t0, Y' and Z' likewise;  u' = (fx * X') / Z' + cx, v' = (fy * Y') / Z' + cy;
 *     dx = u' / scale_x - x, dy = v' / scale_y - y;   s = dx*dx + dy*dy if Z' > 0, else +inf (a NaN Z' included).
 * PASSES.  Every sum runs over the track's members in ascending frame order from +0.0, a member that does not take part adding nothing.
 *   1. W0 = sum g, S0_j = sum g * Xw_j over the observations;  L0_j = S0_j / W0.
 *   2. An observation is KEPT iff sqrt(s) < threshold for s the SCORE of L0 (a NaN fails).  W = sum g, S_j = sum g * Xw_j over the kept.
 *      With n_kept >= min_obs: L_j = S_j / W, status 0.  Otherwise L = L0, status 1.  A track with no observation: L = +0.0, status 2,
 *      and nothing below but zeros.
 *   3. residual of an observation = sqrt(s) for s the SCORE of L - not of L0;  rms = sqrt((sum s over the kept) / n_kept), 0 without.
 * Outputs per track, (n_bank * K) rows, every element written; a row past n_tracks is zeros with status -1:
 *   xyz (3) float64: L;   n_obs, n_kept, status int32;   weight_sum float64: W of pass 2;   rms float64.
 * Outputs per keypoint, every element written:
 *   residual (n_bank, K) float64: -1 where the keypoint is not an observation (or no member of any track, under foreign links);
 *   kept (n_bank, K) int32: 1 or 0.
 * With weight NULL and with a bank of exactly 1.0f the outputs are the same bytes.  Scaling every weight by a power of two (no
 * overflow, no underflow) scales weight_sum exactly and leaves every other output's bytes.
 * Launches: two.  (a) fill: residual -1, kept 0.  (b) ONE THREAD PER TRACK walks its chain three times: a track's result is a
 * function of its own members alone and its sums have one order.  The trade-off as measured (tools/track_probe.py): the
 * launch costs what its LONGEST track's three serial walks cost, not the sum of the work - over the same 306 500 keypoints it takes
 * about nine times as long with a longest track of 92 members as with none longer than 8.  A wave per track would walk once and run
 * the second and third pass across its lanes, at the price of idle lanes on the median track of 7 members; it is not built.
 * SSLAM_E_INVALID: a NULL pointer (weight apart); n_bank or K <= 0; min_obs < 2; a threshold that is negative, NaN or infinite; fx,
 * fy, depth_scale, scale_x, scale_y, view_w or view_h not finite and positive; cx or cy not finite; a pointer that misses its
 * alignment.  SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
int sslt_landmarks(const float *kp_bank, const int32_t *kp_depth_bank, const double *C, int n_bank, int K, double fx, double fy,
                   double cx, double cy, double depth_scale, double scale_x, double scale_y, double view_w, double view_h,
                   double threshold, const int32_t *next, const int32_t *next_frame, const int32_t *root_frame, const int32_t *root_slot,
                   const int32_t *n_tracks, const float *weight, int min_obs, double *xyz, int32_t *n_obs, int32_t *n_kept,
                   int32_t *status, double *weight_sum, double *rms, double *residual, int32_t *kept, void *stream);

/* ---- Online: one frame of a growing track bank, inside a captured step.
 * PERSISTENT STATE, the caller's, a bank of `capacity` frames:
 *   t, next_id (1) int32 each: the frames stepped and the tracks numbered so far;
 *   prev, next, track_id, age (capacity, K) int32;   prev_frame, next_frame (capacity) int32.
 *   A fresh state is t = 0, next_id = 0; the rows of the frames 0 .. t - 1 are written, nothing past them is read by the step.
 * STEP INPUTS, this step's link row, all device memory - no host value enters the step:
 *   matches (n1, 2) int64, count (1) int32, mask (n1) int32 or NULL: one row of sslt_link_pairs' operands;
 *   first (1) int32: the bank frame the row's first member names, -1 for none.
 * THE STEP, t and next_id as read.  One 256-thread workgroup, K <= SSLT_MAX_K:
 * 0. COUNTER.  t outside 0 .. capacity - 1: status = 4, out_track_id and out_age all -1, n_new 0, and the STATE IS UNTOUCHED.
 * 1. The row (a, t), a = first[0], is a LINK ROW iff 0 <= a < t and next_frame[a] == -1 (no earlier step linked to a: the lowest
 *    row with that `first`; it is the only row with this `second`).  Its links: the LINK SLOT rule of sslt_link_pairs.
 * 2. Row t of the state: prev[t][s] = idx1 of the link naming s, else -1;  next[t] = -1;  prev_frame[t] = a for a link row, else -1;
 *    next_frame[t] = -1;  and for a link row next_frame[a] = t, next[a][idx1] = idx2 for every link.
 * 3. A slot with a predecessor p takes track_id[a][p] and age[a][p] + 1.  The others take next_id, next_id + 1, ... in slot order
 *    (a workgroup scan) and age 0;  n_new counts them.
 * 4. t <- t + 1, next_id <- next_id + n_new.
 * Outputs: out_track_id, out_age (K) int32: row t as written;   n_new (1), status (1) int32: 0, or 4.
 * THE CONTRACT: after n steps the rows 0 .. n - 1 of prev, next, prev_frame, next_frame equal sslt_link_pairs over the rows
 * (first_i, i) stepped so far, and those of track_id and age equal sslt_track_ids over them, bit for bit, next_id being n_tracks.
 * Launch: one kernel; three LDS arrays of K words (48 KB at K = 4096).
 * SSLAM_E_INVALID: a NULL pointer (mask apart); n1, K or capacity <= 0; a pointer that misses its alignment.
 * SSLAM_E_UNSUPPORTED: SIZE LIMITS above.  Every refusal comes before anything is launched and writes nothing. */
int sslt_track_step(int32_t *t, int32_t *next_id, int32_t *prev, int32_t *next, int32_t *prev_frame, int32_t *next_frame,
                    int32_t *track_id, int32_t *age, const int64_t *matches, const int32_t *count, const int32_t *mask,
                    const int32_t *first, int n1, int K, int capacity, int32_t *out_track_id, int32_t *out_age, int32_t *n_new,
                    int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
