/*
 * sslam_ext.h - C ABI of libsslam_ext.so: the second native library of the project (gfx950), for stages that refine what
 * libsslam_hip.so (sslam_hip.h) produced.  Same conventions as there: every pointer is a CALLER-OWNED DEVICE pointer, the library
 * never allocates, frees, synchronises or reads back; `stream` is a hipStream_t passed as void*; the return value is SSLAM_OK or a
 * negative SSLAM_E_* code of sslam_hip.h; all floating point is IEEE fp32, every operation named below rounded once, in the order
 * written (built with -ffp-contract=off and the correctly rounded divide), so a result is the same bits as tests/subcell_ref.py.
 * The entries carry the prefix sslx_.
 */
#ifndef SSLAM_EXT_H
#define SSLAM_EXT_H

#include <stdint.h>

#include "sslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ALIGNMENT, every entry that takes device pointers: the LEAST alignment in bytes of each pointer argument - the widest access
 * the entry's kernel makes to it (4 an fp32 or int32 word, 8 an (x, y) pair stored as one).  A pointer that misses its alignment:
 * SSLAM_E_INVALID before anything is launched, nothing written.  A result is a function of the operands' values, not of their
 * addresses (tests/test_gpu_subcell.py runs every pointer at its least alignment, just past and just before a 256-byte boundary).
 * No entry takes a stride.
 *   sslx_subcell_keypoints: sal 4, idx 4, kp_xy_sub 8, kp_pixel_sub 8, flags 4
 */

int sslx_version(void);
const char *sslx_arch(void);          /* "gfx950" */
long long sslx_launch_count(void);    /* kernels this library has launched in this process - a launch that returned
                                         SSLAM_E_LAUNCH is not counted (diagnostic; relaxed atomic) */

#define SSLX_SUBCELL_MAX_CELLS 4096   /* G * G of a frame */
#define SSLX_SUBCELL_MAX_K 4096
#define SSLX_FLAG_X 1                 /* flags bit 0: x refined */
#define SSLX_FLAG_Y 2                 /* flags bit 1: y refined */
#define SSLX_FLAG_RANGE 4             /* flags bit 2: idx outside [0, G*G) */

/* Sub-cell keypoint localisation: each keypoint of sslam_select_keypoints moved from its cell to the vertex of the parabola through
 * the saliency of the cell and of its two neighbours, per axis (separable three-point fit).
 *   sal (n_frames, G, G) fp32, the map the keypoints were selected from; idx (n_frames, K) int32 flat cells as
 *   sslam_select_keypoints writes them: x = idx % G, y = idx / G.
 * Per keypoint, per axis (x: neighbours (x - 1, y) and (x + 1, y); y: (x, y - 1) and (x, y + 1)), with c the cell's value, m the
 * lower and p the upper neighbour's, all fp32, each operation rounded once:
 *   the offset is +0.0f and the axis is NOT refined when
 *     - the cell lies on that axis' border (coordinate 0 or G - 1; so always at G <= 2), the neighbours are then not used; or
 *     - a = c - m, b = c - p, and (a >= 0 && b >= 0) is false (the cell is no maximum along the axis; a NaN fails); or
 *     - den = a + b, and (den > 0) is false (a plateau; a NaN fails);
 *   otherwise off = (a - b) / (den + den), kept - and the axis refined - only if (off >= -0.5f && off <= 0.5f), else +0.0f
 *   and not refined.  For finite inputs |a - b| <= a + b survives rounding, so the last test only catches infinities (NaN off).
 * Outputs:
 *   kp_xy_sub (n_frames, K, 2) fp32 = ((float)x + offx, (float)y + offy), patch units as keypoints_patch;
 *   kp_pixel_sub (n_frames, K, 2) fp32 = kp_xy_sub * 16.0f + 8.0f, the product rounded, then the sum;
 *   flags (n_frames, K) int32: SSLX_FLAG_X | SSLX_FLAG_Y as refined; SSLX_FLAG_RANGE alone for an idx outside [0, G*G): nothing
 *   of sal is read for it, kp_xy_sub = (+0.0f, +0.0f) and kp_pixel_sub = (8.0f, 8.0f) by the same formula.
 * Every element of the three outputs is written; nothing else is.
 * Launch: one kernel, one thread per keypoint, 256-thread workgroups; the five saliency loads of a keypoint are issued before any
 * is used; each (x, y) pair is one 8-byte store.  No LDS, no atomics, no workspace: capturable in a graph.
 * SSLAM_E_INVALID: a NULL pointer; n_frames, G or K <= 0; a pointer that misses its alignment (above).
 * SSLAM_E_UNSUPPORTED: G * G above SSLX_SUBCELL_MAX_CELLS; K above SSLX_SUBCELL_MAX_K; n_frames * K above 2^31 - 1.
 * Every refusal comes before anything is launched and writes nothing.
 * SIZE LIMITS (as the block of that name in include/sslam_hip.h: the expressions the dispatch code tests, the code returned where
 * one is false, and the widths in bits of the kernel's index expressions; tests/size_table.py, tests/test_size_limits_cpu.py):
 *   sslx_subcell_keypoints: n_frames * K <= 0x7fffffff, else SSLAM_E_UNSUPPORTED; G <= 64 and K <= 4096, else SSLAM_E_UNSUPPORTED.
 *         offsets: keypoint index n_frames * K 64, frame * G * G 64 */
int sslx_subcell_keypoints(const float *sal, int n_frames, int G, const int32_t *idx, int K, float *kp_xy_sub, float *kp_pixel_sub,
                           int32_t *flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif
