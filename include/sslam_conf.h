/*
 * sslam_conf.h - C ABI of libsslam_conf.so: the seventh native library of the project (gfx950), the keypoint confidence head.
 * Replaces UncertaintyEstimator.forward and the selection rule of UncertaintyEstimator.filter_keypoints_by_confidence (reference
 * semantic-slam/models/uncertainty_estimator.py:46-67 and :123-183): a per-keypoint MLP 384 + D -> 128 -> 64 -> 1 over
 * [backbone feature at the keypoint | refined descriptor], a sigmoid, and a per-frame filter on the result.
 * Same conventions as sslam_hip.h / sslam_ext.h: every pointer is a CALLER-OWNED DEVICE pointer (the two *_host entries apart),
 * the library never allocates, frees, synchronises or reads back; `stream` is a hipStream_t passed as void*; the return value is
 * SSLAM_OK or a negative SSLAM_E_* code of sslam_hip.h; every refusal comes before anything is launched and writes nothing.
 * Results are written with ordinary vector stores; there is no workspace and there are no floating-point atomics: every entry can
 * be captured in a graph.  Built with -ffp-contract=off and the correctly rounded divide: a fused multiply-add happens exactly
 * where fmaf is written below, every other operation is rounded once, and a result is the same bits as tests/confidence_ref.py.
 * The entries carry the prefix sslc_.
 */
#ifndef SSLAM_CONF_H
#define SSLAM_CONF_H

#include <stdint.h>

#include "sslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ALIGNMENT, every entry that takes device pointers: the LEAST alignment in bytes of each pointer argument - the widest access
 * the entry's kernel makes to it (4 an fp32 or int32 word, 16 four of them loaded as one).  A pointer that misses its alignment:
 * SSLAM_E_INVALID before anything is launched, nothing written.  A result is a function of the operands' values, not of their
 * addresses (tests/test_gpu_confidence.py runs every pointer at its least alignment, just past and just before a 256-byte boundary).
 * No entry takes a stride.
 *   sslc_confidence_rows: x 16, desc 16, packed 16, conf 4
 *   sslc_gather_confidence: feat 16, kp_xy 4, desc 16, packed 16, conf 4
 *   sslc_confidence_filter: conf 4, slot 4, count 4, conf_out 4
 *   sslc_take_rows: src 4, slot 4, dst 4
 */

/* ---- SIZE LIMITS: the expressions the dispatch code tests, the code returned where one is false, and the widths in bits of the
 * kernels' index expressions (tests/conf_table.py restates them, tests/test_confidence_cpu.py holds the header to the table).
 *   sslc_confidence_rows: rows <= 0x7fffffff, else SSLAM_E_UNSUPPORTED; D == 128 or D == 256, else SSLAM_E_UNSUPPORTED. offsets: row * 384 64, row * D 64, tile = rows / 32 31
 *   sslc_gather_confidence: n_frames * K <= 0x7fffffff, else SSLAM_E_UNSUPPORTED; D == 128 or D == 256, else SSLAM_E_UNSUPPORTED. offsets: frame * G * G * 384 64, row * D 64, tile = rows / 32 31
 *   sslc_confidence_filter: K <= 4096, else SSLAM_E_UNSUPPORTED. offsets: frame * K 64
 *   sslc_take_rows: n_frames * K * width <= 0x7fffffff, else SSLAM_E_UNSUPPORTED. offsets: word index n_frames * K * width 64
 */

int sslc_version(void);
const char *sslc_arch(void);          /* "gfx950" */
long long sslc_launch_count(void);    /* kernels this library has launched in this process - a launch that returned
                                         SSLAM_E_LAUNCH is not counted (diagnostic; relaxed atomic) */

#define SSLC_DINO_DIM 384             /* the one feature width: SSLAM_C */
#define SSLC_HIDDEN_DIM 128           /* the one hidden width; the second layer has SSLC_HIDDEN_DIM / 2 units */
#define SSLC_FILTER_MAX_K 4096
#define SSLC_TILE_ROWS 32             /* keypoint rows of one workgroup */
#define SSLC_CONF_MIN 1.17549435e-38f /* the least confidence above zero: FLT_MIN, the least normal fp32 */

/* ---- The packed head.  The six tensors of the reference's state_dict - mlp.0.weight (128, 384 + D), mlp.0.bias (128),
 * mlp.2.weight (64, 128), mlp.2.bias (64), mlp.4.weight (1, 64), mlp.4.bias (1) - in ONE buffer of `total` floats, at the offsets
 * (in floats, each a multiple of 4) the layout returns.  The two matrices stand in MFMA-fragment order, [k / 8][n][8 floats KP8]
 * as sslam_pack_linear_host writes it: W[n][k] at ((k / 8) * N + n) * 8 + kp8(k % 8), kp8 = (0, 2, 4, 6, 1, 3, 5, 7) -> position.
 * Supported: dino_dim 384; descriptor_dim 128 or 256; hidden_dim 128.  Anything else: SSLAM_E_UNSUPPORTED (a caller then runs
 * the head elsewhere).  SSLAM_E_INVALID: a NULL pointer, a non-positive dimension. */
typedef struct {
    int d;                 /* descriptor_dim */
    long long total;       /* floats in the packed buffer */
    long long w1, b1;      /* packed mlp.0.weight, mlp.0.bias */
    long long w2, b2;      /* packed mlp.2.weight, mlp.2.bias */
    long long w3, b3;      /* mlp.4.weight as it is, mlp.4.bias */
} sslc_confidence_layout_t;
int sslc_confidence_layout(int dino_dim, int descriptor_dim, int hidden_dim, sslc_confidence_layout_t *layout_host);
/* w_host: the six host pointers in state_dict order */
int sslc_confidence_pack_host(const float *const *w_host, int dino_dim, int descriptor_dim, int hidden_dim, float *out_host);

/* ---- The head on rows that are already gathered: x (rows, 384) fp32, desc (rows, D) fp32, packed as above -> conf (rows) fp32.
 * NUMERICS, all IEEE fp32, per row, `in` = [x_0 .. x_383, d_0 .. d_{D-1}]:
 *   h1[n] = relu(chain over k = 0 .. 383 + D, from b1[n]:  acc = fmaf(in[k], W1[n][k], acc)),  n = 0 .. 127
 *   h2[n] = relu(chain over k = 0 .. 127, from b2[n]:      acc = fmaf(h1[k], W2[n][k], acc)),  n = 0 .. 63
 *   logit = chain over k = 0 .. 63, from b3:               acc = fmaf(h2[k], W3[k], acc)
 *   s     = 1.0f / (1.0f + expf_c(-logit)),  expf_c the canonical exponential of the project (sslam_sigmoid of csrc/common.h)
 *   conf  = s < SSLC_CONF_MIN ? +0.0f : s     (no subnormal confidence is written)
 *   relu(v) = v > 0 ? v : +0.0f.
 * Each chain is ONE fused-multiply-add chain in increasing k: the first two run on v_mfma_f32_32x32x2_f32, which computes exactly
 * that chain (tests/test_gpu_parity.py::test_mfma_chain_is_fmaf_chain), the last on the vector pipe.
 * Rows are independent: a row's confidence is a function of that row's operands and the weights alone - not of its position, of
 * its tile or of the launch shape.  Finite inputs give a confidence in [0, 1].  The canonical exponential clamps its argument to
 * [-87, 88], so the canonical sigmoid alone never reaches 0: its floor is the subnormal 1.0f / (1.0f + expf_c(88.0f)) = 6.05e-39.
 * The last line removes that: wherever s is a normal number - every logit above about -87.3 - conf is s, the bits of ora.sigmoid;
 * below, conf is exactly +0.0f, as a logit above about 17 gives exactly 1.0f.  Non-finite inputs are outside the contract; nothing
 * is written outside conf either way.
 * Launch: one kernel, one workgroup of 256 threads per SSLC_TILE_ROWS rows; the tile ([x | desc] in KP8 order, 388 + D floats a
 * row) lives in LDS; the products are evaluated transposed (weights the A operand), so the ReLU works on registers; the packed
 * weights are fetched by buffer loads at scalar offsets, not staged in LDS.  A last tile that is not full reads the last row
 * again and writes only the rows there are.
 * SSLAM_E_INVALID: a NULL pointer; rows <= 0; a pointer that misses its alignment.  SSLAM_E_UNSUPPORTED: D other than 128 or 256;
 * rows above 2^31 - 1. */
int sslc_confidence_rows(const float *x, const float *desc, long long rows, int D, const float *packed, float *conf, void *stream);

/* ---- The same rows, the 384 features taken inside the kernel by the bilinear gather of sslam_gather (grid_sample bilinear,
 * align_corners=True, zero padding; csrc/gather_taps.h): feat (n_frames, G, G, 384), kp_xy (n_frames, K, 2) in patch units,
 * desc (n_frames, K, D) -> conf (n_frames, K).  Nothing of width 384 is written to memory.  The same bits as sslam_gather
 * followed by sslc_confidence_rows.
 * SSLAM_E_INVALID: a NULL pointer; n_frames <= 0, G <= 1 or K <= 0; a pointer that misses its alignment.
 * SSLAM_E_UNSUPPORTED: D other than 128 or 256; n_frames * K above 2^31 - 1. */
int sslc_gather_confidence(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *desc, int D,
                           const float *packed, float *conf, void *stream);

/* ---- The selection rule of filter_keypoints_by_confidence, per frame: conf (n_frames, K) fp32 ->
 *   slot (n_frames, K) int32, count (n_frames) int32, conf_out (n_frames, K) fp32.
 *   Slot k is kept iff conf[k] >= threshold (a NaN confidence fails; with a NaN threshold every slot fails).
 *   A frame that keeps none keeps the slot of its largest confidence, the lowest index on equality (a NaN is never the largest;
 *   a frame of NaNs keeps slot 0).
 *   count[f] = the number kept, 1 .. K;  slot[f, 0 .. count) = the kept slots in ascending order;
 *   slot[f, count .. K) = the last kept slot again (the reference's pad repeats the last kept keypoint);
 *   conf_out[f, j] = conf[f, slot[f, j]] for j < count, +0.0f from there on (the reference pads the confidence with zeros).
 * Every element of the three outputs is written; nothing else is.
 * Launch: one kernel, one workgroup of 256 threads per frame; integer prefix sums only.
 * SSLAM_E_INVALID: a NULL pointer; n_frames or K <= 0; a pointer that misses its alignment; an output that starts where conf
 * starts.  SSLAM_E_UNSUPPORTED: K above SSLC_FILTER_MAX_K. */
int sslc_confidence_filter(const float *conf, int n_frames, int K, float threshold, int32_t *slot, int32_t *count, float *conf_out,
                           void *stream);

/* ---- dst[f, j, :] = src[f, slot[f, j], :] for rows of `width` 4-byte words: src and dst (n_frames, K, width), slot
 * (n_frames, K) int32 as the filter writes it.  The words are moved as bit patterns: fp32 and int32 alike.  One launch per array,
 * one thread per word.  A slot outside 0 .. K - 1 reads nothing: its row of dst is written as zero words.
 * SSLAM_E_INVALID: a NULL pointer; n_frames, K or width <= 0; a pointer that misses its alignment; dst == src (dst must not
 * overlap src).  SSLAM_E_UNSUPPORTED: n_frames * K * width above 2^31 - 1. */
int sslc_take_rows(const void *src, const int32_t *slot, int n_frames, int K, int width, void *dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif
