// refine.hip - A6 + A7: bilinear feature gather and the descriptor MLP, fused per 32-row tile.
// Replaces DinoBackbone.extract_at_keypoints (reference semantic-slam/models/dino_backbone.py:114-152) and
// DescriptorRefiner.forward / ResidualBlock.forward (semantic-slam/models/descriptor_refiner.py:58-126).
//
// One workgroup (4 waves; three are co-resident per CU) owns 32 keypoint rows for the WHOLE chain: gather ->
// input_proj+ReLU -> n_blocks x {LN, fc1, ReLU, LN, fc2, +identity, ReLU} -> output_proj -> L2 normalise.  The 32x384
// activation tile lives in LDS (KP8 order, 388-float rows).  The products are evaluated TRANSPOSED: the weight
// fragment is the MFMA A operand and the activation rows the B operand, so a lane's accumulators hold ONE activation row
// (96 of its columns per wave).  ReLU, the residual identity and LayerNorm then work on registers: row statistics are
// lane-local sums, one xor-32 shuffle and a 4-wave exchange through LDS; the tile is written once per layer in 8-byte
// pairs.  (The earlier row-per-wave LayerNorm on the LDS tile cost ~1 000 instructions per call, and every instruction
// a wave issues besides its MFMAs takes issue time from the matrix pipe it shares - DESIGN_HISTORY.md section 9.)
// The pre-packed weights (3.17 MB, L2-resident, shared by all workgroups) are NOT staged through LDS: they are stored in
// MFMA-fragment order ([k/8][n][8 floats KP8]) and fetched by buffer loads with scalar (layer, k-group, tile) offsets,
// 1 KB coalesced per wave-instruction, two k-groups ahead.  A layer's GEMM has no barrier.
// All contractions are v_mfma_f32_32x32x2_f32 chains in increasing k from the bias: bit-identical to the oracle.
//
// Roofline: MFMA-bound, 1 572 864 FLOP per row (786.4 MFLOP per 500-keypoint frame) against 1.5 KB in / 0.5 KB out.
#include "common.h"
#include "gather_taps.h"

namespace {

#ifndef SSLAM_REFINE_WMR
#define SSLAM_REFINE_WMR 1
#endif
constexpr int WMR = SSLAM_REFINE_WMR;   // waves along M: 1 -> 32-row workgroups of 4 waves (3 co-resident per CU, so the
                                        // gather / LayerNorm phases of one overlap the GEMMs of the others); 2 -> 64 rows
constexpr int RM = 32 * WMR;        // rows per workgroup
constexpr int NTHR = 256 * WMR;
constexpr int HID = SSLAM_HID;      // 384
constexpr int LDH = HID + 4;        // activation row stride (floats)
constexpr int NKG = HID / 8;        // 48 k-groups of 8 per layer
constexpr int H_FLOATS = RM * LDH;
constexpr int SCRATCH_FLOATS = 256;     // two [4][32] row-statistic exchange buffers
constexpr int SMEM_FLOATS = H_FLOATS + SCRATCH_FLOATS;   // 100 352 B

struct RefArgs {
    const float *packed;
    sslam_refiner_layout_t lay;
};

// acc[t] (32 rows x 32 cols each, t-th N tile of this wave) = bias + H(64 x 384) . W^T, one fma chain per output in
// increasing k.  B fragments come straight from global memory (fragment-ordered packed weights), ring of 3 k-groups.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int NT>
__device__ __forceinline__ void gemm_lds(const float *H, __amdgpu_buffer_rsrc_t wrs, int w_off, const float *__restrict__ bias,
                                         int tid, f32x16 (&acc)[NT]) {
    constexpr int N = 128 * NT;
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5, wm = wave >> 2, wn = wave & 3;
    // TRANSPOSED product: the weight fragment is the MFMA A operand and the activation row the B operand, so the
    // accumulator of lane (r, h) holds activation row m = r and output columns n = slab + 32t + crow(e, h) (runs of
    // four consecutive n).  The fma chain of every output is unchanged (a*b commutes, k ascending from the bias).
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + wn * 32 * NT + t * 32 + 8 * q + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; i++) acc[t][4 * q + i] = bv[i];
        }
    // lane's B fragment of k-group g, tile t: 16 B at ((g*N + n)*8 + 4h) floats, n = wn*32*NT + t*32 + r.  Buffer loads:
    // address = descriptor base + 32-bit lane offset (constant) + SCALAR offset of (layer, k-group, tile), so the k loop
    // carries no vector address arithmetic at all - every non-MFMA instruction costs matrix-pipe issue time (DESIGN_HISTORY.md section 9)
    const int loff = ((wn * 32 * NT + r) * 2 + h) * 16;
    const float *A = H + (wm * 32 + r) * LDH + 4 * h;
    f32x4 b0[NT], b1[NT], b2[NT];
#define LOAD_B(dst, g)                                                               \
    _Pragma("unroll") for (int t = 0; t < NT; t++)                                   \
        dst[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, loff, w_off + ((g) * N + t * 32) * 32, 0));
#define STEP(cur, g)                                                                  \
    {                                                                                 \
        const f32x4 a = an;                                                           \
        an = *reinterpret_cast<const f32x4 *>(A + 8 * (((g) + 1) < NKG ? (g) + 1 : (g))); /* next k-group's A */ \
        _Pragma("unroll") for (int st = 0; st < 4; st++)                              \
            _Pragma("unroll") for (int t = 0; t < NT; t++) acc[t] = mfma32(cur[t][st], a[st], acc[t]); \
    }
    LOAD_B(b0, 0);
    LOAD_B(b1, 1);
    f32x4 an = *reinterpret_cast<const f32x4 *>(A);
#pragma unroll 1
    for (int g = 0; g < NKG; g += 3) {
        // the refills are UNCONDITIONAL (clamped index, a redundant reload in the last trip): with a branch around them the
        // compiler cannot count the loads in flight and falls back to s_waitcnt vmcnt(0) before the third step of every
        // trip, which drains the whole prefetch ring
        // (sched_barrier: program order = issue order, or the scheduler sinks the loads next to their uses)
        LOAD_B(b2, g + 2);
        __builtin_amdgcn_sched_barrier(0);
        STEP(b0, g);
        __builtin_amdgcn_sched_barrier(0);
        LOAD_B(b0, min(g + 3, NKG - 1));
        __builtin_amdgcn_sched_barrier(0);
        STEP(b1, g + 1);
        __builtin_amdgcn_sched_barrier(0);
        LOAD_B(b1, min(g + 4, NKG - 1));
        __builtin_amdgcn_sched_barrier(0);
        STEP(b2, g + 2);
        __builtin_amdgcn_sched_barrier(0);
    }
#undef LOAD_B
#undef STEP
}

// this wave's 32 rows x 96 columns (transposed accumulators) -> activation tile (KP8 positions): the four consecutive
// columns c .. c + 3 of an accumulator quad land at floats 0, 4, 1, 5 of their group of 8.  Two ds_write2_b32 per quad, written
// as such: from C++ stores hipcc builds 8-byte writes of the pairs (c, c + 2), (c + 1, c + 3), which need those pairs in adjacent
// registers - six v_mov per quad, and every vector instruction of a hand-over is issue time the matrix pipe does not get.
// (The compiler does not count these LDS operations: lds_quads_done() waits for them before the barrier that publishes the tile.)
template <int V>
struct IC {
    static constexpr int value = V;
};
template <int DW>
__device__ __forceinline__ void store_quad(unsigned row_lds, float y0, float y1, float y2, float y3) {
    asm volatile("ds_write2_b32 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(row_lds), "v"(y0), "v"(y1), "n"(DW), "n"(DW + 4) : "memory");
    asm volatile("ds_write2_b32 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(row_lds), "v"(y2), "v"(y3), "n"(DW + 1), "n"(DW + 5) : "memory");
}
__device__ __forceinline__ void lds_quads_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ unsigned lds_addr(const float *p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const float *)p;
}
// ReLU of an MFMA accumulator: ONE v_max_f32.  From `x > 0 ? x : 0` or
// fmaxf hipcc first canonicalises the operand (v_max_f32 x, x, x - it quiets a signalling NaN, which no arithmetic result is)
// and then takes the maximum: 96 instructions per sweep where 48 do the work, all of them issue time the matrix pipe does not
// get.  Same bits for every input that can occur here: max(+0, -0) = +0 and max(0, quiet NaN) = 0, as the ternary gives.
__device__ __forceinline__ float relu(float x) {
    float y;
    asm("v_max_f32 %0, 0, %1" : "=v"(y) : "v"(x));
    return y;
}
template <int I>
__device__ __forceinline__ void store_rows_from(unsigned row_lds, const f32x16 (&v)[3]) {
    if constexpr (I < 12) {
        constexpr int t = I / 4, q = I % 4;
        store_quad<32 * t + 8 * q>(row_lds, v[t][4 * q], v[t][4 * q + 1], v[t][4 * q + 2], v[t][4 * q + 3]);
        store_rows_from<I + 1>(row_lds, v);
    }
}
__device__ __forceinline__ void store_rows(float *H, int tid, const f32x16 (&v)[3]) {
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5, wn = wave & 3;
    store_rows_from<0>(lds_addr(H + r * LDH + wn * 96 + 2 * h), v);
    lds_quads_done();
}

// lane-local partial p of one row statistic -> its total over the row's 384 (or 128) columns, in the canonical tree of the
// oracle (slab_total): the two half-waves of a wave, then the four waves in order.  `part` is a [4][32] LDS array; the
// caller alternates between two of them so that consecutive reductions need no extra barrier.
__device__ __forceinline__ float row_total(float p, float *part, int tid) {
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5, wn = wave & 3;
    p = p + __shfl_xor(p, 32);
    if (h == 0) part[wn * 32 + r] = p;
    __syncthreads();
    return ((part[r] + part[32 + r]) + part[64 + r]) + part[96 + r];
}

// LayerNorm(384) of the wave's transposed accumulators (row m = r per lane), written to the activation tile as the next
// GEMM's operand; v itself (the residual identity, where it is one) stays untouched in registers.  Oracle: layernorm384.
// The affine parameters of the lane's 48 columns are 12 (gamma, beta) quads from the L2-resident packed buffer.  They are
// requested THREE QUADS AHEAD through a register ring, the first three before the row statistics: loaded where they are used,
// hipcc waits for each pair right behind its request - 12 serial L2 round trips per call, most of a hand-over's 40-50 k cycles.
__device__ __forceinline__ void layernorm_store(float *H, float *part0, float *part1, const float *__restrict__ gam,
                                                const float *__restrict__ bet, int tid, const f32x16 (&v)[3]) {
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5, wn = wave & 3;
    const float *gp = gam + wn * 96 + 4 * h, *bp = bet + wn * 96 + 4 * h;      // quad i = (t, qd) = (i / 4, i % 4) at + 32 t + 8 qd
    constexpr int AHEAD = 3;
    f32x4 g4[AHEAD], b4[AHEAD];
#define LN_REQ(i_)                                                                                       \
    {                                                                                                    \
        g4[(i_) % AHEAD] = *reinterpret_cast<const f32x4 *>(gp + 32 * ((i_) / 4) + 8 * ((i_) % 4));      \
        b4[(i_) % AHEAD] = *reinterpret_cast<const f32x4 *>(bp + 32 * ((i_) / 4) + 8 * ((i_) % 4));      \
    }
#pragma unroll
    for (int i = 0; i < AHEAD; i++) LN_REQ(i)
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) s = s + v[t][e];
    const float mean = row_total(s, part0, tid) / 384.0f;
    float q = 0.0f;
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const float d = v[t][e] - mean;
            q = __builtin_fmaf(d, d, q);
        }
    const float var = row_total(q, part1, tid) / 384.0f;
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    const unsigned row_lds = lds_addr(H + r * LDH + wn * 96 + 2 * h);
    auto quad = [&](auto ic) {
        constexpr int i = decltype(ic)::value, t = i / 4, qd = i % 4;
        const f32x4 gq = g4[i % AHEAD], bq = b4[i % AHEAD];
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; j++) y[j] = __builtin_fmaf((v[t][4 * qd + j] - mean) * rstd, gq[j], bq[j]);
        if constexpr (i + AHEAD < 12) LN_REQ(i + AHEAD)
        __builtin_amdgcn_sched_barrier(0);      // keeps the request of quad i + 3 in front of the arithmetic of quad i + 1
        store_quad<32 * t + 8 * qd>(row_lds, y[0], y[1], y[2], y[3]);
    };
    quad(IC<0>{}); quad(IC<1>{}); quad(IC<2>{}); quad(IC<3>{}); quad(IC<4>{}); quad(IC<5>{});
    quad(IC<6>{}); quad(IC<7>{}); quad(IC<8>{}); quad(IC<9>{}); quad(IC<10>{}); quad(IC<11>{});
    lds_quads_done();
#undef LN_REQ
}

// Optional phase timers (build with -DSSLAM_CLOCK_PROBE, read with tools/clock_probe.py): wave 0 of the first 4096 workgroups
// records its lifetime and the shader-clock cycles it spent in the gather, the GEMM loops, the LayerNorm calls, the tile
// stores and waiting at barriers.  Compiled out of the product build.
#ifdef SSLAM_CLOCK_PROBE
__device__ unsigned long long g_probe_refine[8 * 4096];
#define PROBE_BEGIN() const unsigned long long pr_t0 = clock64(); unsigned long long pr_q = 0, pr_acc[6] = {0, 0, 0, 0, 0, 0}
#define PROBE(slot, stmt) { pr_q = clock64(); stmt; pr_acc[slot] += clock64() - pr_q; }
#define PROBE_END()                                                                                         \
    if (threadIdx.x == 0 && blockIdx.x < 4096) {                                                            \
        g_probe_refine[8 * blockIdx.x] = clock64() - pr_t0;                                                 \
        for (int i_ = 0; i_ < 6; i_++) g_probe_refine[8 * blockIdx.x + 1 + i_] = pr_acc[i_];                \
    }
#else
#define PROBE_BEGIN()
#define PROBE(slot, stmt) { stmt; }
#define PROBE_END()
#endif
// Issue priority: a wave outside its GEMM loops (gather, LayerNorm hand-over, tile stores, epilogue) runs at priority 1, inside
// them at 0: the arbiter otherwise serves the co-resident workgroups' back-to-back MFMAs first and a hand-over of ~1 000
// instructions takes 40-50 k cycles; with the hint it is through sooner and back to feeding the matrix pipe (-1.5 %).
#define PRIO_OTHER() __builtin_amdgcn_s_setprio(1)
#define PRIO_GEMM() __builtin_amdgcn_s_setprio(0)
enum { PR_GATHER = 0, PR_GEMM = 1, PR_LN = 2, PR_STORE = 3, PR_BARRIER = 4 };

// WL (work list): row i of the launch is global row list[i], i < *n_list - the distinct keypoints of all frames, packed by
// distinct_rep_kernel / distinct_list_kernel below; the grid is sized for the worst case (every row distinct) and the
// workgroups beyond the device-side tile count leave at once.  Rows are independent in this kernel (every fma chain, row
// statistic and norm uses one row only), so which tile a row sits in changes no bit of it.
// NT: 32-column tiles of the output projection per wave = descriptor width / 128 (1 or 2).
template <bool WL, int NT>
__global__ __launch_bounds__(NTHR, WMR == 1 ? 3 : 2) void gather_refine_kernel(const float *__restrict__ feat, int G,
                                                             const float *__restrict__ kp_xy, int K,
                                                             const float *__restrict__ x_in, long long rows,
                                                             const int *__restrict__ list, const int *__restrict__ n_list,
                                                             RefArgs args, float *__restrict__ desc) {
    __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
    float *H = smem, *scratch = smem + H_FLOATS;
    const int tid = threadIdx.x;
    int n_tiles = gridDim.x;
    if constexpr (WL) {
        rows = *n_list;
        n_tiles = (int)((rows + RM - 1) / RM);
        if ((int)blockIdx.x >= n_tiles) return;
    }
    PROBE_BEGIN();
    PRIO_OTHER();
    // XCD-aware order: workgroup b runs on XCD b % 8; give every XCD one contiguous range of row tiles so that the ~8
    // tiles gathering from one frame's feature map share that XCD's L2 instead of fetching the frame into all eight
    long long R0;
    {
        const int b = blockIdx.x, q = n_tiles / 8, rem = n_tiles % 8, x = b % 8;
        R0 = (long long)((x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + b / 8) * RM;
    }
    const float *pk = args.packed;
    const sslam_refiner_layout_t &L = args.lay;
    // buffer descriptor over the packed weights (raw buffer, 32-bit element format word as on gfx90a/gfx94x/gfx950)
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pk), 0, (int)(L.total * 4), 0x00020000);

    // ---- phase 0: fill the activation tile (gathered features, or rows of x_in) --------------------------------
    {
        // thread (row, part) moves the 8-channel chunks j*8 + part, j = 0..5: the 8 lanes of a row cover 64 CONTIGUOUS floats
        // per step - full 256-byte runs of every tap row, and 8 distinct 4-bank groups for the two ds_write_b128 (the earlier
        // part*6 + j order put the 8 lanes 48 floats apart: 4-way bank conflicts, PMC SQ_LDS_BANK_CONFLICT)
        const int row = tid >> 3, part = tid & 7;
        long long R = R0 + row;
        if (R > rows - 1) R = rows - 1;
        if constexpr (WL) R = list[R];
        float *dst = H + row * LDH;
        if (feat) {
            const long long f = R / K;
            const Taps t = make_taps(feat + f * G * G * SSLAM_C, G, kp_xy[2 * R], kp_xy[2 * R + 1]);
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const int c0 = 8 * (j * 8 + part);
                float4 ev, od;
                kp8_split(blend4(t, c0), blend4(t, c0 + 4), ev, od);
                *reinterpret_cast<float4 *>(dst + c0) = ev;
                *reinterpret_cast<float4 *>(dst + c0 + 4) = od;
            }
        } else {
            const float *src = x_in + R * SSLAM_C;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const int c0 = 8 * (j * 8 + part);
                float4 ev, od;
                kp8_split(*reinterpret_cast<const float4 *>(src + c0), *reinterpret_cast<const float4 *>(src + c0 + 4), ev, od);
                *reinterpret_cast<float4 *>(dst + c0) = ev;
                *reinterpret_cast<float4 *>(dst + c0 + 4) = od;
            }
        }
    }
#ifdef SSLAM_CLOCK_PROBE
    pr_acc[PR_GATHER] = clock64() - pr_t0;
#endif
    PROBE(PR_BARRIER, __syncthreads();)

    // ---- input_proj + ReLU (descriptor_refiner.py:76) -----------------------------------------------------------
    // Hand-over between two GEMMs: every wave turns its accumulators into the next operand IN REGISTERS (ReLU, residual,
    // LayerNorm with lane-local row statistics) and writes the tile once; the barriers inside row_total also order the
    // tile accesses (all waves have left the GEMM that read the tile before anyone writes it).
    float *part0 = scratch, *part1 = scratch + 128;
    f32x16 X[3], acc[3];
    PRIO_GEMM(); PROBE(PR_GEMM, gemm_lds<3>(H, wrs, (int)L.in_w * 4, pk + L.in_b, tid, acc);) PRIO_OTHER();
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) X[t][e] = relu(acc[t][e]);

    // ---- residual blocks (descriptor_refiner.py:108-126) --------------------------------------------------------
    for (int b = 0; b < L.n_blocks; b++) {
        PROBE(PR_LN, layernorm_store(H, part0, part1, pk + L.blk[b][0], pk + L.blk[b][1], tid, X);)
        PROBE(PR_BARRIER, __syncthreads();)
        PRIO_GEMM(); PROBE(PR_GEMM, gemm_lds<3>(H, wrs, (int)L.blk[b][2] * 4, pk + L.blk[b][3], tid, acc);) PRIO_OTHER();
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[t][e] = relu(acc[t][e]);
        PROBE(PR_LN, layernorm_store(H, part0, part1, pk + L.blk[b][4], pk + L.blk[b][5], tid, acc);)
        PROBE(PR_BARRIER, __syncthreads();)
        PRIO_GEMM(); PROBE(PR_GEMM, gemm_lds<3>(H, wrs, (int)L.blk[b][6] * 4, pk + L.blk[b][7], tid, acc);) PRIO_OTHER();
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                // an add's result is canonical: hipcc emits the one v_max_f32 itself here, and keeps the adds packed
                const float v = acc[t][e] + X[t][e];
                X[t][e] = v > 0.0f ? v : 0.0f;
            }
    }
    PROBE(PR_BARRIER, __syncthreads();)            // every wave has finished reading the tile
    PROBE(PR_STORE, store_rows(H, tid, X);)
    PROBE(PR_BARRIER, __syncthreads();)

    // ---- output_proj + L2 normalise (:83-86; F.normalize eps 1e-12) --------------------------------------------
    // wave wn owns the columns wn * 32 NT + 32 t + crow(e, h); the lane's share of the L2 sum is one fma chain in (t, e) order
    f32x16 o[NT];
    PRIO_GEMM(); PROBE(PR_GEMM, gemm_lds<NT>(H, wrs, (int)L.out_w * 4, pk + L.out_b, tid, o);) PRIO_OTHER();
    {
        const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5, wn = wave & 3;
        float ss = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int e = 0; e < 16; e++) ss = __builtin_fmaf(o[t][e], o[t][e], ss);
        const float den = fmaxf(sqrtf(row_total(ss, part0, tid)), 1e-12f);
        if (R0 + r < rows) {
            long long Ro = R0 + r;
            if constexpr (WL) Ro = list[Ro];
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    f32x4 w4;
#pragma unroll
                    for (int i = 0; i < 4; i++) w4[i] = o[t][4 * q + i] / den;
                    *reinterpret_cast<f32x4 *>(desc + Ro * (128 * NT) + wn * 32 * NT + 32 * t + 8 * q + 4 * h) = w4;
                }
        }
    }
    PROBE_END();
}

__global__ __launch_bounds__(256) void gather_kernel(const float *__restrict__ feat, int G, const float *__restrict__ kp_xy,
                                                      int K, long long rows, float *__restrict__ out) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;   // one float4 of one row
    const long long R = item / (SSLAM_C / 4);
    if (R >= rows) return;
    const int c0 = (int)(item % (SSLAM_C / 4)) * 4;
    const long long f = R / K;
    const Taps t = make_taps(feat + f * G * G * SSLAM_C, G, kp_xy[2 * R], kp_xy[2 * R + 1]);
    *reinterpret_cast<float4 *>(out + R * SSLAM_C + c0) = blend4(t, c0);
}

// ---- distinct-row work list ------------------------------------------------------------------------------------------
// select_keypoints almost always ends in the reference's pad (select.hip: the NMS survivors first, then the top raw
// saliencies, among which the survivors re-appear): ~7 % of a frame's keypoints repeat an earlier one bit for bit, and
// equal coordinates give equal taps, equal gathered rows and equal descriptors.  Three small launches around the MLP let it
// run every distinct (x, y) of a frame once:
//   distinct_rep_kernel   rep[R] = the lowest row of R's frame with the same 64 coordinate bits; counts[f] = distinct rows
//   distinct_list_kernel  list = the rows with rep[R] == R, frames in order, slots ascending, all frames in ONE run (a tile
//                         boundary per frame would give back half the gain); counts[n_frames] = their number
//   copy_duplicates_kernel (after the MLP)  desc[R] = desc[rep[R]] where rep[R] != R
// Workspace (int32 words): counts[n_frames + 1] | rep[rows] | list[rows], each part on a 256-byte boundary.
constexpr int DN = 256;                     // threads of the two list kernels, one workgroup per frame
constexpr int DISTINCT_MAX_K = 4096;        // the LDS hash table holds 2 K slots (32 KB here)
// Up to three workgroups per CU are resident: a launch of no more than 256 x 3 tiles is ONE round with or without the
// duplicates, and the extra launches would only add latency (single frames, the online stepper).
constexpr long long DISTINCT_MIN_ROWS = 256 * 3 * RM + 1;

__device__ __forceinline__ bool is_nan_bits(unsigned u) { return (u & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ unsigned hash_xy(unsigned x, unsigned y) {
    unsigned h = x * 0x9e3779b1u ^ (y + 0x7f4a7c15u) * 0x85ebca6bu;
    h ^= h >> 15;
    h *= 0x2c1b3c6du;
    return h ^ (h >> 13);
}
// sum of v over the workgroup (DN threads); `red` is an LDS array of DN / 64 ints, free again after the call
__device__ __forceinline__ int block_sum(int v, int *red, int tid) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < DN / 64; w++) s += red[w];
    return s;
}

// Open addressing on the coordinate BITS (+0.0 and -0.0 differ; a NaN coordinate never merges): a table slot holds a row of
// its key, lowered to the smallest such row by atomicMin - so the result does not depend on the order of the insertions.
__global__ __launch_bounds__(DN) void distinct_rep_kernel(const unsigned *__restrict__ kp_bits, int K, int T,
                                                          int *__restrict__ rep, int *__restrict__ counts) {
    extern __shared__ int tab[];            // T slots, T a power of two >= 2 K: every probe sequence meets an empty slot
    __shared__ int red[DN / 64];
    const int tid = threadIdx.x, f = blockIdx.x, mask = T - 1;
    const unsigned *kp = kp_bits + 2ll * f * K;
    for (int i = tid; i < T; i += DN) tab[i] = -1;
    __syncthreads();
    for (int j = tid; j < K; j += DN) {
        const unsigned x = kp[2 * j], y = kp[2 * j + 1];
        if (is_nan_bits(x) || is_nan_bits(y)) continue;
        for (unsigned h = hash_xy(x, y) & mask;; h = (h + 1) & mask) {
            const int cur = atomicCAS(&tab[h], -1, j);
            if (cur == -1) break;
            if (kp[2 * cur] == x && kp[2 * cur + 1] == y) {
                atomicMin(&tab[h], j);
                break;
            }
        }
    }
    __syncthreads();
    int n = 0;
    for (int j = tid; j < K; j += DN) {
        const unsigned x = kp[2 * j], y = kp[2 * j + 1];
        int r = j;
        if (!(is_nan_bits(x) || is_nan_bits(y)))
            for (unsigned h = hash_xy(x, y) & mask;; h = (h + 1) & mask) {
                const int cur = tab[h];     // never empty before the key's own slot: the slot was on j's insertion path
                if (cur < 0) break;
                if (kp[2 * cur] == x && kp[2 * cur + 1] == y) {
                    r = cur;
                    break;
                }
            }
        rep[(long long)f * K + j] = f * K + r;
        n += r == j;
    }
    n = block_sum(n, red, tid);
    if (tid == 0) counts[f] = n;
}

__global__ __launch_bounds__(DN) void distinct_list_kernel(const int *__restrict__ rep, int K, int n_frames,
                                                           int *__restrict__ counts, int *__restrict__ list) {
    __shared__ int red[DN / 64];
    const int tid = threadIdx.x, f = blockIdx.x, lane = tid & 63;
    int before = 0;                         // distinct rows of the frames in front of this one
    for (int i = tid; i < f; i += DN) before += counts[i];
    before = block_sum(before, red, tid);
    // thread tid owns the slots [b, e) of the frame; exclusive scan of the per-thread counts
    const int chunk = (K + DN - 1) / DN, b = min(tid * chunk, K), e = min(b + chunk, K), R0 = f * K;
    int local = 0;
    for (int j = b; j < e; j++) local += rep[R0 + j] == R0 + j;
    int incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();
    if (lane == 63) red[tid >> 6] = incl;
    __syncthreads();
    int slot = before + incl - local;
    for (int w = 0; w < (tid >> 6); w++) slot += red[w];
    for (int j = b; j < e; j++)
        if (rep[R0 + j] == R0 + j) list[slot++] = R0 + j;
    if (f == n_frames - 1 && tid == DN - 1) counts[n_frames] = slot;     // the last thread of the last frame ends at the total
}

template <int D>
__global__ __launch_bounds__(256) void copy_duplicates_kernel(const int *__restrict__ rep, long long rows, float *desc) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;   // one float4 of one row
    const long long R = item / (D / 4);
    if (R >= rows) return;
    const long long src = rep[R];
    if (src == R) return;
    const int c0 = (int)(item % (D / 4)) * 4;
    *reinterpret_cast<float4 *>(desc + R * D + c0) = *reinterpret_cast<const float4 *>(desc + src * D + c0);
}

struct DistinctWs {
    long long counts, rep, list, bytes;     // byte offsets of the three parts, and the total
};
DistinctWs distinct_ws(int n_frames, long long rows) {
    auto up = [](long long b) { return (b + 255) & ~255LL; };
    DistinctWs w;
    w.counts = 0;
    w.rep = up(((long long)n_frames + 1) * 4);
    w.list = w.rep + up(rows * 4);
    w.bytes = w.list + up(rows * 4);
    return w;
}
// the launch form of a (n_frames, K) call, from its shape alone; test-only knob SSLAM_REFINE_DISTINCT: 0 = direct, 1 = work list
bool distinct_form(int n_frames, int K) {
    const long long rows = (long long)n_frames * K;
    if (K > DISTINCT_MAX_K || rows > 0x7fffffffLL) return false;        // rows are int32 in the list
    const long long forced = sslam_knob(KNOB_REFINE_DISTINCT, -1);
    return forced < 0 ? rows >= DISTINCT_MIN_ROWS : forced != 0;
}

// d: the descriptor width, 128 or 256 (checked by the entries)
int launch_refine(const float *feat, int G, const float *kp_xy, int K, const float *x_in, long long rows,
                  const float *packed, int n_blocks, int d, float *desc, void *stream) {
    RefArgs a;
    a.packed = packed;
    if (sslam_refiner_layout_d(n_blocks, d, &a.lay) != SSLAM_OK) return SSLAM_E_UNSUPPORTED;
    const unsigned grid = (unsigned)((rows + RM - 1) / RM);
    if (d == 128)
        hipLaunchKernelGGL((gather_refine_kernel<false, 1>), dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, feat, G, kp_xy, K, x_in,
                           rows, (const int *)nullptr, (const int *)nullptr, a, desc);
    else
        hipLaunchKernelGGL((gather_refine_kernel<false, 2>), dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, feat, G, kp_xy, K, x_in,
                           rows, (const int *)nullptr, (const int *)nullptr, a, desc);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

int launch_refine_distinct(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed, int n_blocks,
                           int d, float *desc, void *workspace, void *stream) {
    RefArgs a;
    a.packed = packed;
    if (sslam_refiner_layout_d(n_blocks, d, &a.lay) != SSLAM_OK) return SSLAM_E_UNSUPPORTED;
    const long long rows = (long long)n_frames * K;
    const DistinctWs w = distinct_ws(n_frames, rows);
    int *counts = (int *)((char *)workspace + w.counts), *rep = (int *)((char *)workspace + w.rep),
        *list = (int *)((char *)workspace + w.list);
    int T = 64;
    while (T < 2 * K) T <<= 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(distinct_rep_kernel, dim3(n_frames), dim3(DN), (size_t)T * 4, st, (const unsigned *)kp_xy, K, T, rep, counts);
    SSLAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(distinct_list_kernel, dim3(n_frames), dim3(DN), 0, st, rep, K, n_frames, counts, list);
    SSLAM_CHECK_LAUNCH();
    const unsigned grid = (unsigned)((rows + RM - 1) / RM);        // worst case: the host does not know the count
    if (d == 128)
        hipLaunchKernelGGL((gather_refine_kernel<true, 1>), dim3(grid), dim3(NTHR), 0, st, feat, G, kp_xy, K, (const float *)nullptr, rows,
                           (const int *)list, (const int *)(counts + n_frames), a, desc);
    else
        hipLaunchKernelGGL((gather_refine_kernel<true, 2>), dim3(grid), dim3(NTHR), 0, st, feat, G, kp_xy, K, (const float *)nullptr, rows,
                           (const int *)list, (const int *)(counts + n_frames), a, desc);
    SSLAM_CHECK_LAUNCH();
    const dim3 cgrid((unsigned)((rows * (d / 4) + 255) / 256));
    if (d == 128)
        hipLaunchKernelGGL(copy_duplicates_kernel<128>, cgrid, dim3(256), 0, st, rep, rows, desc);
    else
        hipLaunchKernelGGL(copy_duplicates_kernel<256>, cgrid, dim3(256), 0, st, rep, rows, desc);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

}  // namespace

static bool width_ok(int d) { return d == 128 || d == 256; }

extern "C" int sslam_refiner_layout_d(int n_blocks, int d, sslam_refiner_layout_t *L) {
    if (!L || n_blocks < 0 || n_blocks > 8) return SSLAM_E_INVALID;
    if (!width_ok(d)) return SSLAM_E_UNSUPPORTED;
    long long off = 0;
    auto take = [&](long long n) { const long long o = off; off += n; return o; };
    L->n_blocks = n_blocks;
    L->in_w = take((long long)HID * SSLAM_C);
    L->in_b = take(HID);
    for (int b = 0; b < 8; b++)
        for (int k = 0; k < 8; k++) L->blk[b][k] = 0;
    for (int b = 0; b < n_blocks; b++) {
        L->blk[b][0] = take(HID); L->blk[b][1] = take(HID);
        L->blk[b][2] = take((long long)HID * HID); L->blk[b][3] = take(HID);
        L->blk[b][4] = take(HID); L->blk[b][5] = take(HID);
        L->blk[b][6] = take((long long)HID * HID); L->blk[b][7] = take(HID);
    }
    L->out_w = take((long long)d * HID);
    L->out_b = take(d);
    L->total = off;
    return SSLAM_OK;
}
extern "C" int sslam_refiner_layout(int n_blocks, sslam_refiner_layout_t *L) { return sslam_refiner_layout_d(n_blocks, SSLAM_D, L); }

// w (n_out, k_in) -> [k-group = k/8][n][8 floats in KP8 order]: the MFMA B-fragment order
extern "C" int sslam_pack_linear_host(const float *w, int n_out, int k_in, float *out) {
    if (!w || !out || n_out <= 0 || k_in <= 0 || (k_in % 8)) return SSLAM_E_INVALID;
    for (int n = 0; n < n_out; n++)
        for (int k = 0; k < k_in; k++)
            out[((long long)(k / 8) * n_out + n) * 8 + kp8(k % 8)] = w[(long long)n * k_in + k];
    return SSLAM_OK;
}

extern "C" int sslam_refiner_pack_host_d(const float *const *w, int n_blocks, int d, float *out) {
    sslam_refiner_layout_t L;
    if (!w || !out) return SSLAM_E_INVALID;
    if (const int rc = sslam_refiner_layout_d(n_blocks, d, &L)) return rc;
    auto cp = [&](long long off, const float *src, int n) { for (int i = 0; i < n; i++) out[off + i] = src[i]; };
    sslam_pack_linear_host(w[0], HID, SSLAM_C, out + L.in_w);
    cp(L.in_b, w[1], HID);
    for (int b = 0; b < n_blocks; b++) {
        const float *const *p = w + 2 + 8 * b;
        cp(L.blk[b][0], p[0], HID); cp(L.blk[b][1], p[1], HID);
        sslam_pack_linear_host(p[2], HID, HID, out + L.blk[b][2]); cp(L.blk[b][3], p[3], HID);
        cp(L.blk[b][4], p[4], HID); cp(L.blk[b][5], p[5], HID);
        sslam_pack_linear_host(p[6], HID, HID, out + L.blk[b][6]); cp(L.blk[b][7], p[7], HID);
    }
    const float *const *po = w + 2 + 8 * n_blocks;
    sslam_pack_linear_host(po[0], d, HID, out + L.out_w);
    cp(L.out_b, po[1], d);
    return SSLAM_OK;
}
extern "C" int sslam_refiner_pack_host(const float *const *w, int n_blocks, float *out) {
    // as before the width-taking entry: every failure of the layout is SSLAM_E_INVALID here
    return sslam_refiner_pack_host_d(w, n_blocks, SSLAM_D, out) == SSLAM_OK ? SSLAM_OK : SSLAM_E_INVALID;
}

extern "C" int sslam_refine_d(const float *x, long long rows, const float *packed, int n_blocks, float *desc, int d, void *stream) {
    if (!x || !packed || !desc || rows <= 0) return SSLAM_E_INVALID;
    if (((uintptr_t)x | (uintptr_t)packed | (uintptr_t)desc) & 15) return SSLAM_E_INVALID;
    if (!width_ok(d)) return SSLAM_E_UNSUPPORTED;
    return launch_refine(nullptr, 0, nullptr, 1, x, rows, packed, n_blocks, d, desc, stream);
}
extern "C" int sslam_refine(const float *x, long long rows, const float *packed, int n_blocks, float *desc, void *stream) {
    if (!x || !packed || !desc || rows <= 0) return SSLAM_E_INVALID;
    if (((uintptr_t)x | (uintptr_t)packed | (uintptr_t)desc) & 15) return SSLAM_E_INVALID;      // desc: stored as 16-byte vectors
    return launch_refine(nullptr, 0, nullptr, 1, x, rows, packed, n_blocks, SSLAM_D, desc, stream);
}

extern "C" int sslam_gather_refine_d(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed,
                                     int n_blocks, float *desc, int d, void *stream) {
    if (!feat || !kp_xy || !packed || !desc || n_frames <= 0 || G <= 1 || K <= 0) return SSLAM_E_INVALID;
    if (((uintptr_t)feat | (uintptr_t)packed | (uintptr_t)desc) & 15) return SSLAM_E_INVALID;
    if (sslam_misaligned(4, kp_xy)) return SSLAM_E_INVALID;
    if (!width_ok(d)) return SSLAM_E_UNSUPPORTED;
    return launch_refine(feat, G, kp_xy, K, nullptr, (long long)n_frames * K, packed, n_blocks, d, desc, stream);
}
extern "C" int sslam_gather_refine(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed,
                                   int n_blocks, float *desc, void *stream) {
    if (!feat || !kp_xy || !packed || !desc || n_frames <= 0 || G <= 1 || K <= 0) return SSLAM_E_INVALID;
    if (((uintptr_t)feat | (uintptr_t)packed | (uintptr_t)desc) & 15) return SSLAM_E_INVALID;   // desc: stored as 16-byte vectors
    if (sslam_misaligned(4, kp_xy)) return SSLAM_E_INVALID;
    return launch_refine(feat, G, kp_xy, K, nullptr, (long long)n_frames * K, packed, n_blocks, SSLAM_D, desc, stream);
}

extern "C" long long sslam_gather_refine_workspace_bytes(int n_frames, int K) {
    if (n_frames <= 0 || K <= 0) return SSLAM_E_INVALID;
    return distinct_form(n_frames, K) ? distinct_ws(n_frames, (long long)n_frames * K).bytes : 0;
}

static int gather_refine_ws(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed, int n_blocks,
                            int d, float *desc, void *workspace, long long workspace_bytes, void *stream) {
    if (sslam_misaligned(4, workspace)) return SSLAM_E_INVALID;      // int32 words; NULL is allowed: the direct launch
    if (distinct_form(n_frames, K) && workspace &&
        workspace_bytes >= distinct_ws(n_frames, (long long)n_frames * K).bytes)
        return launch_refine_distinct(feat, n_frames, G, kp_xy, K, packed, n_blocks, d, desc, workspace, stream);
    return launch_refine(feat, G, kp_xy, K, nullptr, (long long)n_frames * K, packed, n_blocks, d, desc, stream);
}
// the workspace (sslam_gather_refine_workspace_bytes) does not depend on the width: it holds row indices only
extern "C" int sslam_gather_refine_ws_d(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed,
                                        int n_blocks, float *desc, void *workspace, long long workspace_bytes, int d, void *stream) {
    if (!feat || !kp_xy || !packed || !desc || n_frames <= 0 || G <= 1 || K <= 0) return SSLAM_E_INVALID;
    if (((uintptr_t)feat | (uintptr_t)packed | (uintptr_t)desc) & 15) return SSLAM_E_INVALID;
    if (sslam_misaligned(4, kp_xy)) return SSLAM_E_INVALID;
    if (!width_ok(d)) return SSLAM_E_UNSUPPORTED;
    return gather_refine_ws(feat, n_frames, G, kp_xy, K, packed, n_blocks, d, desc, workspace, workspace_bytes, stream);
}
extern "C" int sslam_gather_refine_ws(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *packed,
                                      int n_blocks, float *desc, void *workspace, long long workspace_bytes, void *stream) {
    if (!feat || !kp_xy || !packed || !desc || n_frames <= 0 || G <= 1 || K <= 0) return SSLAM_E_INVALID;
    if (((uintptr_t)feat | (uintptr_t)packed | (uintptr_t)desc) & 15) return SSLAM_E_INVALID;   // desc: stored as 16-byte vectors
    if (sslam_misaligned(4, kp_xy)) return SSLAM_E_INVALID;
    return gather_refine_ws(feat, n_frames, G, kp_xy, K, packed, n_blocks, SSLAM_D, desc, workspace, workspace_bytes, stream);
}

extern "C" int sslam_gather(const float *feat, int n_frames, int G, const float *kp_xy, int K, float *out, void *stream) {
    if (!feat || !kp_xy || !out || n_frames <= 0 || G <= 1 || K <= 0) return SSLAM_E_INVALID;
    if (((uintptr_t)feat | (uintptr_t)out) & 15 || sslam_misaligned(4, kp_xy)) return SSLAM_E_INVALID;
    const long long rows = (long long)n_frames * K, items = rows * (SSLAM_C / 4);
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, feat, G, kp_xy,
                       K, rows, out);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

#ifdef SSLAM_CLOCK_PROBE
extern "C" int sslam_probe_refine(unsigned long long *host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_probe_refine), sizeof(unsigned long long) * 8 * 4096) == hipSuccess ? 0 : -3;
}
#endif
