// validate.hip - checkpoint validation on the device: the statistics from which the host composes the seven loss terms and the
// five batch metrics of the reference's SemanticSLAMTrainer.validate() (train.py:451-499 -> _forward_pass :292-408 under
// no_grad, losses/self_supervised.py).  Forward only.  Three launch groups, nothing read back:
//   row_lse_kernel          per pair: lse_i = log sum_j exp(x_ij), x_ij = clamp(s_ij / T, -50, 50) - the K x K logits of
//                           DescriptorMatchingLoss.forward (self_supervised.py:58-62), never written to memory
//   edge_pool_kernel        per frame: gray -> 3 x 3 Sobel -> magnitude -> 16 x 16 block means + the frame maximum
//                           (EdgeAwarenessLoss.forward, :248-260), one pass over the fp32 image
//   val_frame_stats_kernel  per frame: the sums of the saliency terms (:186-214, :287-314), the centred sums of the edge
//                           correlation (:270-275), the per-dimension descriptor moments (:102-109)
//   val_pair_stats_kernel   per pair: MSE of the two saliency maps (:180-182), the mutual-nearest-neighbour count of
//                           _find_matches (train.py:410-449) and the cross-entropy sums over its rows
// Every sum has ONE order, fixed by the shapes alone (a lane's own elements in increasing index, then a fixed tree), so a
// frame's or a pair's results do not depend on how a sequence is cut into launches or on its place in one.
//
// row_lse_kernel is the row direction of match.hip's sim_argmax_kernel with another reduction: the same operand layout (the
// query on the lane as the B operand, 32 candidates on the accumulator rows, 132-float LDS rows, double-buffered candidate
// tiles of 64), hence the same similarity bits.  The row maximum is an INPUT (s12 of the arg-max launch; division by T > 0 and
// the clamp are monotone, so clamp(s12_i / T) = max_j x_ij): one pass, no rescaling.  Stager and the pair-naming structs are
// restated here rather than moved to a header, so that match.hip compiles from the text it had.
// Roofline: MFMA-bound like M1's row direction (K^2 * 128 * 2 FLOP per pair) plus ~32 vector instructions per similarity
// (correctly rounded division, clamp, sslam_expf).
#include "common.h"

namespace {

constexpr int QB = 128;            // queries per workgroup (32 per wave)
constexpr int CB = 64;             // candidates per stage (two MFMA tiles per wave)
constexpr int NTM = 256;           // threads per workgroup
// LDS rows are D + 4 floats (132 / 260): conflict-free b128 fragment reads

// rows x D floats -> KP8 image in LDS; load half (global -> registers) and store half (registers -> LDS), so that the next
// candidate tile is in flight during the MFMAs.  Rows beyond n_valid re-read row 0 and are stored as zeros.
template <int ROWS, int D>
struct Stager {
    static constexpr int GL = D == 128 ? 4 : 5, GM = D / 8 - 1, LDD = D + 4;      // D / 8 groups of 8 floats per row
    static constexpr int ITEMS = ROWS * (D / 8) / NTM;
    float4 lo[ITEMS], hi[ITEMS];
    bool ok[ITEMS];
    __device__ __forceinline__ void load(const float *__restrict__ src, int first, int n_valid, int tid) {
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int it = tid + NTM * i, row = it >> GL, g = it & GM;
            ok[i] = first + row < n_valid;
            const float4 *p = reinterpret_cast<const float4 *>(src + (long long)(ok[i] ? first + row : 0) * D + 8 * g);
            lo[i] = p[0];
            hi[i] = p[1];
        }
    }
    __device__ __forceinline__ void store(float *dst, int tid) const {
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int it = tid + NTM * i, row = it >> GL, g = it & GM;
            float4 ev, od;
            const bool k = ok[i];
            kp8_split(make_float4(k ? lo[i].x : 0.f, k ? lo[i].y : 0.f, k ? lo[i].z : 0.f, k ? lo[i].w : 0.f),
                      make_float4(k ? hi[i].x : 0.f, k ? hi[i].y : 0.f, k ? hi[i].z : 0.f, k ? hi[i].w : 0.f), ev, od);
            *reinterpret_cast<float4 *>(dst + row * LDD + 8 * g) = ev;
            *reinterpret_cast<float4 *>(dst + row * LDD + 8 * g + 4) = od;
        }
    }
};

// which two frames pair p names (the conventions of sslam_sim_argmax_rows[_pairs]); false = an absent pair: zero fill
struct StridedPairs {
    __device__ __forceinline__ bool frames(long long p, long long &f1, long long &f2) const {
        f1 = f2 = p;
        return true;
    }
};
struct ListedPairs {
    const int *first, *second;
    int n_bank;
    __device__ __forceinline__ bool frames(long long p, long long &f1, long long &f2) const {
        const int a = first[p], b = second[p];
        if ((unsigned)a >= (unsigned)n_bank || (unsigned)b >= (unsigned)n_bank) return false;      // -1: the documented sentinel
        f1 = a;
        f2 = b;
        return true;
    }
};

__device__ __forceinline__ float logit(float s, float temperature) {      // self_supervised.py:58-59
    return fminf(fmaxf(s / temperature, -50.0f), 50.0f);
}

// grid: (pair, query block) in the XCD-aware order of sim_argmax_kernel; 4 waves x 32 queries.  D = 256: the stage of 64 candidates
// is 2 x 65 KB of LDS and the queries 128 registers - one workgroup per CU, as in sim_argmax_kernel
template <int D, class PAIRS>
__global__ __launch_bounds__(NTM, D == 128 ? 2 : 1) void row_lse_kernel(const float *__restrict__ desc1, long long stride1, int n1,
                                                         const float *__restrict__ desc2, long long stride2, int n2,
                                                         const float *__restrict__ s12, float temperature,
                                                         float *__restrict__ lse, float *__restrict__ ce,
                                                         float *__restrict__ s00, int n_pairs, int qblocks, PAIRS pairs) {
    constexpr int LDD = D + 4;
    __shared__ __attribute__((aligned(16))) float Cs[2 * CB * LDD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const long long pair = (long long)(slot / qblocks) * 8 + xcd;
    if (pair >= n_pairs) return;
    const int q0 = (slot % qblocks) * QB;
    long long f1, f2;
    if (!pairs.frames(pair, f1, f2)) {
        const int i = q0 + tid;
        if (tid < QB && i < n1) {
            if (lse) lse[pair * n1 + i] = 0.0f;
            if (ce) ce[pair * n1 + i] = 0.0f;
        }
        if (q0 == 0 && tid == 0 && s00) s00[pair] = 0.0f;
        return;
    }
    const float *q = desc1 + f1 * stride1, *c = desc2 + f2 * stride2;
    const int nq = n1, nc = n2;

    Stager<CB, D> sc;
    sc.load(c, 0, nc, tid);
    const int qi = q0 + wave * 32 + r;
    const bool qok = qi < nq;
    float qreg[D / 2];      // this lane's query as the B operand of all D / 2 MFMA steps: step i multiplies k = 2 i + h
    {
        const float4 *qp = reinterpret_cast<const float4 *>(q + (long long)(qok ? qi : 0) * D);
        const float qm = qok ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < D / 4; i++) {
            const float4 v = qp[i];
            qreg[2 * i] = (h ? v.y : v.x) * qm;
            qreg[2 * i + 1] = (h ? v.w : v.z) * qm;
        }
    }
    const float m = logit(qok ? s12[pair * n1 + qi] : 0.0f, temperature);      // = max_j x_ij
    sc.store(Cs, tid);
    __syncthreads();

    const int nstage = (nc + CB - 1) / CB;
    float sum = 0.0f;
    for (int s = 0; s < nstage; s++) {
        if (s + 1 < nstage) sc.load(c, (s + 1) * CB, nc, tid);      // in flight during the MFMAs below
        const float *A = Cs + (s & 1) * CB * LDD + r * LDD + 4 * h;
        f32x16 acc[2];
#pragma unroll
        for (int e = 0; e < 16; e++) acc[0][e] = acc[1][e] = 0.0f;
#pragma unroll
        for (int g = 0; g < D / 8; g++) {
            // KP8 image: the float4 at 8 g + 4 h holds k = 8 g + 2 st + h, st = 0..3 -> MFMA step 4 g + st
            const f32x4 a0 = *reinterpret_cast<const f32x4 *>(A + 8 * g);
            const f32x4 a1 = *reinterpret_cast<const f32x4 *>(A + 32 * LDD + 8 * g);
#pragma unroll
            for (int st = 0; st < 4; st++) {
                acc[0] = mfma32(a0[st], qreg[4 * g + st], acc[0]);
                acc[1] = mfma32(a1[st], qreg[4 * g + st], acc[1]);
            }
        }
        // the buffer written here was last read in stage s - 1, which every wave left through the barrier below
        if (s + 1 < nstage) sc.store(Cs + ((s + 1) & 1) * CB * LDD, tid);
        if (s == 0 && qi == 0 && h == 0 && s00) s00[pair] = acc[0][0];      // S[0][0]: the padded rows' target (train.py:445)
        const bool last = s + 1 == nstage;
#pragma unroll
        for (int ct = 0; ct < 2; ct++)
#pragma unroll
            for (int e = 0; e < 16; e++) {      // j increases with (s, ct, e): this lane's candidates in increasing index
                const int j = s * CB + 32 * ct + (e & 3) + 8 * (e >> 2) + 4 * h;
                float t = sslam_expf(logit(acc[ct][e], temperature) - m);
                if (last) t = j < nc ? t : 0.0f;      // rows beyond nc of the last tile
                sum = sum + t;
            }
        __syncthreads();
    }
    const float tot = sum + __shfl_xor(sum, 32);      // the two half-waves: same query, interleaved candidate rows
    if (h == 0 && qok) {
        const float l = sslam_logf(tot);              // tot >= 1: the maximum's own term
        if (ce) ce[pair * n1 + qi] = l;
        if (lse) lse[pair * n1 + qi] = m + l;
    }
}

// ---- Sobel / pool.  One workgroup per (column segment of up to 32 cells, cell row, frame): the gray image of its 18 rows
// goes to LDS through 128-bit loads with a zero halo where the image ends (padding = 1 of F.conv2d, :252-253), then every
// thread walks columns downwards with a three-row window.
constexpr int SEG = 512;           // pixel columns per workgroup
constexpr int GW = SEG + 8;        // LDS row: gray column x of the segment at 4 + x, the halo columns at 3 and 4 + width

__global__ __launch_bounds__(256) void edge_pool_kernel(const float *__restrict__ img, int S, int G,
                                                        float *__restrict__ pooled, unsigned *__restrict__ edge_max) {
    __shared__ __attribute__((aligned(16))) float gray[18 * GW];
    __shared__ float wmax[4];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * SEG, gy = blockIdx.y;
    const long long f = blockIdx.z;
    const int W = min(SEG, S - c0);      // a multiple of 16
    const long long plane = (long long)S * S;
    const float *base = img + f * 3 * plane;
    const int w4 = W >> 2;
    for (int it = tid; it < 18 * w4; it += 256) {
        const int rr = it / w4, x4 = it - rr * w4;
        const int y = 16 * gy - 1 + rr;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < S) {
            const float *p = base + (long long)y * S + c0 + 4 * x4;
            const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + plane),
                         c = *reinterpret_cast<const float4 *>(p + 2 * plane);
            g.x = 0.299f * a.x + 0.587f * b.x + 0.114f * c.x;      // :248, left to right
            g.y = 0.299f * a.y + 0.587f * b.y + 0.114f * c.y;
            g.z = 0.299f * a.z + 0.587f * b.z + 0.114f * c.z;
            g.w = 0.299f * a.w + 0.587f * b.w + 0.114f * c.w;
        }
        *reinterpret_cast<float4 *>(gray + rr * GW + 4 + 4 * x4) = g;
    }
    if (tid < 36) {      // the two halo columns of the 18 rows
        const int rr = tid >> 1, side = tid & 1;
        const int y = 16 * gy - 1 + rr, x = side ? c0 + W : c0 - 1;
        float g = 0.0f;
        if (y >= 0 && y < S && x >= 0 && x < S) {
            const float *p = base + (long long)y * S + x;
            g = 0.299f * p[0] + 0.587f * p[plane] + 0.114f * p[2 * plane];
        }
        gray[rr * GW + (side ? 4 + W : 3)] = g;
    }
    __syncthreads();
    float mx = 0.0f;
    for (int x = tid; x < SEG; x += 256) {      // uniform trip count: the 16-lane sums below need whole waves
        float colsum = 0.0f;
        if (x < W) {
            const float *gp = gray + 3 + x;      // gp[0], gp[1], gp[2]: columns x - 1, x, x + 1 of a row
            float l0 = gp[0], m0 = gp[1], r0 = gp[2], l1 = gp[GW], m1 = gp[GW + 1], r1 = gp[GW + 2];
#pragma unroll
            for (int yy = 0; yy < 16; yy++) {
                const float l2 = gp[(yy + 2) * GW], m2 = gp[(yy + 2) * GW + 1], r2 = gp[(yy + 2) * GW + 2];
                const float gx = ((r0 - l0) + 2.0f * (r1 - l1)) + (r2 - l2);
                const float gyv = ((l2 - l0) + 2.0f * (m2 - m0)) + (r2 - r0);
                const float mag = sqrtf((gx * gx + gyv * gyv) + 1e-8f);      // :254
                colsum = colsum + mag;
                mx = fmaxf(mx, mag);
                l0 = l1; m0 = m1; r0 = r1;
                l1 = l2; m1 = m2; r1 = r2;
            }
        }
        // the 16 columns of a cell are 16 adjacent lanes
        colsum = colsum + __shfl_xor(colsum, 8);
        colsum = colsum + __shfl_xor(colsum, 4);
        colsum = colsum + __shfl_xor(colsum, 2);
        colsum = colsum + __shfl_xor(colsum, 1);
        if (x < W && (x & 15) == 0)      // adaptive_avg_pool2d to (G, G) of an image of 16 G pixels: the 16 x 16 block mean (:260)
            pooled[(f * G + gy) * G + ((c0 + x) >> 4)] = colsum * (1.0f / 256.0f);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    // mag > 0 always: the bit patterns of positive floats order like the floats, and max is order-free
    if (tid == 0) atomicMax(edge_max + f, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}

// sum over the workgroup in a fixed tree: the wave butterfly, then ((w0 + w1) + w2) + w3
__device__ __forceinline__ float block_sum(float v, float *red, int tid) {
    v = bfly64(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float block_max(float v, float *red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// one workgroup per frame; stats row: SSLAM_VAL_* slots of include/sslam_hip.h.  D: the descriptor width (128: two row-parity
// half-sums per dimension on the 256 threads; 256: one thread per dimension, all rows in increasing index)
template <int D>
__global__ __launch_bounds__(256) void val_frame_stats_kernel(const float *__restrict__ sal, const float *__restrict__ pooled,
                                                              const float *__restrict__ edge_max, const float *__restrict__ desc,
                                                              int G, int K, float *__restrict__ stats,
                                                              float *__restrict__ desc_mean, float *__restrict__ desc_m2) {
    __shared__ float red[4];
    __shared__ float part[256];
    const int tid = threadIdx.x;
    const long long f = blockIdx.x;
    const int cells = G * G;
    const float *s = sal + f * cells;
    float a = 0.f, mx = -INFINITY, dx = 0.f, dy = 0.f, hi = 0.f;
    for (int i = tid; i < cells; i += 256) {
        const float v = s[i];
        a = a + v;
        mx = fmaxf(mx, v);
        if (i % G < G - 1) dx = dx + fabsf(s[i + 1] - v);      // :300
        if (i < cells - G) dy = dy + fabsf(s[i + G] - v);      // :301
        hi = hi + (v > 0.6f ? 1.0f : 0.0f);                    // :309 (a count: exact in fp32)
    }
    float smean = block_sum(a, red, tid) / (float)cells;
    {   // one correction step: the mean of a CONSTANT map is then the constant itself, whatever the sum rounded to, so that its
        // centred sums are exactly 0 (the edge correlation of such a map is 0, as in the reference, not roundoff over roundoff)
        float r = 0.f;
        for (int i = tid; i < cells; i += 256) r = r + (s[i] - smean);
        smean = smean + block_sum(r, red, tid) / (float)cells;
    }
    mx = block_max(mx, red, tid);
    dx = block_sum(dx, red, tid);
    dy = block_sum(dy, red, tid);
    hi = block_sum(hi, red, tid);
    float *o = stats + f * SSLAM_VAL_FRAME_STATS;
    if (pooled) {
        const float *P = pooled + f * cells;
        float pa = 0.f;
        for (int i = tid; i < cells; i += 256) pa = pa + P[i];
        const float pmean = block_sum(pa, red, tid) / (float)cells;
        float A = 0.f, E = 0.f;
        for (int i = tid; i < cells; i += 256) {
            const float dp = P[i] - pmean, ds = s[i] - smean;
            A = A + dp * ds;
            E = E + dp * dp;
        }
        A = block_sum(A, red, tid);
        E = block_sum(E, red, tid);
        if (tid == 0) {
            o[SSLAM_VAL_EDGE_A] = A;
            o[SSLAM_VAL_EDGE_E] = E;
            o[SSLAM_VAL_EDGE_MEAN] = pmean;
            o[SSLAM_VAL_EDGE_MAX] = edge_max[f];
        }
    } else if (tid == 0) {
        o[SSLAM_VAL_EDGE_A] = o[SSLAM_VAL_EDGE_E] = o[SSLAM_VAL_EDGE_MEAN] = o[SSLAM_VAL_EDGE_MAX] = 0.0f;
    }
    float ss = 0.f;
    for (int i = tid; i < cells; i += 256) {
        const float ds = s[i] - smean;
        ss = ss + ds * ds;
    }
    ss = block_sum(ss, red, tid);
    if (tid == 0) {
        o[SSLAM_VAL_SAL_MEAN] = smean;
        o[SSLAM_VAL_SAL_VAR] = ss / (float)cells;      // unbiased=False, :196
        o[SSLAM_VAL_SAL_MAX] = mx;
        o[SSLAM_VAL_SAL_DX] = dx;
        o[SSLAM_VAL_SAL_DY] = dy;
        o[SSLAM_VAL_SAL_HIGH] = hi;
        o[SSLAM_VAL_SAL_SS] = ss;
        for (int i = SSLAM_VAL_EDGE_MAX + 1; i < SSLAM_VAL_FRAME_STATS; i++) o[i] = 0.0f;
    }
    if (desc) {      // per dimension: mean, then the centred sum of squares; thread = (row parity, dimension)
        constexpr int NPAR = 256 / D;      // row classes per dimension: 2 or 1
        const float *d = desc + f * (long long)K * D;
        const int dim = tid & (D - 1), par = tid >> (D == 128 ? 7 : 8);
        float t = 0.f;
        for (int k = par; k < K; k += NPAR) t = t + d[(long long)k * D + dim];
        __syncthreads();
        part[tid] = t;
        __syncthreads();
        const float mean = (NPAR == 2 ? part[dim] + part[dim + (NPAR == 2 ? D : 0)] : part[dim]) / (float)K;
        float q = 0.f;
        for (int k = par; k < K; k += NPAR) {
            const float c = d[(long long)k * D + dim] - mean;
            q = q + c * c;
        }
        __syncthreads();
        part[tid] = q;
        __syncthreads();
        if (par == 0) {
            desc_mean[f * D + dim] = mean;
            desc_m2[f * D + dim] = NPAR == 2 ? part[dim] + part[dim + (NPAR == 2 ? D : 0)] : part[dim];
        }
    }
}

// one workgroup per pair; stats row: SSLAM_VAL_PAIR_* slots
template <class PAIRS>
__global__ __launch_bounds__(256) void val_pair_stats_kernel(const float *__restrict__ sal1, const float *__restrict__ sal2, int cells,
                                                             const int *__restrict__ nn12, const int *__restrict__ nn21,
                                                             const float *__restrict__ s12, const float *__restrict__ ce,
                                                             const float *__restrict__ s00, int n1, int n2, float temperature,
                                                             float *__restrict__ stats, int *__restrict__ n_matches, PAIRS pairs) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const long long p = blockIdx.x;
    float *o = stats + p * SSLAM_VAL_PAIR_STATS;
    long long f1, f2;
    if (!pairs.frames(p, f1, f2)) {
        if (tid < SSLAM_VAL_PAIR_STATS) o[tid] = 0.0f;
        if (tid == 0) n_matches[p] = 0;
        return;
    }
    const float *sa = sal1 + f1 * cells, *sb = sal2 + f2 * cells;
    float mse = 0.f;
    for (int i = tid; i < cells; i += 256) {
        const float d = sa[i] - sb[i];
        mse = mse + d * d;
    }
    mse = block_sum(mse, red, tid) / (float)cells;      // F.mse_loss, :182
    nn12 += p * n1;
    nn21 += p * n2;
    ce += p * n1;
    float cnt = 0.f, cs = 0.f;
    for (int i = tid; i < n1; i += 256) {
        const int j = nn12[i];
        if ((unsigned)j < (unsigned)n2 && nn21[j] == i) {      // train.py:425
            cnt = cnt + 1.0f;
            cs = cs + ce[i];                                   // lse_i - x_{i, nn12(i)}: the row's cross-entropy (:62)
        }
    }
    cnt = block_sum(cnt, red, tid);
    cs = block_sum(cs, red, tid);
    if (tid == 0) {
        // a padded row (0, 0) of the trainer's match list (train.py:445): lse_0 - x_00 = ce_0 + (max_j x_0j - x_00)
        const float pad = ce[0] + (logit(s12[p * n1], temperature) - logit(s00[p], temperature));
        o[SSLAM_VAL_PAIR_REPEAT] = mse;
        o[SSLAM_VAL_PAIR_CE_SUM] = cs;
        o[SSLAM_VAL_PAIR_PAD_CE] = pad;
        o[SSLAM_VAL_PAIR_MATCHES] = cnt;
        n_matches[p] = (int)cnt;
    }
}

template <int D, class PAIRS>
int launch_row_lse(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2, int n_pairs,
                   const float *s12, float temperature, float *lse, float *ce, float *s00, void *stream, PAIRS pairs) {
    const int qb1 = (n1 + QB - 1) / QB;
    if ((long long)n_pairs * qb1 > 0x7ffffff0LL / 8) return SSLAM_E_UNSUPPORTED;
    const dim3 grid((unsigned)((n_pairs + 7) / 8 * 8 * qb1), 1, 1);
    hipLaunchKernelGGL((row_lse_kernel<D, PAIRS>), grid, dim3(NTM), 0, (hipStream_t)stream, desc1, stride1, n1, desc2, stride2, n2, s12,
                       temperature, lse, ce, s00, n_pairs, qb1, pairs);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

bool temperature_ok(float t) { return t > 0.0f && t < INFINITY; }

}  // namespace

#define SSLAM_BY_WIDTH(d_, call128_, call256_) ((d_) == 128 ? (call128_) : (d_) == 256 ? (call256_) : SSLAM_E_UNSUPPORTED)

extern "C" int sslam_row_lse_d(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2,
                               int n_pairs, const float *s12, float temperature, float *lse, float *ce, float *s00, int d, void *stream) {
    if (!desc1 || !desc2 || !s12 || (!lse && !ce) || n1 <= 0 || n2 <= 0 || n_pairs <= 0 || !temperature_ok(temperature))
        return SSLAM_E_INVALID;
    if (((uintptr_t)desc1 | (uintptr_t)desc2) & 15 || (stride1 & 3) || (stride2 & 3)) return SSLAM_E_INVALID;
    if (sslam_misaligned(4, s12, lse, ce, s00)) return SSLAM_E_INVALID;
    return SSLAM_BY_WIDTH(d,
                          launch_row_lse<128>(desc1, stride1, n1, desc2, stride2, n2, n_pairs, s12, temperature, lse, ce, s00, stream, StridedPairs{}),
                          launch_row_lse<256>(desc1, stride1, n1, desc2, stride2, n2, n_pairs, s12, temperature, lse, ce, s00, stream, StridedPairs{}));
}
extern "C" int sslam_row_lse(const float *desc1, long long stride1, int n1, const float *desc2, long long stride2, int n2,
                             int n_pairs, const float *s12, float temperature, float *lse, float *ce, float *s00, void *stream) {
    return sslam_row_lse_d(desc1, stride1, n1, desc2, stride2, n2, n_pairs, s12, temperature, lse, ce, s00, SSLAM_D, stream);
}

extern "C" int sslam_row_lse_pairs_d(const float *bank, long long frame_stride, int n_bank, int K, const int32_t *pair_first,
                                     const int32_t *pair_second, int n_pairs, const float *s12, float temperature, float *lse,
                                     float *ce, float *s00, int d, void *stream) {
    if (!bank || !pair_first || !pair_second || !s12 || (!lse && !ce) || n_bank <= 0 || K <= 0 || n_pairs <= 0 ||
        !temperature_ok(temperature))
        return SSLAM_E_INVALID;
    if (((uintptr_t)bank & 15) || (frame_stride & 3) || (((uintptr_t)pair_first | (uintptr_t)pair_second) & 3)) return SSLAM_E_INVALID;
    if (sslam_misaligned(4, s12, lse, ce, s00)) return SSLAM_E_INVALID;
    const ListedPairs lp{pair_first, pair_second, n_bank};
    return SSLAM_BY_WIDTH(d,
                          launch_row_lse<128>(bank, frame_stride, K, bank, frame_stride, K, n_pairs, s12, temperature, lse, ce, s00, stream, lp),
                          launch_row_lse<256>(bank, frame_stride, K, bank, frame_stride, K, n_pairs, s12, temperature, lse, ce, s00, stream, lp));
}
extern "C" int sslam_row_lse_pairs(const float *bank, long long frame_stride, int n_bank, int K, const int32_t *pair_first,
                                   const int32_t *pair_second, int n_pairs, const float *s12, float temperature, float *lse,
                                   float *ce, float *s00, void *stream) {
    return sslam_row_lse_pairs_d(bank, frame_stride, n_bank, K, pair_first, pair_second, n_pairs, s12, temperature, lse, ce, s00, SSLAM_D,
                                 stream);
}

extern "C" int sslam_edge_pool(const float *images_chw, int n_frames, int size, float *pooled, float *edge_max, void *stream) {
    if (!images_chw || !pooled || !edge_max || n_frames <= 0 || size <= 0) return SSLAM_E_INVALID;
    if (((uintptr_t)images_chw & 15) || sslam_misaligned(4, pooled, edge_max)) return SSLAM_E_INVALID;
    if (size % 16 || size / 16 > 65535 || n_frames > 65535) return SSLAM_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    // 0 is below the bits of every magnitude: the maximum is a 32-bit unsigned atomic max, which no order can change
    if (hipMemsetAsync(edge_max, 0, (size_t)n_frames * sizeof(float), st) != hipSuccess) return SSLAM_E_LAUNCH;
    const int G = size / 16;
    hipLaunchKernelGGL(edge_pool_kernel, dim3((unsigned)((size + SEG - 1) / SEG), (unsigned)G, (unsigned)n_frames), dim3(256), 0, st,
                       images_chw, size, G, pooled, (unsigned *)edge_max);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

extern "C" int sslam_val_frame_stats_d(const float *saliency, const float *pooled, const float *edge_max, const float *descriptors,
                                       int n_frames, int G, int K, float *stats, float *desc_mean, float *desc_m2, int d, void *stream) {
    if (!saliency || !stats || n_frames <= 0 || G <= 0 || G > 4096) return SSLAM_E_INVALID;
    if ((pooled != nullptr) != (edge_max != nullptr)) return SSLAM_E_INVALID;
    if (descriptors && (!desc_mean || !desc_m2 || K <= 0)) return SSLAM_E_INVALID;
    if (sslam_misaligned(4, saliency, pooled, edge_max, descriptors, stats, desc_mean, desc_m2)) return SSLAM_E_INVALID;      // word by word
    if (d != 128 && d != 256) return SSLAM_E_UNSUPPORTED;
    if (d == 128)
        hipLaunchKernelGGL(val_frame_stats_kernel<128>, dim3((unsigned)n_frames), dim3(256), 0, (hipStream_t)stream, saliency, pooled,
                           edge_max, descriptors, G, K, stats, desc_mean, desc_m2);
    else
        hipLaunchKernelGGL(val_frame_stats_kernel<256>, dim3((unsigned)n_frames), dim3(256), 0, (hipStream_t)stream, saliency, pooled,
                           edge_max, descriptors, G, K, stats, desc_mean, desc_m2);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}
extern "C" int sslam_val_frame_stats(const float *saliency, const float *pooled, const float *edge_max, const float *descriptors,
                                     int n_frames, int G, int K, float *stats, float *desc_mean, float *desc_m2, void *stream) {
    return sslam_val_frame_stats_d(saliency, pooled, edge_max, descriptors, n_frames, G, K, stats, desc_mean, desc_m2, SSLAM_D, stream);
}

static bool pair_stats_args_ok(const float *saliency, int G, const int32_t *nn12, const int32_t *nn21, const float *s12, const float *ce,
                               const float *s00, int n1, int n2, int n_pairs, float temperature, const float *stats,
                               const int32_t *n_matches) {
    return saliency && nn12 && nn21 && s12 && ce && s00 && stats && n_matches && G > 0 && G <= 4096 && n1 > 0 && n2 > 0 &&
           n_pairs > 0 && temperature_ok(temperature) && !sslam_misaligned(4, saliency, nn12, nn21, s12, ce, s00, stats, n_matches);
}

extern "C" int sslam_val_pair_stats(const float *saliency1, const float *saliency2, int G, const int32_t *nn12, const int32_t *nn21,
                                    const float *s12, const float *ce, const float *s00, int n1, int n2, int n_pairs,
                                    float temperature, float *stats, int32_t *n_matches, void *stream) {
    if (!pair_stats_args_ok(saliency1, G, nn12, nn21, s12, ce, s00, n1, n2, n_pairs, temperature, stats, n_matches) || !saliency2 || sslam_misaligned(4, saliency2))
        return SSLAM_E_INVALID;
    hipLaunchKernelGGL(val_pair_stats_kernel<StridedPairs>, dim3((unsigned)n_pairs), dim3(256), 0, (hipStream_t)stream, saliency1, saliency2,
                       G * G, nn12, nn21, s12, ce, s00, n1, n2, temperature, stats, n_matches, StridedPairs{});
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}

extern "C" int sslam_val_pair_stats_pairs(const float *saliency_bank, int G, int n_bank, const int32_t *pair_first,
                                          const int32_t *pair_second, const int32_t *nn12, const int32_t *nn21, const float *s12,
                                          const float *ce, const float *s00, int K, int n_pairs, float temperature, float *stats,
                                          int32_t *n_matches, void *stream) {
    if (!pair_stats_args_ok(saliency_bank, G, nn12, nn21, s12, ce, s00, K, K, n_pairs, temperature, stats, n_matches) || !pair_first ||
        !pair_second || n_bank <= 0)
        return SSLAM_E_INVALID;
    if (((uintptr_t)pair_first | (uintptr_t)pair_second) & 3) return SSLAM_E_INVALID;
    hipLaunchKernelGGL(val_pair_stats_kernel<ListedPairs>, dim3((unsigned)n_pairs), dim3(256), 0, (hipStream_t)stream, saliency_bank, saliency_bank,
                       G * G, nn12, nn21, s12, ce, s00, K, K, temperature, stats, n_matches, ListedPairs{pair_first, pair_second, n_bank});
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}
