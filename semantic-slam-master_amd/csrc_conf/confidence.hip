// confidence.hip - libsslam_conf.so: the keypoint confidence head (include/sslam_conf.h states the arithmetic operation by
// operation; tests/confidence_ref.py restates it in numpy).  Replaces UncertaintyEstimator.forward and the selection rule of
// filter_keypoints_by_confidence (reference semantic-slam/models/uncertainty_estimator.py:46-67, :123-183).
//
// One workgroup (4 waves) owns 32 keypoint rows for the whole chain: fill ([gathered feature | descriptor], KP8 order, LDS) ->
// Linear(384 + D, 128) + ReLU -> Linear(128, 64) + ReLU -> Linear(64, 1) -> sigmoid (a subnormal result written as 0).
// As in csrc/refine.hip the products are evaluated TRANSPOSED (weight fragment = MFMA A operand, activation rows = B operand), so a lane's accumulators hold one row and
// the ReLU works on registers; the packed weights (L2-resident) are fetched by buffer loads at scalar offsets, a ring of eight
// k-groups, and are not staged in LDS.  The first layer is 4 waves x 32 columns; the second (1/8 of the work) runs on two waves;
// the last is a 64-term chain on the vector pipe, one lane per row.  The hidden tiles re-use the input tile's LDS.
// Roofline: 2 * ((384 + D) * 128 + 128 * 64 + 64) FLOP per row (147 584 at D = 128) against 1.5 KB + 4 D bytes in and 4 bytes out.
#include "../csrc/common.h"
#include "../csrc/gather_taps.h"

#include "../../include/sslam_conf.h"

namespace {

constexpr int RM = SSLC_TILE_ROWS;      // rows per workgroup
constexpr int NTHR = 256;
constexpr int N1 = SSLC_HIDDEN_DIM, N2 = SSLC_HIDDEN_DIM / 2;
constexpr int LD1 = N1 + 4;             // row stride of the first hidden tile (KP8 order)
constexpr int LD2 = N2 + 1;             // row stride of the second hidden tile (natural order, read one row per lane)

long long g_launches = 0;   // diagnostic launch counter (sslc_launch_count): relaxed atomic adds, the library's only mutable state

struct ConfArgs {
    const float *packed;
    sslc_confidence_layout_t lay;
};

// This wave's 32 rows x 32 columns (columns 32 wn .. 32 wn + 31 of the layer's N) = bias + H(32 x 8 KG) . W^T, one fma chain per
// output in increasing k.  H: LDS tile in KP8 order, row stride LD.  Accumulator e of lane (r, h) is row r, column
// 32 wn + crow(e, h).  Weight fragments straight from global memory, a ring of eight k-groups; the refills are unconditional
// (clamped index) so that the compiler can count the loads in flight (csrc/refine.hip, gemm_lds).
template <int N, int KG, int LD>
__device__ __forceinline__ f32x16 gemm_tile(const float *H, __amdgpu_buffer_rsrc_t wrs, int w_off, const float *__restrict__ bias,
                                            int lane, int wn) {
    constexpr int RING = 8;     // k-groups in flight + 1: a step is only four MFMAs (256 cycles), so the ring is deep
    static_assert(KG % RING == 0, "the loop takes one turn of the ring per trip");
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + wn * 32 + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; i++) acc[4 * q + i] = bv[i];
    }
    // lane's fragment of k-group g: 16 B at ((g * N + n) * 8 + 4 h) floats, n = 32 wn + r
    const int loff = ((wn * 32 + r) * 2 + h) * 16;
    const float *A = H + r * LD + 4 * h;
    f32x4 b[RING];
#define LOAD_B(g) __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, loff, w_off + (g) * N * 32, 0))
#pragma unroll
    for (int u = 0; u < RING - 1; u++) b[u] = LOAD_B(u);
    f32x4 an = *reinterpret_cast<const f32x4 *>(A);
#pragma unroll 1
    for (int g = 0; g < KG; g += RING) {
#pragma unroll
        for (int u = 0; u < RING; u++) {
            b[(u + RING - 1) % RING] = LOAD_B(min(g + u + RING - 1, KG - 1));
            __builtin_amdgcn_sched_barrier(0);
            const f32x4 a = an;
            an = *reinterpret_cast<const f32x4 *>(A + 8 * min(g + u + 1, KG - 1));
#pragma unroll
            for (int st = 0; st < 4; st++) acc = mfma32(b[u][st], a[st], acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef LOAD_B
    return acc;
}

__device__ __forceinline__ float relu(float v) { return v > 0.0f ? v : 0.0f; }

// feat != nullptr: the features are gathered at kp_xy (the gather form); else they are rows of x_in (the rows form).
// Two workgroups share a CU at D = 128 (66 KB of LDS each); the 82 KB tile of D = 256 leaves room for one.
template <int D>
__global__ __launch_bounds__(NTHR, D == 128 ? 2 : 1) void confidence_kernel(const float *__restrict__ feat, int G, const float *__restrict__ kp_xy,
                                                              int K, const float *__restrict__ x_in, const float *__restrict__ desc,
                                                              long long rows, ConfArgs args, float *__restrict__ conf) {
    constexpr int K1 = SSLAM_C + D;     // input width
    constexpr int LDH = K1 + 4;         // input row stride (floats)
    static_assert(RM * LD1 + RM * LD2 <= RM * LDH, "the hidden tiles fit the input tile");
    __shared__ __attribute__((aligned(16))) float smem[RM * LDH];
    float *H = smem, *H1 = smem, *H2 = smem + RM * LD1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    // XCD-aware order (csrc/refine.hip): workgroup b runs on XCD b % 8; every XCD takes one contiguous range of row tiles, so that
    // the tiles gathering from one frame's feature map share that XCD's L2
    long long R0;
    {
        const int n_tiles = gridDim.x, b = blockIdx.x, q = n_tiles / 8, rem = n_tiles % 8, x = b % 8;
        R0 = (long long)((x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + b / 8) * RM;
    }
    const float *pk = args.packed;
    const sslc_confidence_layout_t &L = args.lay;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pk), 0, (int)(L.total * 4), 0x00020000);

    // ---- fill the tile: thread (row, part) moves the 8-float chunks j * 8 + part, 64 contiguous floats per row and step -----
    {
        const int row = tid >> 3, part = tid & 7;
        long long R = R0 + row;
        if (R > rows - 1) R = rows - 1;     // a ragged last tile reads the last row again; only rows < `rows` are written
        float *dst = H + row * LDH;
        if (feat) {
            const long long f = R / K;
            const Taps t = make_taps(feat + f * G * G * SSLAM_C, G, kp_xy[2 * R], kp_xy[2 * R + 1]);
#pragma unroll
            for (int j = 0; j < SSLAM_C / 64; j++) {
                const int c0 = 8 * (j * 8 + part);
                float4 ev, od;
                kp8_split(blend4(t, c0), blend4(t, c0 + 4), ev, od);
                *reinterpret_cast<float4 *>(dst + c0) = ev;
                *reinterpret_cast<float4 *>(dst + c0 + 4) = od;
            }
        } else {
            const float *src = x_in + R * SSLAM_C;
#pragma unroll
            for (int j = 0; j < SSLAM_C / 64; j++) {
                const int c0 = 8 * (j * 8 + part);
                float4 ev, od;
                kp8_split(*reinterpret_cast<const float4 *>(src + c0), *reinterpret_cast<const float4 *>(src + c0 + 4), ev, od);
                *reinterpret_cast<float4 *>(dst + c0) = ev;
                *reinterpret_cast<float4 *>(dst + c0 + 4) = od;
            }
        }
        const float *dsrc = desc + R * D;
#pragma unroll
        for (int j = 0; j < D / 64; j++) {
            const int c0 = 8 * (j * 8 + part);
            float4 ev, od;
            kp8_split(*reinterpret_cast<const float4 *>(dsrc + c0), *reinterpret_cast<const float4 *>(dsrc + c0 + 4), ev, od);
            *reinterpret_cast<float4 *>(dst + SSLAM_C + c0) = ev;
            *reinterpret_cast<float4 *>(dst + SSLAM_C + c0 + 4) = od;
        }
    }
    __syncthreads();

    // ---- mlp.0 + ReLU: wave wn owns the hidden columns 32 wn .. 32 wn + 31 --------------------------------------------------
    const f32x16 a1 = gemm_tile<N1, K1 / 8, LDH>(H, wrs, (int)L.w1 * 4, pk + L.b1, lane, wave);
    __syncthreads();        // every wave has finished reading the input tile: the hidden tile takes its place
    {
        float *dst = H1 + r * LD1 + wave * 32;
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int i = 0; i < 4; i++) dst[8 * q + kp8(4 * h + i)] = relu(a1[4 * q + i]);
    }
    __syncthreads();

    // ---- mlp.2 + ReLU: 64 columns, waves 0 and 1 (a chain cannot be split over k; giving the layer to waves 2 and 3 in every
    // other workgroup, so that co-resident workgroups load different SIMDs, measured no gain: 488.9 against 487.3 us) ---------
    if (wave < 2) {
        const f32x16 a2 = gemm_tile<N2, N1 / 8, LD1>(H1, wrs, (int)L.w2 * 4, pk + L.b2, lane, wave);
        float *dst = H2 + r * LD2 + wave * 32 + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int i = 0; i < 4; i++) dst[8 * q + i] = relu(a2[4 * q + i]);
    }
    __syncthreads();

    // ---- mlp.4 + sigmoid: one lane per row ----------------------------------------------------------------------------------
    if (tid < RM && R0 + tid < rows) {
        const float *w3 = pk + L.w3, *hr = H2 + tid * LD2;
        float acc = pk[L.b3];
#pragma unroll 16
        for (int k = 0; k < N2; k++) acc = __builtin_fmaf(hr[k], w3[k], acc);
        // no subnormal confidence: the canonical sigmoid's floor, 1 / (1 + expf_c(88)) = 6.05e-39, is written as +0.0f - a saturated
        // negative logit gives exactly 0, as a saturated positive one gives exactly 1
        const float c = sslam_sigmoid(acc);
        conf[R0 + tid] = c < SSLC_CONF_MIN ? 0.0f : c;
    }
}

// ---- the per-frame filter -----------------------------------------------------------------------------------------------------
constexpr int FN = 256;     // threads of a frame's workgroup; thread t owns the slots t * per .. (t + 1) * per - 1, per <= 16

__global__ __launch_bounds__(FN) void filter_kernel(const float *__restrict__ conf, int K, float threshold, int *__restrict__ slot,
                                                    int *__restrict__ count, float *__restrict__ conf_out) {
    __shared__ float c[SSLC_FILTER_MAX_K];
    __shared__ int scan[FN];
    __shared__ float best_v[FN];
    __shared__ int best_i[FN];
    __shared__ int last_kept;
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * K;
    for (int k = tid; k < K; k += FN) c[k] = conf[base + k];
    __syncthreads();
    const int per = (K + FN - 1) / FN, k0 = min(tid * per, K), k1 = min(k0 + per, K);
    int kept = 0, bi = K;
    float bv = -__builtin_inff();
    for (int k = k0; k < k1; k++) {
        const float v = c[k];
        kept += v >= threshold ? 1 : 0;
        const float w = v == v ? v : -__builtin_inff();     // a NaN is never the largest
        if (bi == K || w > bv) { bv = w; bi = k; }
    }
    scan[tid] = kept;
    best_v[tid] = bv;
    best_i[tid] = bi;
    __syncthreads();
    // inclusive integer prefix sum over the threads, and the arg-max (the lowest slot on equality), by doubling
    for (int o = 1; o < FN; o <<= 1) {
        const int add = tid >= o ? scan[tid - o] : 0;
        float ov = bv;
        int oi = bi;
        if (tid + o < FN) { ov = best_v[tid + o]; oi = best_i[tid + o]; }
        __syncthreads();
        scan[tid] += add;
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        best_v[tid] = bv;
        best_i[tid] = bi;
        __syncthreads();
    }
    const int total = scan[FN - 1], off = scan[tid] - kept;
    if (total == 0) {
        // keep the frame's largest confidence alone (best_i[0]: thread 0 has folded every thread's candidate)
        const int a = best_i[0];
        for (int j = tid; j < K; j += FN) {
            slot[base + j] = a;
            conf_out[base + j] = j == 0 ? c[a] : 0.0f;
        }
        if (tid == 0) count[blockIdx.x] = 1;
        return;
    }
    int j = off;
    for (int k = k0; k < k1; k++)
        if (c[k] >= threshold) {
            slot[base + j] = k;
            conf_out[base + j] = c[k];
            if (j == total - 1) last_kept = k;
            j++;
        }
    __syncthreads();
    const int last = last_kept;
    for (int p = total + tid; p < K; p += FN) {
        slot[base + p] = last;
        conf_out[base + p] = 0.0f;
    }
    if (tid == 0) count[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void take_rows_kernel(const unsigned *__restrict__ src, const int *__restrict__ slot, int K, int width,
                                                         long long total, unsigned *__restrict__ dst) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;      // one word of dst
    if (t >= total) return;
    const long long row = t / width;
    const int w = (int)(t - row * width);
    const long long f = row / K;
    const int s = slot[row];
    dst[t] = (s >= 0 && s < K) ? src[(f * K + s) * width + w] : 0u;
}

inline bool width_ok(int d) { return d == 128 || d == 256; }

int launch_confidence(const float *feat, int G, const float *kp_xy, int K, const float *x, const float *desc, long long rows, int D,
                      const float *packed, float *conf, void *stream) {
    ConfArgs a;
    a.packed = packed;
    if (sslc_confidence_layout(SSLC_DINO_DIM, D, SSLC_HIDDEN_DIM, &a.lay) != SSLAM_OK) return SSLAM_E_UNSUPPORTED;
    const unsigned grid = (unsigned)((rows + RM - 1) / RM);
    if (D == 128)
        hipLaunchKernelGGL(confidence_kernel<128>, dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, feat, G, kp_xy, K, x, desc, rows, a, conf);
    else
        hipLaunchKernelGGL(confidence_kernel<256>, dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, feat, G, kp_xy, K, x, desc, rows, a, conf);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}

}  // namespace

extern "C" int sslc_version(void) { return 100; }
extern "C" const char *sslc_arch(void) { return "gfx950"; }
extern "C" long long sslc_launch_count(void) { return __atomic_load_n(&g_launches, __ATOMIC_RELAXED); }

extern "C" int sslc_confidence_layout(int dino_dim, int descriptor_dim, int hidden_dim, sslc_confidence_layout_t *L) {
    if (!L || dino_dim <= 0 || descriptor_dim <= 0 || hidden_dim <= 0) return SSLAM_E_INVALID;
    if (dino_dim != SSLC_DINO_DIM || !width_ok(descriptor_dim) || hidden_dim != SSLC_HIDDEN_DIM) return SSLAM_E_UNSUPPORTED;
    long long off = 0;
    auto take = [&](long long n) { const long long o = off; off += (n + 3) / 4 * 4; return o; };
    L->d = descriptor_dim;
    L->w1 = take((long long)N1 * (dino_dim + descriptor_dim));
    L->b1 = take(N1);
    L->w2 = take((long long)N2 * N1);
    L->b2 = take(N2);
    L->w3 = take(N2);
    L->b3 = take(1);
    L->total = off;
    return SSLAM_OK;
}

extern "C" int sslc_confidence_pack_host(const float *const *w, int dino_dim, int descriptor_dim, int hidden_dim, float *out) {
    sslc_confidence_layout_t L;
    if (!w || !out) return SSLAM_E_INVALID;
    for (int i = 0; i < 6; i++)
        if (!w[i]) return SSLAM_E_INVALID;
    if (const int rc = sslc_confidence_layout(dino_dim, descriptor_dim, hidden_dim, &L)) return rc;
    for (long long i = 0; i < L.total; i++) out[i] = 0.0f;
    // w (n_out, k_in) -> [k-group = k / 8][n][8 floats in KP8 order]: the MFMA fragment order of sslam_pack_linear_host
    auto pack = [&](const float *src, int n_out, int k_in, float *dst) {
        for (int n = 0; n < n_out; n++)
            for (int k = 0; k < k_in; k++) dst[((long long)(k / 8) * n_out + n) * 8 + kp8(k % 8)] = src[(long long)n * k_in + k];
    };
    auto cp = [&](long long off, const float *src, int n) { for (int i = 0; i < n; i++) out[off + i] = src[i]; };
    pack(w[0], N1, dino_dim + descriptor_dim, out + L.w1);
    cp(L.b1, w[1], N1);
    pack(w[2], N2, N1, out + L.w2);
    cp(L.b2, w[3], N2);
    cp(L.w3, w[4], N2);
    cp(L.b3, w[5], 1);
    return SSLAM_OK;
}

extern "C" int sslc_confidence_rows(const float *x, const float *desc, long long rows, int D, const float *packed, float *conf,
                                    void *stream) {
    if (!x || !desc || !packed || !conf || rows <= 0) return SSLAM_E_INVALID;
    if (sslam_misaligned(16, x, desc, packed) || sslam_misaligned(4, conf)) return SSLAM_E_INVALID;
    if (!width_ok(D) || rows > 0x7fffffffLL) return SSLAM_E_UNSUPPORTED;
    return launch_confidence(nullptr, 0, nullptr, 1, x, desc, rows, D, packed, conf, stream);
}

extern "C" int sslc_gather_confidence(const float *feat, int n_frames, int G, const float *kp_xy, int K, const float *desc, int D,
                                      const float *packed, float *conf, void *stream) {
    if (!feat || !kp_xy || !desc || !packed || !conf || n_frames <= 0 || G <= 1 || K <= 0) return SSLAM_E_INVALID;
    if (sslam_misaligned(16, feat, desc, packed) || sslam_misaligned(4, kp_xy, conf)) return SSLAM_E_INVALID;
    const long long rows = (long long)n_frames * K;
    if (!width_ok(D) || rows > 0x7fffffffLL) return SSLAM_E_UNSUPPORTED;
    return launch_confidence(feat, G, kp_xy, K, nullptr, desc, rows, D, packed, conf, stream);
}

extern "C" int sslc_confidence_filter(const float *conf, int n_frames, int K, float threshold, int32_t *slot, int32_t *count,
                                      float *conf_out, void *stream) {
    if (!conf || !slot || !count || !conf_out || n_frames <= 0 || K <= 0) return SSLAM_E_INVALID;
    if (sslam_misaligned(4, conf, slot, count, conf_out)) return SSLAM_E_INVALID;
    if ((const void *)conf == (const void *)slot || (const void *)conf == (const void *)count || conf == conf_out) return SSLAM_E_INVALID;
    if (K > SSLC_FILTER_MAX_K) return SSLAM_E_UNSUPPORTED;
    hipLaunchKernelGGL(filter_kernel, dim3((unsigned)n_frames), dim3(FN), 0, (hipStream_t)stream, conf, K, threshold, (int *)slot,
                       (int *)count, conf_out);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);
    return SSLAM_OK;
}

extern "C" int sslc_take_rows(const void *src, const int32_t *slot, int n_frames, int K, int width, void *dst, void *stream) {
    if (!src || !slot || !dst || n_frames <= 0 || K <= 0 || width <= 0) return SSLAM_E_INVALID;
    if (sslam_misaligned(4, src, slot, dst) || src == dst) return SSLAM_E_INVALID;
    const long long nk = (long long)n_frames * K;                   // judged first: nk * width then fits 64 bits
    if (nk > 0x7fffffffLL || nk * width > 0x7fffffffLL) return SSLAM_E_UNSUPPORTED;
    const long long total = nk * width;
    hipLaunchKernelGGL(take_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned *)src,
                       (const int *)slot, K, width, total, (unsigned *)dst);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);
    return SSLAM_OK;
}
