// rank.hip - the step the reference's callers take after a matcher: rank a pair's match list by its value and keep the best
// `best` rows (visualize_matches_sequence.py:224-225: np.argsort(-match_quality)[:max_matches]; visualize_matches.py:150-151:
// sorted(matches, key=similarity, reverse=True)[:max_matches]).  On the device, so that a consumer moves `best` rows per pair
// and not K, and so that a captured step can rank without its count ever reaching the host.
//
// The order: better value first, equal values in ascending input slot.  Better is larger, or smaller with `ascending`
// (M4's value is a cosine distance).  -0.0f == +0.0f; NaN rows come last in either direction, in slot order.  That is the
// reference's stable M2 order, and one of the orders its M1 argsort may give - the only one where the values are distinct.
//
// One 64-bit key per live slot: the high word a monotone unsigned image of value + 0.0f (complemented when ascending, 0 for a
// NaN), the low word ~slot.  The keys of a pair are pairwise distinct and every live key is above the padding key 0, so sorting
// them descending has ONE result whatever network sorts them: the output is a function of the inputs alone.
#include "common.h"

namespace {

constexpr int RANK_MAX_N1 = SSLAM_RANK_MAX_N1;      // 32 KB of keys in LDS (the precedent: DISTINCT_MAX_K in refine.hip)

__device__ __forceinline__ unsigned long long rank_key(float v, int slot, int ascending) {
    const unsigned u = __float_as_uint(v + 0.0f);                       // -0.0f + 0.0f = +0.0f: the two zeros get one image
    unsigned m = (u >> 31) ? ~u : (u | 0x80000000u);                    // larger float <=> larger m; -inf -> 0x007fffff
    if (ascending) m = ~m;                                              // +inf -> 0x007fffff: a number's image is never 0
    if (v != v) m = 0u;
    return ((unsigned long long)m << 32) | (unsigned)~(unsigned)slot;   // ~slot >= 0xfffff000: a live key is never 0
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long k, int j) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, j);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), j);
    return ((unsigned long long)hi << 32) | lo;
}

// steps j = j0, j0 / 2, .. 1 (j0 <= 32) of merge size k on the element e this lane holds: the partner e ^ j is lane ^ j of the
// same wave.  The whole network sorts DESCENDING: the block of e is descending where (e & k) == 0, and in a descending block the
// lower index keeps the larger key.
__device__ __forceinline__ unsigned long long wave_steps(unsigned long long key, int e, int k, int j0) {
    for (int j = j0; j >= 1; j >>= 1) {
        const unsigned long long other = shfl_xor_u64(key, j);
        const bool keep_max = ((e & k) == 0) == ((e & j) == 0);
        key = keep_max ? (key > other ? key : other) : (key < other ? key : other);
    }
    return key;
}

// one workgroup per pair.  LDS: max(64, next power of two >= n1) keys.
__global__ __launch_bounds__(256) void match_rank_kernel(const long long *__restrict__ matches, const float *__restrict__ value,
                                                          const int *__restrict__ count, int n1, int best, int ascending,
                                                          long long *__restrict__ out_matches, float *__restrict__ out_value,
                                                          int *__restrict__ out_count, int *__restrict__ out_slot) {
    extern __shared__ unsigned long long keys[];
    const int tid = threadIdx.x;
    const long long p = blockIdx.x;
    matches += p * n1 * 2;
    value += p * n1;
    out_matches += p * best * 2;
    out_value += p * best;
    if (out_slot) out_slot += p * best;
    int c = count[p];                                  // read once; the arrays need not come from a finalize kernel:
    c = c < 0 ? 0 : (c > n1 ? n1 : c);                 // never index outside them
    const int kept = c < best ? c : best;
    int P = 64;                                        // the sort size: whole waves, a power of two >= c
    while (P < c) P <<= 1;

    if (c > 0) {
        // keys in, and every merge size up to 64 on registers: element e = chunk * 256 + tid sits in lane e & 63 of its wave
        for (int e = tid; e < P; e += 256) {           // P is a multiple of 64: a wave is in this loop with all lanes or none
            unsigned long long key = e < c ? rank_key(value[e], e, ascending) : 0ull;
            for (int k = 2; k <= 64; k <<= 1) key = wave_steps(key, e, k, k >> 1);
            keys[e] = key;
        }
        for (int k = 128; k <= P; k <<= 1) {
            for (int j = k >> 1; j >= 64; j >>= 1) {   // exchange distances that leave the wave: through LDS, one thread per couple
                __syncthreads();
                for (int t = tid; t < (P >> 1); t += 256) {
                    const int i = 2 * t - (t & (j - 1)), l = i + j;
                    const unsigned long long a = keys[i], b = keys[l];
                    if ((a < b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[l] = a;
                    }
                }
            }
            __syncthreads();
            for (int e = tid; e < P; e += 256) keys[e] = wave_steps(keys[e], e, k, 32);
        }
        __syncthreads();
    }

    if (tid == 0) out_count[p] = kept;
    for (int r = tid; r < best; r += 256) {
        long long m0 = 0, m1 = 0;
        float v = 0.f;
        int slot = 0;
        if (r < kept) {
            slot = (int)~(unsigned)keys[r];            // < c by construction: the first c keys are the live ones
            m0 = matches[2 * slot];
            m1 = matches[2 * slot + 1];
            v = value[slot];
        }
        out_matches[2 * r] = m0;                       // rows kept .. best - 1 are zeroed, as the finalize kernels zero their tails
        out_matches[2 * r + 1] = m1;
        out_value[r] = v;
        if (out_slot) out_slot[r] = slot;
    }
}

}  // namespace

extern "C" int sslam_match_rank(const int64_t *matches, const float *value, const int32_t *count, int n1, int n_pairs, int best,
                                int ascending, int64_t *out_matches, float *out_value, int32_t *out_count, int32_t *out_slot,
                                void *stream) {
    if (!matches || !value || !count || !out_matches || !out_value || !out_count || n1 <= 0 || n_pairs <= 0 || best <= 0 || best > n1)
        return SSLAM_E_INVALID;
    if (ascending != 0 && ascending != 1) return SSLAM_E_INVALID;
    // read and written element by element: the match rows int64, everything else 4-byte words
    if (sslam_misaligned(8, matches, out_matches) || sslam_misaligned(4, value, count, out_value, out_count, out_slot)) return SSLAM_E_INVALID;
    const void *ins[3] = {matches, value, count}, *outs[4] = {out_matches, out_value, out_count, out_slot};
    for (const void *o : outs)
        for (const void *in : ins)
            if (o && o == in) return SSLAM_E_INVALID;      // no output may start where an input starts
    if (n1 > RANK_MAX_N1) return SSLAM_E_UNSUPPORTED;
    int P = 64;
    while (P < n1) P <<= 1;
    hipLaunchKernelGGL(match_rank_kernel, dim3((unsigned)n_pairs), dim3(256), (size_t)P * sizeof(unsigned long long), (hipStream_t)stream,
                       (const long long *)matches, value, count, n1, best, ascending, (long long *)out_matches, out_value, out_count,
                       out_slot);
    SSLAM_CHECK_LAUNCH();
    return SSLAM_OK;
}
