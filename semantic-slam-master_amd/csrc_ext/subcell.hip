// subcell.hip - libsslam_ext.so: sub-cell keypoint localisation (include/sslam_ext.h states the arithmetic operation by
// operation; tests/subcell_ref.py restates it in numpy float32).  One thread per keypoint: the selection kernel left the dense
// saliency map in device memory, and a keypoint needs five words of it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sslam_ext.h"

namespace {

constexpr int NT = 256;

long long g_launches = 0;   // diagnostic launch counter (sslx_launch_count): relaxed atomic adds, the library's only mutable state

// one axis of the separable three-point parabola: the offset in cells, `refined` set when it is kept
__device__ __forceinline__ float axis_offset(float c, float m, float p, bool border, bool &refined) {
    const float a = c - m, b = c - p;
    const float den = a + b;
    const float off = (a - b) / (den + den);
    refined = !border && (a >= 0.0f && b >= 0.0f) && (den > 0.0f) && (off >= -0.5f && off <= 0.5f);
    return refined ? off : 0.0f;
}

__global__ __launch_bounds__(NT) void subcell_kernel(const float *__restrict__ sal, int G, const int *__restrict__ idx, int K, int total,
                                                      float2 *__restrict__ kp_xy_sub, float2 *__restrict__ kp_pixel_sub,
                                                      int *__restrict__ flags) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= total) return;
    const int n = G * G;
    const int cell = idx[t];
    float fx = 0.0f, fy = 0.0f;
    int fl = SSLX_FLAG_RANGE;
    if (cell >= 0 && cell < n) {
        const float *s = sal + (t / K) * (long long)n;
        const int y = cell / G, x = cell - y * G;
        const bool bx = x == 0 || x == G - 1, by = y == 0 || y == G - 1;
        // a border axis loads the cell itself in place of the neighbour it lacks: five loads in flight, none out of the frame
        const float c = s[cell];
        const float xm = s[bx ? cell : cell - 1], xp = s[bx ? cell : cell + 1];
        const float ym = s[by ? cell : cell - G], yp = s[by ? cell : cell + G];
        bool rx, ry;
        const float ox = axis_offset(c, xm, xp, bx, rx), oy = axis_offset(c, ym, yp, by, ry);
        fx = (float)x + ox;
        fy = (float)y + oy;
        fl = (rx ? SSLX_FLAG_X : 0) | (ry ? SSLX_FLAG_Y : 0);
    }
    kp_xy_sub[t] = make_float2(fx, fy);
    kp_pixel_sub[t] = make_float2(fx * 16.0f + 8.0f, fy * 16.0f + 8.0f);
    flags[t] = fl;
}

inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int sslx_version(void) { return 100; }
extern "C" const char *sslx_arch(void) { return "gfx950"; }
extern "C" long long sslx_launch_count(void) { return __atomic_load_n(&g_launches, __ATOMIC_RELAXED); }

extern "C" int sslx_subcell_keypoints(const float *sal, int n_frames, int G, const int32_t *idx, int K, float *kp_xy_sub,
                                      float *kp_pixel_sub, int32_t *flags, void *stream) {
    if (!sal || !idx || !kp_xy_sub || !kp_pixel_sub || !flags || n_frames <= 0 || G <= 0 || K <= 0) return SSLAM_E_INVALID;
    if (misaligned(sal, 4) || misaligned(idx, 4) || misaligned(kp_xy_sub, 8) || misaligned(kp_pixel_sub, 8) || misaligned(flags, 4))
        return SSLAM_E_INVALID;
    if (G > 64 || K > SSLX_SUBCELL_MAX_K) return SSLAM_E_UNSUPPORTED;      // 64 * 64 = SSLX_SUBCELL_MAX_CELLS
    const long long total = (long long)n_frames * K;
    if (total > 0x7fffffffLL) return SSLAM_E_UNSUPPORTED;
    const unsigned blocks = (unsigned)((total + NT - 1) / NT);
    hipLaunchKernelGGL(subcell_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, sal, G, (const int *)idx, K, (int)total,
                       reinterpret_cast<float2 *>(kp_xy_sub), reinterpret_cast<float2 *>(kp_pixel_sub), (int *)flags);
    if (hipGetLastError() != hipSuccess) return SSLAM_E_LAUNCH;
    __atomic_fetch_add(&g_launches, 1, __ATOMIC_RELAXED);      // a launch that failed is not counted
    return SSLAM_OK;
}
