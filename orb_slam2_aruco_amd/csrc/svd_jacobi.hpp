// svd_jacobi.hpp -- cv::SVD for CV_32F as OpenCV 3.4 computes it (its one-sided Jacobi: double sums of float products, float rotations,
// FLT_EPSILON * 2), per lane and in registers.  Shared by initializer.hip (16 x 9, 9 x 8, 3 x 3 and the 4 x 4 of Triangulate) and
// new_map_points.hip (the 4 x 4 of CreateNewMapPoints).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace orbfe {

// ---------------------------------------------------------------- OpenCV 3.4 restated (device) --
struct CvRng {
    uint64_t state;
    __device__ explicit CvRng(uint64_t s) : state(s ? s : 0xffffffffull) {}
    __device__ unsigned next()
    {
        state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
        return (unsigned)state;
    }
};

// JacobiSVDImpl_<float> (modules/core/src/lapack.cpp) on At = the n x m transposed input, n1 rows of storage for U.
// W: singular values (descending); Vt: n x n; At rows 0..n1-1: U^T when WANT_U.  Loops over compile-time bounds: registers only.
template <int M, int N, int N1, bool WANT_U>
__device__ __forceinline__ void svd_jacobi(float (&At)[N1][M], float (&Wout)[N], float (&Vt)[N][N])
{
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    double W[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd += (double)At[i][k] * At[i][k];
        W[i] = sd;
#pragma unroll
        for (int k = 0; k < N; k++) Vt[i][k] = 0;
        Vt[i][i] = 1;
    }
    const int max_iter = M > 30 ? M : 30;
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < N - 1; i++)
#pragma unroll
            for (int j = i + 1; j < N; j++) {
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < M; k++) p += (double)At[i][k] * At[j][k];
                if (fabs(p) <= eps * sqrt((double)a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float t0 = c * At[i][k] + s * At[j][k];
                    const float t1 = -s * At[i][k] + c * At[j][k];
                    At[i][k] = t0;
                    At[j][k] = t1;
                    a += (double)t0 * t0;
                    b += (double)t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const float t0 = c * Vt[i][k] + s * Vt[j][k];
                    const float t1 = -s * Vt[i][k] + c * Vt[j][k];
                    Vt[i][k] = t0;
                    Vt[j][k] = t1;
                }
            }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd += (double)At[i][k] * At[i][k];
        W[i] = sqrt(sd);
    }
    // selection sort, descending; the swap of rows i and j is written as predicated swaps with every candidate row
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < N; k++)
            if (wj < W[k]) { j = k; wj = W[k]; }
#pragma unroll
        for (int r = i + 1; r < N; r++)
            if (r == j) {
                const double tw = W[i]; W[i] = W[r]; W[r] = tw;
#pragma unroll
                for (int k = 0; k < M; k++) { const float t = At[i][k]; At[i][k] = At[r][k]; At[r][k] = t; }
#pragma unroll
                for (int k = 0; k < N; k++) { const float t = Vt[i][k]; Vt[i][k] = Vt[r][k]; Vt[r][k] = t; }
            }
    }
#pragma unroll
    for (int i = 0; i < N; i++) Wout[i] = (float)W[i];
    if (!WANT_U) return;
    CvRng rng(0x12345678);
#pragma unroll
    for (int i = 0; i < N1; i++) {
        double sd = i < N ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / M);
#pragma unroll
            for (int k = 0; k < M; k++) At[i][k] = (rng.next() & 256) != 0 ? val0 : -val0;
            for (int it2 = 0; it2 < 2; it2++) {
#pragma unroll
                for (int j = 0; j < i; j++) {
                    sd = 0;
#pragma unroll
                    for (int k = 0; k < M; k++) sd += At[i][k] * At[j][k];
                    float asum = 0;
#pragma unroll
                    for (int k = 0; k < M; k++) {
                        const float t = (float)(At[i][k] - sd * At[j][k]);
                        At[i][k] = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
#pragma unroll
                    for (int k = 0; k < M; k++) At[i][k] *= asum;
                }
            }
            sd = 0;
#pragma unroll
            for (int k = 0; k < M; k++) sd += (double)At[i][k] * At[i][k];
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
#pragma unroll
        for (int k = 0; k < M; k++) At[i][k] *= s;
    }
}

} // namespace orbfe
