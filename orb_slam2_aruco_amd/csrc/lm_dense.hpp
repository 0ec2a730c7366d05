// lm_dense.hpp -- what the two g2o restatements on the device with a dense system (pose_optimizer.hip: SE3Quat, 6 DoF;
// sim3_optimizer.hip: Sim3, 7 DoF) share: Eigen's quaternion pieces, the projection error, the Huber kernel, and the dense
// Levenberg-Marquardt step templated on the dimension D -- an edge's quadratic form added to the lm_nsum<D> sums (each kernel
// unpacks them into H and b itself: the note above so_optimize in sim3_optimizer.hip), the dense LDLT with diagonal pivoting behind
// (H + lambda I) x = b, the gain denominator -- and the fixed-order sum over a workgroup of 256.  The scalar lambda / rho / stop
// rules are lm_rules.hpp's (local_ba.hip runs them too).  Everything in double, as g2o runs it.
#pragma once
#include "lm_rules.hpp"
#include "orbfe_common.hpp"
#include <cfloat>
#include <cmath>

namespace orbfe {
namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_WAVES = LM_THREADS / 64;

struct Quat {
    double x, y, z, w;
};

// Eigen's Quaternion::toRotationMatrix
__device__ __forceinline__ void rot_of(const Quat& q, double (&R)[3][3])
{
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

// Eigen's Quaternion(const Matrix3&): the trace branch, else the largest diagonal entry
__device__ Quat quat_from_matrix(const double (&m)[3][3])
{
    Quat q;
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (m[2][1] - m[1][2]) * t;
        q.y = (m[0][2] - m[2][0]) * t;
        q.z = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double v[3];
        t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        v[i] = 0.5 * t;
        t = 0.5 / t;
        q.w = (m[k][j] - m[j][k]) * t;
        v[j] = (m[j][i] + m[i][j]) * t;
        v[k] = (m[k][i] + m[i][k]) * t;
        q.x = v[0]; q.y = v[1]; q.z = v[2];
    }
    return q;
}

__device__ __forceinline__ void cross(const double (&a)[3], const double (&b)[3], double (&r)[3])
{
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// q v = v + w uv + qv x uv, uv = 2 (qv x v)
__device__ __forceinline__ void rotate(const Quat& q, const double (&v)[3], double (&r)[3])
{
    const double qv[3] = {q.x, q.y, q.z};
    double uv[3], c[3];
    cross(qv, v, uv);
    for (int i = 0; i < 3; i++) uv[i] += uv[i];
    cross(qv, uv, c);
    for (int i = 0; i < 3; i++) r[i] = v[i] + q.w * uv[i] + c[i];
}

// Eigen's quaternion product, not normalised
__device__ __forceinline__ Quat qmul(const Quat& a, const Quat& b)
{
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}

struct Cam {
    double fx, fy, cx, cy;
};

__device__ __forceinline__ void project_error(const double (&Xc)[3], double ox, double oy, const Cam& K, double (&err)[2])
{
    err[0] = ox - ((Xc[0] / Xc[2]) * K.fx + K.cx);
    err[1] = oy - ((Xc[1] / Xc[2]) * K.fy + K.cy);
}

__device__ __forceinline__ double chi2_of(const double (&e)[2], double info) { return e[0] * (info * e[0]) + e[1] * (info * e[1]); }

// RobustKernelHuber::robustify: rho[0], rho[1]
__device__ __forceinline__ void huber(double chi2, double delta, double (&rho)[2])
{
    const double dsqr = delta * delta;
    if (chi2 <= dsqr) {
        rho[0] = chi2;
        rho[1] = 1.;
    } else {
        const double s = sqrt(chi2);
        rho[0] = 2 * s * delta - dsqr;
        rho[1] = delta / s;
    }
}

// Eigen's LDLT (lower triangle, diagonal pivoting on the largest remaining |diagonal|): isPositive() and x = H^-1 b (x untouched
// when it is not).  A zero pivot leaves its column as it is and solves to 0, so a row and column that hold lambda alone are accepted.
template <int N> __device__ bool ldlt_solve(double (&m)[N][N], const double (&b)[N], double (&x)[N])
{
    const int n = N;
    int tr[N];
    int sign = 0;   // 0 zero, 1 positive semidefinite, -1 negative semidefinite, 2 indefinite
    for (int k = 0; k < n; k++) {
        int big = k;
        double bv = fabs(m[k][k]);
        for (int i = k + 1; i < n; i++)
            if (fabs(m[i][i]) > bv) {
                bv = fabs(m[i][i]);
                big = i;
            }
        tr[k] = big;
        if (k != big) {
            for (int j = 0; j < k; j++) {
                const double t = m[k][j]; m[k][j] = m[big][j]; m[big][j] = t;
            }
            for (int i = big + 1; i < n; i++) {
                const double t = m[i][k]; m[i][k] = m[i][big]; m[i][big] = t;
            }
            {
                const double t = m[k][k]; m[k][k] = m[big][big]; m[big][big] = t;
            }
            for (int i = k + 1; i < big; i++) {
                const double t = m[i][k];
                m[i][k] = m[big][i];
                m[big][i] = t;
            }
        }
        if (k > 0) {
            double temp[N];
            for (int j = 0; j < k; j++) temp[j] = m[j][j] * m[k][j];
            double s = 0;
            for (int j = 0; j < k; j++) s += m[k][j] * temp[j];
            m[k][k] -= s;
            for (int i = k + 1; i < n; i++) {
                double si = 0;
                for (int j = 0; j < k; j++) si += m[i][j] * temp[j];
                m[i][k] -= si;
            }
        }
        const double akk = m[k][k];
        const bool valid = fabs(akk) > 0;
        if (k == 0 && !valid) {
            sign = 0;
            for (int j = 0; j < n; j++) tr[j] = j;
            break;
        }
        if (valid)
            for (int i = k + 1; i < n; i++) m[i][k] /= akk;
        if (sign == 1) {
            if (akk < 0) sign = 2;
        } else if (sign == -1) {
            if (akk > 0) sign = 2;
        } else if (sign == 0) {
            if (akk > 0) sign = 1;
            else if (akk < 0) sign = -1;
        }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double y[N];
    for (int i = 0; i < n; i++) y[i] = b[i];
    for (int k = 0; k < n; k++) {
        const double t = y[k]; y[k] = y[tr[k]]; y[tr[k]] = t;
    }
    for (int i = 0; i < n; i++) {
        double s = y[i];
        for (int j = 0; j < i; j++) s -= m[i][j] * y[j];
        y[i] = s;
    }
    for (int i = 0; i < n; i++) y[i] = fabs(m[i][i]) > DBL_MIN ? y[i] / m[i][i] : 0.0;
    for (int i = n - 1; i >= 0; i--) {
        double s = y[i];
        for (int j = i + 1; j < n; j++) s -= m[j][i] * y[j];
        y[i] = s;
    }
    for (int k = n - 1; k >= 0; k--) {
        const double t = y[k]; y[k] = y[tr[k]]; y[tr[k]] = t;
    }
    for (int i = 0; i < n; i++) x[i] = y[i];
    return true;
}

// ------------------------------------------------------------------------------------- the dense system, D = 6 or 7 --
// what a linearisation pass sums: the robust chi2, H's upper triangle row by row, b
template <int D> constexpr int lm_nsum = 1 + D * (D + 1) / 2 + D;

// BaseUnaryEdge / BaseBinaryEdge::constructQuadraticForm for Omega = info I: H += J^T (rho' Omega) J, b += J^T rho' (-Omega e)
template <int D>
__device__ __forceinline__ void add_edge(const double (&err)[2], const double (&J)[2][D], double info, double rho1, double (&s)[lm_nsum<D>])
{
    const double w = rho1 * info;
    const double r0 = rho1 * -(info * err[0]), r1 = rho1 * -(info * err[1]);
    int k = 1;
#pragma unroll
    for (int a = 0; a < D; a++)
#pragma unroll
        for (int c = a; c < D; c++, k++) s[k] += J[0][a] * (w * J[0][c]) + J[1][a] * (w * J[1][c]);
#pragma unroll
    for (int a = 0; a < D; a++) s[1 + D * (D + 1) / 2 + a] += J[0][a] * r0 + J[1][a] * r1;
}

// (H + lambda I) x = b from the previous update x0 (which stays when the damped system is not positive); returns isPositive()
template <int D>
__device__ __forceinline__ bool damped_solve(const double (&H)[D][D], const double (&b)[D], double lambda, const double (&x0)[D], double (&x)[D])
{
    double Hl[D][D];
    for (int r = 0; r < D; r++)
        for (int cc = 0; cc < D; cc++) Hl[r][cc] = H[r][cc];
    for (int j = 0; j < D; j++) Hl[j][j] += lambda;
    for (int j = 0; j < D; j++) x[j] = x0[j];
    return ldlt_solve(Hl, b, x);
}

// the denominator of the gain ratio, without its 1e-3 (lm_judge_trial adds it)
template <int D> __device__ __forceinline__ double gain_scale(const double (&x)[D], const double (&b)[D], double lambda)
{
    double scale = 0;
    for (int j = 0; j < D; j++) scale += x[j] * (lambda * x[j] + b[j]);
    return scale;
}

// sum of N doubles over the workgroup: butterfly inside each wave, then the waves in order; the result is valid in thread 0
template <int N> __device__ __forceinline__ void block_sum(double (&v)[N], double* red)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    }
    if (lane == 0)
        for (int k = 0; k < N; k++) red[w * N + k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < N; k++) {
            double s = red[k];
            for (int ww = 1; ww < LM_WAVES; ww++) s += red[ww * N + k];
            v[k] = s;
        }
}

// "Each thread a contiguous run, then the workgroup": f(i) for the run of [0, n) that is thread threadIdx.x's of T, in index order.
// What f adds up, block_sum (or a wave's butterfly, T = 64) adds over the threads.
template <int T = LM_THREADS, class F> __device__ __forceinline__ void run_for(int n, F f)
{
    const int per = (n + T - 1) / T;
    const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
    for (int i = lo; i < hi; i++) f(i);
}

// this thread's part of the sum of n doubles (the whole sum in thread 0 behind block_sum)
__device__ __forceinline__ double run_sum(const double* v, int n)
{
    double s = 0;
    run_for(n, [&](int i) { s += v[i]; });
    return s;
}

__device__ __forceinline__ int block_count(int c, double* red)
{
    double v[1] = {(double)c};
    block_sum<1>(v, red);
    return (int)v[0];
}

constexpr size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }

// what a workgroup may ask for, static and dynamic LDS together
inline int max_lds()
{
    static int v = 0;
    if (!v) {
        int dev = 0, b = 0;
        (void)hipGetDevice(&dev);
        v = hipDeviceGetAttribute(&b, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && b > 0 ? b : 65536;
    }
    return v;
}

} // namespace
} // namespace orbfe
