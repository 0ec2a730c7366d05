// ba_edges.hpp -- the edges of the two bundle adjustments on the device (local_ba.hip, global_ba.hip): EdgeSE3ProjectXYZ with g2o's
// analytic Jacobians, EdgeMarker with g2o's numeric ones, the blocks an edge adds to its vertices, and the wave-level sums.
#pragma once
#include "lm_dense.hpp"
#include "se3_quat.hpp"

namespace orbfe {
namespace {

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ bool finite_f(float v) { return isfinite(v); }

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

struct MonoLin {
    double err[2], Jp[2][6], Jx[2][3];
};

// EdgeSE3ProjectXYZ: computeError and linearizeOplus (types_six_dof_expmap.cpp:103-139)
__device__ __noinline__ void lba_mono_linearize(const SE3& T, const double (&Xw)[3], double ox, double oy, const Cam& K, MonoLin& o)
{
    double Xc[3], R[3][3];
    map(T, Xw, Xc);
    project_error(Xc, ox, oy, K, o.err);
    const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z;
    const double s = -1. / z;
    const double t0[3] = {s * K.fx, s * 0., s * (-x / z * K.fx)}, t1[3] = {s * 0., s * K.fy, s * (-y / z * K.fy)};
    rot_of(T.q, R);
    for (int c = 0; c < 3; c++) {
        o.Jx[0][c] = t0[0] * R[0][c] + t0[1] * R[1][c] + t0[2] * R[2][c];
        o.Jx[1][c] = t1[0] * R[0][c] + t1[1] * R[1][c] + t1[2] * R[2][c];
    }
    o.Jp[0][0] = x * y / z_2 * K.fx;
    o.Jp[0][1] = -(1 + (x * x / z_2)) * K.fx;
    o.Jp[0][2] = y / z * K.fx;
    o.Jp[0][3] = -1. / z * K.fx;
    o.Jp[0][4] = 0;
    o.Jp[0][5] = x / z_2 * K.fx;
    o.Jp[1][0] = (1 + y * y / z_2) * K.fy;
    o.Jp[1][1] = -x * y / z_2 * K.fy;
    o.Jp[1][2] = -x / z * K.fy;
    o.Jp[1][3] = 0;
    o.Jp[1][4] = -1. / z * K.fy;
    o.Jp[1][5] = y / z_2 * K.fy;
}

__device__ __noinline__ void lba_mono_error(const SE3& T, const double (&Xw)[3], double ox, double oy, const Cam& K, double (&err)[2])
{
    double Xc[3];
    map(T, Xw, Xc);
    project_error(Xc, ox, oy, K, err);
}

// EdgeMarker::computeError: obs - pi((c2g g2m) point)
__device__ __noinline__ void lba_marker_error(const SE3& Tc, const SE3& Tm, const double (&pm)[3], double ox, double oy, const Cam& K,
                                              double (&err)[2])
{
    const SE3 Tcm = mul(Tc, Tm);
    double Xc[3];
    map(Tcm, pm, Xc);
    project_error(Xc, ox, oy, K, err);
}

// BaseBinaryEdge::linearizeOplus for one vertex: central differences through exp(+-1e-9 e_d) * estimate
__device__ __noinline__ void lba_marker_jacobian(const SE3& Tc, const SE3& Tm, bool camera, const double (&pm)[3], double ox, double oy,
                                                 const Cam& K, double (&J)[2][6])
{
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    for (int d = 0; d < 6; d++) {
        double u[6] = {0, 0, 0, 0, 0, 0}, ep[2], em[2];
        u[d] = delta;
        SE3 E = se3_exp(u);
        if (camera) lba_marker_error(mul(E, Tc), Tm, pm, ox, oy, K, ep);
        else lba_marker_error(Tc, mul(E, Tm), pm, ox, oy, K, ep);
        u[d] = -delta;
        E = se3_exp(u);
        if (camera) lba_marker_error(mul(E, Tc), Tm, pm, ox, oy, K, em);
        else lba_marker_error(Tc, mul(E, Tm), pm, ox, oy, K, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
}

__device__ __forceinline__ bool all_finite(const double* v, int n)
{
    bool ok = true;
    for (int i = 0; i < n; i++) ok = ok && isfinite(v[i]);
    return ok;
}

// upper triangle of Ja^T w Ja (21) and Ja^T r (6)
__device__ __noinline__ void lba_diag_block(const double (&J)[2][6], double w, double r0, double r1, double* out)
{
    int k = 0;
    for (int a = 0; a < 6; a++)
        for (int c = a; c < 6; c++, k++) out[k] = J[0][a] * (w * J[0][c]) + J[1][a] * (w * J[1][c]);
    for (int a = 0; a < 6; a++) out[21 + a] = J[0][a] * r0 + J[1][a] * r1;
}

} // namespace
} // namespace orbfe
