// se3_quat.hpp -- g2o's SE3Quat as the device restatements use it (pose_optimizer.hip, local_ba.hip): product, map, the exponential
// map with its small-angle branch, Converter::toSE3Quat / toCvMat.  Everything in double.
#pragma once
#include "lm_dense.hpp"

namespace orbfe {
namespace {

// ------------------------------------------------------------------------------------------ SE3Quat --
struct SE3 {
    Quat q;
    double t[3];
    double pad;   // 64 B in LDS
};

__device__ __forceinline__ void normalize_rotation(Quat& q)
{
    if (q.w < 0) {
        q.x *= -1; q.y *= -1; q.z *= -1; q.w *= -1;
    }
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (n2 > 0) {
        const double n = sqrt(n2);
        q.x /= n; q.y /= n; q.z /= n; q.w /= n;
    }
}

__device__ __forceinline__ SE3 mul(const SE3& a, const SE3& b)
{
    SE3 r = a;
    double qt[3];
    rotate(a.q, b.t, qt);
    for (int i = 0; i < 3; i++) r.t[i] += qt[i];
    r.q = qmul(a.q, b.q);
    normalize_rotation(r.q);
    return r;
}

__device__ __forceinline__ void map(const SE3& T, const double (&p)[3], double (&r)[3])
{
    rotate(T.q, p, r);
    for (int i = 0; i < 3; i++) r[i] += T.t[i];
}

__device__ SE3 se3_from_Rt(const double (&R)[3][3], const double (&t)[3])
{
    SE3 T;
    T.q = quat_from_matrix(R);
    for (int i = 0; i < 3; i++) T.t[i] = t[i];
    T.pad = 0;
    normalize_rotation(T.q);
    return T;
}

// 3 x 4 row-major float -> SE3Quat (Converter::toSE3Quat)
__device__ SE3 se3_from_float(const float* Rt)
{
    double R[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = Rt[r * 4 + c];
        t[r] = Rt[r * 4 + 3];
    }
    return se3_from_Rt(R, t);
}

// SE3Quat::exp: the small-angle branch (theta < 1e-5) takes R = V = I + Omega + Omega^2
__device__ SE3 se3_exp(const double (&u)[6])
{
    const double om0 = u[0], om1 = u[1], om2 = u[2];
    const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
    const double O[3][3] = {{0, -om2, om1}, {om2, 0, -om0}, {-om1, om0, 0}};
    double O2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    if (theta < 0.00001) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
                V[i][j] = R[i][j];
            }
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
        const double c = (theta - sin(theta)) / pow(theta, 3.0);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
                V[i][j] = ((i == j ? 1.0 : 0.0) + b * O[i][j]) + c * O2[i][j];
            }
    }
    double t[3];
    for (int i = 0; i < 3; i++) t[i] = V[i][0] * u[3] + V[i][1] * u[4] + V[i][2] * u[5];
    return se3_from_Rt(R, t);
}

// Converter::toCvMat(SE3Quat): the rotation matrix of the quaternion (Eigen's toRotationMatrix), rounded to float
__device__ void to_float(const SE3& T, float* Rt)
{
    const Quat& q = T.q;
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rt[r * 4 + c] = (float)R[r * 3 + c];
        Rt[r * 4 + 3] = (float)T.t[r];
    }
}

} // namespace
} // namespace orbfe
