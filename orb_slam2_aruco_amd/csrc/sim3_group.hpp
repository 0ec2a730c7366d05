// sim3_group.hpp -- g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) as the device restatements use it (sim3_optimizer.hip,
// essential_graph.hip): product, map, inverse, the exponential map of the Vector7d constructor and log(), each with g2o's branches and
// g2o's order of operations.  Everything in double.
#pragma once
#include "lm_dense.hpp"

namespace orbfe {
namespace {

// ------------------------------------------------------------------------------------------ g2o::Sim3 --
struct Sim3 {
    Quat q;       // not normalised: Sim3's product and constructors never do
    double t[3];
    double s;
};

__device__ __forceinline__ Sim3 mul(const Sim3& a, const Sim3& b)
{
    Sim3 r;
    double qt[3];
    r.q = qmul(a.q, b.q);
    rotate(a.q, b.t, qt);
    for (int i = 0; i < 3; i++) r.t[i] = a.s * qt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

__device__ __forceinline__ void map(const Sim3& S, const double (&p)[3], double (&r)[3])
{
    double qp[3];
    rotate(S.q, p, qp);
    for (int i = 0; i < 3; i++) r[i] = S.s * qp[i] + S.t[i];
}

__device__ __forceinline__ Sim3 inverse(const Sim3& S)
{
    Sim3 r;
    r.q = Quat{-S.q.x, -S.q.y, -S.q.z, S.q.w};
    const double c = -1. / S.s;
    const double v[3] = {c * S.t[0], c * S.t[1], c * S.t[2]};
    rotate(r.q, v, r.t);
    r.s = 1. / S.s;
    return r;
}

// Sim3(const Vector7d&): omega, upsilon, sigma.  Below eps = 1e-5 the rotation is I + Omega + Omega^2 (not orthonormal) and the
// quaternion made of it is not normalised.
__device__ __noinline__ Sim3 sim3_exp(const double (&u)[7])
{
    const double om0 = u[0], om1 = u[1], om2 = u[2], sigma = u[6];
    const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
    const double O[3][3] = {{0, -om2, om1}, {om2, 0, -om0}, {-om1, om0, 0}};
    double O2[3][3], R[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    Sim3 S;
    S.s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C;
    if (theta < eps) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double a = S.s * sin(theta), b = S.s * cos(theta);
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    S.q = quat_from_matrix(R);
    for (int i = 0; i < 3; i++) {
        double W[3];
        for (int j = 0; j < 3; j++) W[j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);
        S.t[i] = W[0] * u[3] + W[1] * u[4] + W[2] * u[5];
    }
    return S;
}

// Eigen's PartialPivLU of a 3 x 3 matrix and its solve: the row of the largest |entry| of the column comes up, unit lower factor
__device__ __forceinline__ void lu3_solve(double (&m)[3][3], const double (&b)[3], double (&x)[3])
{
    int perm[3] = {0, 1, 2};
    for (int k = 0; k < 3; k++) {
        int big = k;
        double bv = fabs(m[k][k]);
        for (int i = k + 1; i < 3; i++)
            if (fabs(m[i][k]) > bv) {
                bv = fabs(m[i][k]);
                big = i;
            }
        if (big != k) {
            for (int j = 0; j < 3; j++) {
                const double t = m[k][j]; m[k][j] = m[big][j]; m[big][j] = t;
            }
            const int t = perm[k]; perm[k] = perm[big]; perm[big] = t;
        }
        if (bv != 0)
            for (int i = k + 1; i < 3; i++) m[i][k] /= m[k][k];
        for (int i = k + 1; i < 3; i++)
            for (int j = k + 1; j < 3; j++) m[i][j] -= m[i][k] * m[k][j];
    }
    double y[3];
    for (int i = 0; i < 3; i++) {
        double s = b[perm[i]];
        for (int j = 0; j < i; j++) s -= m[i][j] * y[j];
        y[i] = s;
    }
    for (int i = 2; i >= 0; i--) {
        double s = y[i];
        for (int j = i + 1; j < 3; j++) s -= m[i][j] * x[j];
        x[i] = s / m[i][i];
    }
}

// Sim3::log: omega from deltaR (half of it above d = 1 - 1e-5, theta / (2 sqrt(1 - d^2)) of it below), sigma = log s, and upsilon
// from W upsilon = t by the LU above; A, B, C by the four branches of |sigma| < 1e-5 and d > 1 - 1e-5
[[maybe_unused]] __device__ __noinline__ void sim3_log(const Sim3& S, double (&res)[7])
{
    const Quat& q = S.q;
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    const double R[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1 - (txx + tyy)}};
    const double sigma = log(S.s);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    const double eps = 0.00001;
    double om[3], A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta;
            const double f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; i++) om[i] = f * dR[i];
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            const double f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; i++) om[i] = f * dR[i];
            const double theta2 = theta * theta;
            const double a = S.s * sin(theta), b = S.s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double O[3][3] = {{0, -om[2], om[1]}, {om[2], 0, -om[0]}, {-om[1], om[0], 0}};
    double W[3][3], ups[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double bo2 = (B * O[i][0]) * O[0][j] + (B * O[i][1]) * O[1][j] + (B * O[i][2]) * O[2][j];
            W[i][j] = (A * O[i][j] + bo2) + C * (i == j ? 1.0 : 0.0);
        }
    lu3_solve(W, S.t, ups);
    for (int i = 0; i < 3; i++) {
        res[i] = om[i];
        res[i + 3] = ups[i];
    }
    res[6] = sigma;
}

} // namespace
} // namespace orbfe
