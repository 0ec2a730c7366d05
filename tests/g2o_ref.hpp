// g2o_ref.hpp -- what the five CPU restatements of the g2o optimizers (pose_opt_ref.cpp, sim3_opt_ref.cpp, essential_ref.cpp, and
// lba_ref.cpp and gba_ref.cpp through ba_ref.hpp, which holds what those two share on top of this) have in common: SE3Quat, the
// projection error, the Huber kernel, the dense LDLT, and OptimizationAlgorithmLevenberg's scalar rules.  No g2o or Eigen here: the
// pieces are restated from their algorithms.
//
// This header includes nothing from orb_slam2_aruco_amd/csrc/, and nothing there includes anything from tests/.  The restatements
// are the second opinion on the device code: the five of them sharing their common pieces keeps that, while sharing a line with the
// device would turn every parity test into a comparison of the code with itself.  The same rules are therefore written twice in this
// repository, once here and once in csrc/ (lm_rules.hpp, lm_dense.hpp, se3_quat.hpp), on purpose.
//
// Plain C++14, compiled into each restatement (g++ -O2 -ffp-contract=off, tests/ref_build.py).
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace {

// ------------------------------------------------------------------------------------------ SE3Quat --
//   quaternion + translation; product = t1 + q1 t2, q1 q2, then w >= 0 and normalisation; exp() with the small-angle branch below
//   theta = 1e-5; construction from a rotation matrix (Eigen's trace / largest-diagonal quaternion) followed by the same normalisation
struct Quat {
    double x, y, z, w;
};
struct SE3 {
    Quat q;
    double t[3];
};

inline void normalize_rotation(Quat& q)
{
    if (q.w < 0) {
        q.x *= -1; q.y *= -1; q.z *= -1; q.w *= -1;
    }
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (n2 > 0) {
        const double n = std::sqrt(n2);
        q.x /= n; q.y /= n; q.z /= n; q.w /= n;
    }
}

inline Quat quat_from_matrix(const double m[3][3])
{
    Quat q;
    double* v[3] = {&q.x, &q.y, &q.z};
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
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
        t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        *v[i] = 0.5 * t;
        t = 0.5 / t;
        q.w = (m[k][j] - m[j][k]) * t;
        *v[j] = (m[j][i] + m[i][j]) * t;
        *v[k] = (m[k][i] + m[i][k]) * t;
    }
    return q;
}

inline void cross(const double a[3], const double b[3], double r[3])
{
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// q v: v + w uv + qv x uv, uv = 2 (qv x v)
inline void rotate(const Quat& q, const double v[3], double r[3])
{
    const double qv[3] = {q.x, q.y, q.z};
    double uv[3], c[3];
    cross(qv, v, uv);
    for (int i = 0; i < 3; i++) uv[i] += uv[i];
    cross(qv, uv, c);
    for (int i = 0; i < 3; i++) r[i] = v[i] + q.w * uv[i] + c[i];
}

inline Quat qmul(const Quat& a, const Quat& b)
{
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}

inline SE3 mul(const SE3& a, const SE3& b)
{
    SE3 r = a;
    double qt[3];
    rotate(a.q, b.t, qt);
    for (int i = 0; i < 3; i++) r.t[i] += qt[i];
    r.q = qmul(a.q, b.q);
    normalize_rotation(r.q);
    return r;
}

inline void map(const SE3& T, const double p[3], double r[3])
{
    rotate(T.q, p, r);
    for (int i = 0; i < 3; i++) r[i] += T.t[i];
}

inline SE3 se3_from_Rt(const double R[3][3], const double t[3])
{
    SE3 T;
    T.q = quat_from_matrix(R);
    for (int i = 0; i < 3; i++) T.t[i] = t[i];
    normalize_rotation(T.q);
    return T;
}

inline SE3 se3_from_float(const float* Rt)
{
    double R[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = Rt[r * 4 + c];
        t[r] = Rt[r * 4 + 3];
    }
    return se3_from_Rt(R, t);
}

inline void mat3mul(const double a[3][3], const double b[3][3], double r[3][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
}

inline SE3 se3_exp(const double u[6])
{
    const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
    const double theta = std::sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[3][3] = {{0, -om[2], om[1]}, {om[2], 0, -om[0]}, {-om[1], om[0], 0}};
    double O2[3][3], R[3][3], V[3][3];
    mat3mul(O, O, O2);
    if (theta < 0.00001) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
        std::memcpy(V, R, sizeof(R));
    } else {
        const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta);
        const double c = (theta - std::sin(theta)) / std::pow(theta, 3);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
                V[i][j] = ((i == j ? 1.0 : 0.0) + b * O[i][j]) + c * O2[i][j];
            }
    }
    double t[3];
    for (int i = 0; i < 3; i++) t[i] = V[i][0] * up[0] + V[i][1] * up[1] + V[i][2] * up[2];
    return se3_from_Rt(R, t);
}

inline void to_float(const SE3& T, float* Rt)
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

// ------------------------------------------------------------------------------------------- edges --
struct Cam {
    double fx, fy, cx, cy;
};

// obs - cam_project(Xc)
inline void project_error(const double Xc[3], double ox, double oy, const Cam& K, double err[2])
{
    err[0] = ox - ((Xc[0] / Xc[2]) * K.fx + K.cx);
    err[1] = oy - ((Xc[1] / Xc[2]) * K.fy + K.cy);
}

inline double chi2_of(const double e[2], double info) { return e[0] * (info * e[0]) + e[1] * (info * e[1]); }

// RobustKernelHuber: rho = (e, 1) inside delta^2, (2 delta sqrt(e) - delta^2, delta / sqrt(e)) outside; H and b weigh by rho[1]
inline void huber(double chi2, double delta, double rho[2])
{
    const double dsqr = delta * delta;
    if (chi2 <= dsqr) {
        rho[0] = chi2;
        rho[1] = 1.;
    } else {
        const double s = std::sqrt(chi2);
        rho[0] = 2 * s * delta - dsqr;
        rho[1] = delta / s;
    }
}

// ------------------------------------------------------------------------------------------ LDLT N x N --
// Diagonal pivoting (largest remaining |diagonal|) on the lower triangle, as Eigen's LDLT; returns isPositive() and x = H^-1 b (x
// untouched when not positive).  A zero pivot leaves its column as it is and solves to 0.
template <int N> bool ldlt_solve(const double Hin[N][N], const double b[N], double x[N])
{
    const int n = N;
    double m[N][N];
    std::memcpy(m, Hin, sizeof(m));
    int tr[N];
    int sign = 0;   // 0 zero, 1 positive semidefinite, -1 negative semidefinite, 2 indefinite
    for (int k = 0; k < n; k++) {
        int big = k;
        double bv = std::fabs(m[k][k]);
        for (int i = k + 1; i < n; i++)
            if (std::fabs(m[i][i]) > bv) {
                bv = std::fabs(m[i][i]);
                big = i;
            }
        tr[k] = big;
        if (k != big) {
            for (int j = 0; j < k; j++) std::swap(m[k][j], m[big][j]);
            for (int i = big + 1; i < n; i++) std::swap(m[i][k], m[i][big]);
            std::swap(m[k][k], m[big][big]);
            for (int i = k + 1; i < big; i++) {
                const double tmp = m[i][k];
                m[i][k] = m[big][i];
                m[big][i] = tmp;
            }
        }
        double temp[N];
        if (k > 0) {
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
        const bool valid = std::fabs(akk) > 0;
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
    std::memcpy(y, b, sizeof(y));
    for (int k = 0; k < n; k++) std::swap(y[k], y[tr[k]]);
    for (int i = 0; i < n; i++) {
        double s = y[i];
        for (int j = 0; j < i; j++) s -= m[i][j] * y[j];
        y[i] = s;
    }
    for (int i = 0; i < n; i++) y[i] = std::fabs(m[i][i]) > DBL_MIN ? y[i] / m[i][i] : 0.0;
    for (int i = n - 1; i >= 0; i--) {
        double s = y[i];
        for (int j = i + 1; j < n; j++) s -= m[j][i] * y[j];
        y[i] = s;
    }
    for (int k = n - 1; k >= 0; k--) std::swap(y[k], y[tr[k]]);
    std::memcpy(x, y, sizeof(y));
    return true;
}

// ------------------------------------------------------------------------------------------ Levenberg-Marquardt --
// OptimizationAlgorithmLevenberg's scalars over one optimize(): lambda0 = 1e-5 max diag H, up to 10 trials an iteration,
// rho = dchi / (x (lambda x + b) + 1e-3), lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)) on success, *= nu (nu *= 2) on failure, the
// stop rules.  lambda and nu start again in every optimize().
struct Levenberg {
    double lambda, ni, currentChi, iniChi, rho;
    int q, nbad;
};

inline void lm_begin(Levenberg& c)
{
    c.lambda = 0;
    c.ni = 2;
    c.nbad = 0;
    c.rho = 0;
}

// behind a linearisation with robust chi2 `chi`; maxdiag (the largest |diagonal| of H) counts in the first iteration only
inline void lm_linearised(Levenberg& c, double chi, bool first, double maxdiag)
{
    c.currentChi = chi;
    c.iniChi = c.currentChi;
    if (first) {
        c.lambda = 1e-5 * maxdiag;
        c.ni = 2;
        c.nbad = 0;
    }
    c.rho = 0;
    c.q = 0;
}

// behind a trial: tempChi its robust chi2, ok2 whether the solve succeeded, scale = sum x (lambda x + b) without the 1e-3.  Returns
// whether the trial is accepted (the caller restores its estimate when not).
inline bool lm_trial(Levenberg& c, double tempChi, bool ok2, double scale)
{
    if (!ok2) tempChi = DBL_MAX;
    c.rho = c.currentChi - tempChi;
    scale += 1e-3;
    c.rho /= scale;
    c.q++;
    if (c.rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow((2 * c.rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        const double sf = std::max(1. / 3., alpha);
        c.lambda *= sf;
        c.ni = 2;
        c.currentChi = tempChi;
        return true;
    }
    c.lambda *= c.ni;
    c.ni *= 2;
    return false;
}

inline bool lm_again(const Levenberg& c) { return c.rho < 0 && c.q < 10; }

// behind the trials of an iteration: whether optimize() stops
inline bool lm_iteration_end(Levenberg& c)
{
    if (c.q == 10 || c.rho == 0) return true;
    if ((c.iniChi - c.currentChi) * 1e3 < c.iniChi) c.nbad++;
    else c.nbad = 0;
    return c.nbad >= 3;
}

} // namespace
