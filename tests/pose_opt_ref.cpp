// pose_opt_ref.cpp -- CPU restatement of ORB_SLAM2's motion-only pose optimization (Optimizer::PoseOptimizationByAruco,
// src/Optimizer.cc of the reference, and PoseOptimization without its stereo branch) for the parity tests of
// orbfe_pose_optimization*.  No g2o or Eigen here: the pieces the reference runs through are restated from their algorithms:
//   SE3Quat                  quaternion + translation; product = t1 + q1 t2, q1 q2, then w >= 0 and normalisation; exp() with the
//                            small-angle branch below theta = 1e-5; construction from a rotation matrix (Eigen's trace /
//                            largest-diagonal quaternion) followed by the same normalisation
//   mono edge                e = obs - pi(T Xw), Omega = invSigma2 I, analytic Jacobian of the left-multiplied increment
//   marker edge              e = obs - pi((T Twm) p), Omega = w I, numeric Jacobian: central differences, delta = 1e-9, through
//                            exp(+-delta e_d) * T (the marker vertex is fixed, so only the camera's six columns)
//   Huber kernel             rho = (e, 1) inside delta^2, (2 delta sqrt(e) - delta^2, delta / sqrt(e)) outside; H and b weigh by rho'
//   Levenberg-Marquardt      lambda0 = 1e-5 max diag H, up to 10 trials an iteration, rho = dchi / (x (lambda x + b) + 1e-3),
//                            lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)) on success, *= nu (nu *= 2) on failure, the stop rules
//   dense solve              LDLT with diagonal pivoting (largest remaining |diagonal|), not positive -> chi2 = DBL_MAX
// Edges are summed in insertion order: mono edges by keypoint index, then the marker edges, marker by marker, corner 0..3.  The
// "cached" error an inlier's chi2 reads after a round is the error at the last pose the active edges were evaluated at, which
// is a rejected trial's pose when the round ended on rejected trials.
// Built by tests/pose_opt_build.py (g++ -O2 -ffp-contract=off) and loaded with ctypes.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct KeyPoint {   // cv::KeyPoint layout
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

struct Marker {     // the library's marker record: undistorted corners, Twm (3 x 4 row-major), corners in the marker frame
    float corners[8];
    float Twm[12];
    float local[12];
};

struct Result {     // the layout of the library's result record
    int32_t n_good, n_initial, n_marker_edges, rounds;
    int32_t n_bad[4];
    int32_t iterations[4];
    int32_t stale_mask;
    int32_t status;
};

// ------------------------------------------------------------------------------------------ SE3Quat --
struct Quat {
    double x, y, z, w;
};
struct SE3 {
    Quat q;
    double t[3];
};

void normalize_rotation(Quat& q)
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

Quat quat_from_matrix(const double m[3][3])
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

void cross(const double a[3], const double b[3], double r[3])
{
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// q v: v + w uv + qv x uv, uv = 2 (qv x v)
void rotate(const Quat& q, const double v[3], double r[3])
{
    const double qv[3] = {q.x, q.y, q.z};
    double uv[3], c[3];
    cross(qv, v, uv);
    for (int i = 0; i < 3; i++) uv[i] += uv[i];
    cross(qv, uv, c);
    for (int i = 0; i < 3; i++) r[i] = v[i] + q.w * uv[i] + c[i];
}

Quat qmul(const Quat& a, const Quat& b)
{
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}

SE3 mul(const SE3& a, const SE3& b)
{
    SE3 r = a;
    double qt[3];
    rotate(a.q, b.t, qt);
    for (int i = 0; i < 3; i++) r.t[i] += qt[i];
    r.q = qmul(a.q, b.q);
    normalize_rotation(r.q);
    return r;
}

void map(const SE3& T, const double p[3], double r[3])
{
    rotate(T.q, p, r);
    for (int i = 0; i < 3; i++) r[i] += T.t[i];
}

SE3 se3_from_Rt(const double R[3][3], const double t[3])
{
    SE3 T;
    T.q = quat_from_matrix(R);
    for (int i = 0; i < 3; i++) T.t[i] = t[i];
    normalize_rotation(T.q);
    return T;
}

SE3 se3_from_float(const float* Rt)
{
    double R[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = Rt[r * 4 + c];
        t[r] = Rt[r * 4 + 3];
    }
    return se3_from_Rt(R, t);
}

void mat3mul(const double a[3][3], const double b[3][3], double r[3][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
}

SE3 se3_exp(const double u[6])
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

void to_float(const SE3& T, float* Rt)
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

struct MonoEdge {
    double obs[2], Xw[3], info;
    int idx;          // keypoint index
    bool outlier;     // level 1
};

struct MarkerEdge {
    double obs[2], p[3], info;
    SE3 Twm;
};

void mono_error(const MonoEdge& e, const SE3& T, const Cam& K, double err[2])
{
    double Xc[3];
    map(T, e.Xw, Xc);
    err[0] = e.obs[0] - ((Xc[0] / Xc[2]) * K.fx + K.cx);
    err[1] = e.obs[1] - ((Xc[1] / Xc[2]) * K.fy + K.cy);
}

void mono_jacobian(const MonoEdge& e, const SE3& T, const Cam& K, double J[2][6])
{
    double Xc[3];
    map(T, e.Xw, Xc);
    const double x = Xc[0], y = Xc[1], invz = 1.0 / Xc[2], invz_2 = invz * invz;
    J[0][0] = x * y * invz_2 * K.fx;
    J[0][1] = -(1 + (x * x * invz_2)) * K.fx;
    J[0][2] = y * invz * K.fx;
    J[0][3] = -invz * K.fx;
    J[0][4] = 0;
    J[0][5] = x * invz_2 * K.fx;
    J[1][0] = (1 + y * y * invz_2) * K.fy;
    J[1][1] = -x * y * invz_2 * K.fy;
    J[1][2] = -x * invz * K.fy;
    J[1][3] = 0;
    J[1][4] = -invz * K.fy;
    J[1][5] = y * invz_2 * K.fy;
}

void marker_error(const MarkerEdge& e, const SE3& T, const Cam& K, double err[2])
{
    const SE3 Tcm = mul(T, e.Twm);
    double p[3];
    map(Tcm, e.p, p);
    err[0] = e.obs[0] - ((p[0] / p[2]) * K.fx + K.cx);
    err[1] = e.obs[1] - ((p[1] / p[2]) * K.fy + K.cy);
}

void marker_jacobian(const MarkerEdge& e, const SE3& T, const Cam& K, double J[2][6])
{
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    for (int d = 0; d < 6; d++) {
        double u[6] = {0, 0, 0, 0, 0, 0}, ep[2], em[2];
        u[d] = delta;
        marker_error(e, mul(se3_exp(u), T), K, ep);
        u[d] = -delta;
        marker_error(e, mul(se3_exp(u), T), K, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
}

double chi2_of(const double e[2], double info) { return e[0] * (info * e[0]) + e[1] * (info * e[1]); }

// Huber: rho[0], rho[1]
void huber(double chi2, double delta, double rho[2])
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

// ------------------------------------------------------------------------------------------ LDLT 6x6 --
// Diagonal pivoting on the lower triangle, as Eigen's LDLT; returns isPositive() and x = H^-1 b (x untouched when not positive)
bool ldlt_solve(const double Hin[6][6], const double b[6], double x[6])
{
    const int n = 6;
    double m[6][6];
    std::memcpy(m, Hin, sizeof(m));
    int tr[6];
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
        double temp[6];
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
    double y[6];
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

// ------------------------------------------------------------------------------------------ the graph --
struct Graph {
    std::vector<MonoEdge> mono;
    std::vector<MarkerEdge> marker;
    Cam K;
    double delta;
    bool mono_kernel;
    SE3 T;         // the camera vertex
    SE3 Tev;       // the pose the active edges' cached errors belong to
};

double active_chi2(Graph& g)
{
    double chi = 0;
    g.Tev = g.T;
    for (const MonoEdge& e : g.mono) {
        if (e.outlier) continue;
        double err[2], rho[2];
        mono_error(e, g.T, g.K, err);
        const double c = chi2_of(err, e.info);
        if (g.mono_kernel) {
            huber(c, g.delta, rho);
            chi += rho[0];
        } else {
            chi += c;
        }
    }
    for (const MarkerEdge& e : g.marker) {
        double err[2], rho[2];
        marker_error(e, g.T, g.K, err);
        huber(chi2_of(err, e.info), g.delta, rho);
        chi += rho[0];
    }
    return chi;
}

void add_edge(const double err[2], const double J[2][6], double info, double rho1, double H[6][6], double b[6])
{
    const double w = rho1 * info;
    const double r0 = rho1 * -(info * err[0]), r1 = rho1 * -(info * err[1]);
    for (int a = 0; a < 6; a++) {
        b[a] += J[0][a] * r0 + J[1][a] * r1;
        for (int c = a; c < 6; c++) H[a][c] += J[0][a] * (w * J[0][c]) + J[1][a] * (w * J[1][c]);
    }
}

void build_system(const Graph& g, double H[6][6], double b[6])
{
    std::memset(H, 0, sizeof(double) * 36);
    std::memset(b, 0, sizeof(double) * 6);
    for (const MonoEdge& e : g.mono) {
        if (e.outlier) continue;
        double err[2], J[2][6], rho[2] = {0, 1};
        mono_error(e, g.T, g.K, err);
        mono_jacobian(e, g.T, g.K, J);
        if (g.mono_kernel) huber(chi2_of(err, e.info), g.delta, rho);
        add_edge(err, J, e.info, rho[1], H, b);
    }
    for (const MarkerEdge& e : g.marker) {
        double err[2], J[2][6], rho[2];
        marker_error(e, g.T, g.K, err);
        marker_jacobian(e, g.T, g.K, J);
        huber(chi2_of(err, e.info), g.delta, rho);
        add_edge(err, J, e.info, rho[1], H, b);
    }
    for (int a = 0; a < 6; a++)
        for (int c = 0; c < a; c++) H[a][c] = H[c][a];
}

// SparseOptimizer::optimize(10) with OptimizationAlgorithmLevenberg.  Returns the iterations run (-1 without active edges); *stale =
// the last trial of the last iteration was rejected (the cached errors are that trial's).
int optimize(Graph& g, int iterations, bool* stale)
{
    *stale = false;
    bool any = !g.marker.empty();
    for (const MonoEdge& e : g.mono) any = any || !e.outlier;
    if (!any) return -1;
    double lambda = 0, ni = 2, x[6] = {0, 0, 0, 0, 0, 0};
    int nbad = 0, it = 0;
    for (it = 0; it < iterations;) {
        double currentChi = active_chi2(g);
        const double iniChi = currentChi;
        double H[6][6], b[6];
        build_system(g, H, b);
        if (it == 0) {
            double md = 0;
            for (int j = 0; j < 6; j++) md = std::max(std::fabs(H[j][j]), md);
            lambda = 1e-5 * md;
            ni = 2;
            nbad = 0;
        }
        double rho = 0;
        int q = 0;
        do {
            const SE3 saved = g.T;
            double Hl[6][6];
            std::memcpy(Hl, H, sizeof(Hl));
            for (int j = 0; j < 6; j++) Hl[j][j] += lambda;
            const bool ok2 = ldlt_solve(Hl, b, x);
            g.T = mul(se3_exp(x), g.T);
            double tempChi = active_chi2(g);
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;
            for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                const double sf = std::max(1. / 3., alpha);
                lambda *= sf;
                ni = 2;
                currentChi = tempChi;
                *stale = false;
            } else {
                lambda *= ni;
                ni *= 2;
                g.T = saved;
                *stale = true;
            }
            q++;
        } while (rho < 0 && q < 10);
        it++;
        if (q == 10 || rho == 0) break;
        if ((iniChi - currentChi) * 1e3 < iniChi) nbad++;
        else nbad = 0;
        if (nbad >= 3) break;
    }
    return it;
}

} // namespace

// One PoseOptimizationByAruco (or PoseOptimization: nm = 0) problem.  kps: n keypoints (mvKeysUn), has_mp[i]: a map point
// (mono), x3Dw: n x 3.  markers: nm records.  chi2_rounds (4 x n, may be NULL): the chi2 of every mono edge at each round's
// classification (NaN where not classified).  Returns 0, or -1 for an octave outside [0, nlevels).
extern "C" int ref_pose_optimization(const KeyPoint* kps, int n, const uint8_t* has_mp, const float* x3Dw, const float* inv_sigma2,
                                     int nlevels, const float* K4, const Marker* markers, int nm, float marker_info,
                                     const float* Tcw_in, float* Tcw_out, uint8_t* outlier, double* chi2_rounds, Result* res)
{
    std::memset(res, 0, sizeof(*res));
    if (chi2_rounds)
        for (int i = 0; i < 4 * n; i++) chi2_rounds[i] = NAN;
    Graph g;
    g.K = Cam{K4[0], K4[1], K4[2], K4[3]};
    g.delta = (double)(float)std::sqrt(5.991);
    g.mono_kernel = true;
    for (int i = 0; i < n; i++) {
        if (!has_mp[i]) continue;
        if (kps[i].octave < 0 || kps[i].octave >= nlevels) return -1;
        MonoEdge e;
        e.obs[0] = kps[i].x;
        e.obs[1] = kps[i].y;
        for (int k = 0; k < 3; k++) e.Xw[k] = x3Dw[3 * i + k];
        e.info = inv_sigma2[kps[i].octave];
        e.idx = i;
        e.outlier = false;
        g.mono.push_back(e);
    }
    res->n_initial = (int)g.mono.size();
    for (const MonoEdge& e : g.mono) outlier[e.idx] = 0;
    std::memcpy(Tcw_out, Tcw_in, 12 * sizeof(float));
    if (res->n_initial < 3) return 0;
    for (int m = 0; m < nm; m++) {
        const SE3 Twm = se3_from_float(markers[m].Twm);
        for (int k = 0; k < 4; k++) {
            MarkerEdge e;
            e.obs[0] = markers[m].corners[2 * k];
            e.obs[1] = markers[m].corners[2 * k + 1];
            for (int c = 0; c < 3; c++) e.p[c] = markers[m].local[3 * k + c];
            e.info = marker_info;
            e.Twm = Twm;
            g.marker.push_back(e);
        }
    }
    res->n_marker_edges = (int)g.marker.size();
    const size_t nedges = g.mono.size() + g.marker.size();
    const SE3 T0 = se3_from_float(Tcw_in);
    int nBad = 0;
    for (int it = 0; it < 4; it++) {
        g.T = T0;
        bool stale = false;
        res->iterations[it] = optimize(g, 10, &stale);
        res->stale_mask |= stale ? 1 << it : 0;
        res->rounds = it + 1;
        nBad = 0;
        for (MonoEdge& e : g.mono) {
            double err[2];
            mono_error(e, e.outlier ? g.T : g.Tev, g.K, err);
            const double c = chi2_of(err, e.info);
            if (chi2_rounds) chi2_rounds[it * n + e.idx] = c;
            if ((float)c > 5.991f) {
                e.outlier = true;
                nBad++;
            } else {
                e.outlier = false;
            }
            outlier[e.idx] = e.outlier ? 1 : 0;
        }
        res->n_bad[it] = nBad;
        if (it == 2) g.mono_kernel = false;
        if (nedges < 10) break;
    }
    to_float(g.T, Tcw_out);
    res->n_good = res->n_initial - nBad;
    return 0;
}

// The numeric marker Jacobian at (T, edge) and, for the test of it, the marker edge's error.  Tcw / Twm: 3x4 float.
extern "C" void ref_marker_jacobian(const float* Tcw, const float* Twm, const double* p, const double* obs, const float* K4, double* J,
                                    double* err)
{
    MarkerEdge e;
    e.obs[0] = obs[0];
    e.obs[1] = obs[1];
    for (int c = 0; c < 3; c++) e.p[c] = p[c];
    e.info = 1;
    e.Twm = se3_from_float(Twm);
    const Cam K{K4[0], K4[1], K4[2], K4[3]};
    const SE3 T = se3_from_float(Tcw);
    double Jm[2][6];
    marker_jacobian(e, T, K, Jm);
    std::memcpy(J, Jm, sizeof(Jm));
    marker_error(e, T, K, err);
}

// T = exp(u) * Tcw, as a 3x4 float (the test of the update's convention)
extern "C" void ref_exp_update(const double* u, const float* Tcw, float* out) { to_float(mul(se3_exp(u), se3_from_float(Tcw)), out); }
