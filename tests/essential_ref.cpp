// CPU restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1245-1542) behind its collect step, for the parity tests of
// csrc/essential_graph.hip.  Test infrastructure only: plain C++14, built by tests/ref_build.py, no g2o, no Eigen, and no line shared
// with orb_slam2_aruco_amd/csrc/.  g2o::Sim3 (product, inverse, map, the Vector7d constructor, log with its four branches, deltaR, the
// 3 x 3 partially pivoted LU), EdgeSim3::computeError, BaseBinaryEdge's central differences and the Levenberg rules (g2o_ref.hpp, with
// lambda0 set to the user's 1e-16 behind lm_linearised) are restated from their algorithms.
//
// The linear system is the full 7 nfree x 7 nfree one, dense, solved by an L D L^T without pivoting in a vertex order the caller
// passes as data (`order`: the free vertices, each once); a pivot <= 0 is "not solved".  Two orders give the spread from which the
// tolerance of the GPU tests is made.  This is not g2o: g2o solves the same system with a sparse Cholesky in its own
// order, and its rounding differs from both.
#include <cstdint>
#include <vector>

#include "g2o_ref.hpp"

namespace {

struct Sim {
    Quat q;
    double t[3], s;
};

Sim sim_of8(const double* v)
{
    Sim S;
    S.q = Quat{v[0], v[1], v[2], v[3]};
    for (int i = 0; i < 3; i++) S.t[i] = v[4 + i];
    S.s = v[7];
    return S;
}

void sim_to8(const Sim& S, double* v)
{
    v[0] = S.q.x; v[1] = S.q.y; v[2] = S.q.z; v[3] = S.q.w;
    for (int i = 0; i < 3; i++) v[4 + i] = S.t[i];
    v[7] = S.s;
}

Sim sim_of_pose(const float* Rt)
{
    double R[3][3];
    Sim S;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = Rt[4 * r + c];
        S.t[r] = Rt[4 * r + 3];
    }
    S.q = quat_from_matrix(R);
    S.s = 1.0;
    return S;
}

Sim operator*(const Sim& a, const Sim& b)
{
    Sim r;
    r.q = qmul(a.q, b.q);
    double v[3];
    rotate(a.q, b.t, v);
    for (int i = 0; i < 3; i++) r.t[i] = a.s * v[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

Sim inv(const Sim& a)
{
    Sim r;
    r.q = Quat{-a.q.x, -a.q.y, -a.q.z, a.q.w};
    const double f = -1. / a.s;
    const double v[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
    rotate(r.q, v, r.t);
    r.s = 1. / a.s;
    return r;
}

void sim_map(const Sim& a, const double p[3], double out[3])
{
    double v[3];
    rotate(a.q, p, v);
    for (int i = 0; i < 3; i++) out[i] = a.s * v[i] + a.t[i];
}

void skew(const double w[3], double O[3][3])
{
    O[0][0] = 0; O[0][1] = -w[2]; O[0][2] = w[1];
    O[1][0] = w[2]; O[1][1] = 0; O[1][2] = -w[0];
    O[2][0] = -w[1]; O[2][1] = w[0]; O[2][2] = 0;
}

void rot_matrix(const Quat& q, double R[3][3])
{
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

// the coefficients of W = A Omega + B Omega^2 + C I shared by the constructor and log()
void abc(double sigma, double s, double theta, bool small_angle, double& A, double& B, double& C)
{
    const double eps = 0.00001;
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (small_angle) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double t2 = theta * theta;
            A = (1 - std::cos(theta)) / t2;
            B = (theta - std::sin(theta)) / (t2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_angle) {
            const double s2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / s2;
            B = ((0.5 * s2 - sigma + 1) * s) / (s2 * sigma);
        } else {
            const double a = s * std::sin(theta), b = s * std::cos(theta);
            const double t2 = theta * theta, c = t2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / t2;
        }
    }
}

Sim sim_exp(const double u[7])
{
    const double w[3] = {u[0], u[1], u[2]};
    const double sigma = u[6], theta = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double O[3][3], O2[3][3], R[3][3];
    skew(w, O);
    mat3mul(O, O, O2);
    Sim S;
    S.s = std::exp(sigma);
    const bool small_angle = theta < 0.00001;
    double A, B, C;
    abc(sigma, S.s, theta, small_angle, A, B, C);
    const double ca = small_angle ? 1.0 : std::sin(theta) / theta, cb = small_angle ? 1.0 : (1 - std::cos(theta)) / (theta * theta);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R[i][j] = small_angle ? ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j] : ((i == j ? 1.0 : 0.0) + ca * O[i][j]) + cb * O2[i][j];
    S.q = quat_from_matrix(R);
    for (int i = 0; i < 3; i++) {
        S.t[i] = 0;
        double row[3];
        for (int j = 0; j < 3; j++) row[j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);
        S.t[i] = row[0] * u[3] + row[1] * u[4] + row[2] * u[5];
    }
    return S;
}

// Eigen's PartialPivLU::solve for a 3 x 3 matrix
void lu_solve3(double a[3][3], const double b[3], double x[3])
{
    int p[3] = {0, 1, 2};
    for (int k = 0; k < 3; k++) {
        int best = k;
        for (int i = k + 1; i < 3; i++)
            if (std::fabs(a[i][k]) > std::fabs(a[best][k])) best = i;
        if (best != k) {
            for (int j = 0; j < 3; j++) std::swap(a[k][j], a[best][j]);
            std::swap(p[k], p[best]);
        }
        if (a[k][k] != 0)
            for (int i = k + 1; i < 3; i++) a[i][k] /= a[k][k];
        for (int i = k + 1; i < 3; i++)
            for (int j = k + 1; j < 3; j++) a[i][j] -= a[i][k] * a[k][j];
    }
    double y[3];
    for (int i = 0; i < 3; i++) {
        y[i] = b[p[i]];
        for (int j = 0; j < i; j++) y[i] -= a[i][j] * y[j];
    }
    for (int i = 2; i >= 0; i--) {
        x[i] = y[i];
        for (int j = i + 1; j < 3; j++) x[i] -= a[i][j] * x[j];
        x[i] /= a[i][i];
    }
}

void sim_log(const Sim& S, double out[7])
{
    double R[3][3];
    rot_matrix(S.q, R);
    const double sigma = std::log(S.s);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dr[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    const bool small_angle = d > 1 - 0.00001;
    double w[3], theta = 0;
    if (small_angle) {
        for (int i = 0; i < 3; i++) w[i] = 0.5 * dr[i];
    } else {
        theta = std::acos(d);
        const double f = theta / (2 * std::sqrt(1 - d * d));
        for (int i = 0; i < 3; i++) w[i] = f * dr[i];
    }
    double A, B, C;
    abc(sigma, S.s, theta, small_angle, A, B, C);
    double O[3][3], BO[3][3], BOO[3][3], W[3][3];
    skew(w, O);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) BO[i][j] = B * O[i][j];
    mat3mul(BO, O, BOO);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) W[i][j] = (A * O[i][j] + BOO[i][j]) + C * (i == j ? 1.0 : 0.0);
    double ups[3];
    lu_solve3(W, S.t, ups);
    for (int i = 0; i < 3; i++) {
        out[i] = w[i];
        out[3 + i] = ups[i];
    }
    out[6] = sigma;
}

void edge_error(const Sim& C, const Sim& vi, const Sim& vj, double err[7]) { sim_log(C * vi * inv(vj), err); }

Sim oplus(const Sim& est, const double upd[7], bool fix_scale)
{
    double u[7];
    std::memcpy(u, upd, sizeof u);
    if (fix_scale) u[6] = 0;
    return sim_exp(u) * est;
}

// g2o's numeric Jacobian of one side (side 0: vertex 0), row-major 7 x 7
void edge_jacobian(const Sim& C, const Sim& vi, const Sim& vj, int side, bool fix_scale, double J[49])
{
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    for (int d = 0; d < 7; d++) {
        double add[7] = {0, 0, 0, 0, 0, 0, 0}, e1[7], e2[7];
        add[d] = delta;
        if (side == 0) edge_error(C, oplus(vi, add, fix_scale), vj, e1);
        else edge_error(C, vi, oplus(vj, add, fix_scale), e1);
        add[d] = -delta;
        if (side == 0) edge_error(C, oplus(vi, add, fix_scale), vj, e2);
        else edge_error(C, vi, oplus(vj, add, fix_scale), e2);
        for (int k = 0; k < 7; k++) J[k * 7 + d] = scalar * (e1[k] - e2[k]);
    }
}

struct Problem {
    int nkf, fixed, ne, np;
    bool fix_scale;
    const int32_t *ei, *ej;
    const float* X;
    const int32_t* pref;
    std::vector<Sim> S0, est, meas;
};

void setup(Problem& P, const float* Tcw, int nkf, int fixed, const int32_t* cpos, const double* csim, int nc, const int32_t* npos, const double* nsim,
           int nn, const int32_t* ei, const int32_t* ej, const int32_t* ekind, int ne, int fix_scale)
{
    P.nkf = nkf; P.fixed = fixed; P.ne = ne; P.np = 0; P.fix_scale = fix_scale != 0; P.ei = ei; P.ej = ej; P.X = nullptr; P.pref = nullptr;
    P.S0.resize((size_t)nkf);
    std::vector<int> nc_of((size_t)nkf, -1);
    for (int k = 0; k < nkf; k++) P.S0[(size_t)k] = sim_of_pose(Tcw + 12 * (size_t)k);
    for (int k = 0; k < nc; k++) P.S0[(size_t)cpos[k]] = sim_of8(csim + 8 * (size_t)k);
    for (int k = 0; k < nn; k++) nc_of[(size_t)npos[k]] = k;
    P.est = P.S0;
    P.meas.resize((size_t)ne);
    for (int e = 0; e < ne; e++) {
        Sim Siw = P.S0[(size_t)ei[e]], Sjw = P.S0[(size_t)ej[e]];
        if (ekind[e] == 1) {
            if (nc_of[(size_t)ei[e]] >= 0) Siw = sim_of8(nsim + 8 * (size_t)nc_of[(size_t)ei[e]]);
            if (nc_of[(size_t)ej[e]] >= 0) Sjw = sim_of8(nsim + 8 * (size_t)nc_of[(size_t)ej[e]]);
        }
        P.meas[(size_t)e] = Sjw * inv(Siw);
    }
}

struct Lin {
    std::vector<double> err, Ji, Jj;   // per edge
    std::vector<double> H, b;          // the system in `order`: 7 n x 7 n, 7 n
    double chi;
};

// slot[v]: the place of vertex v in the system, -1 the fixed one
void linearise(const Problem& P, const std::vector<int>& slot, int n, Lin& L)
{
    L.err.assign((size_t)P.ne * 7, 0); L.Ji.assign((size_t)P.ne * 49, 0); L.Jj.assign((size_t)P.ne * 49, 0);
    L.H.assign((size_t)49 * n * n, 0); L.b.assign((size_t)7 * n, 0);
    L.chi = 0;
    const size_t N = (size_t)7 * n;
    for (int e = 0; e < P.ne; e++) {
        const int i = P.ei[e], j = P.ej[e];
        double* err = &L.err[(size_t)e * 7];
        edge_error(P.meas[(size_t)e], P.est[(size_t)i], P.est[(size_t)j], err);
        double c = 0;
        for (int k = 0; k < 7; k++) c += err[k] * err[k];
        L.chi += c;
        double* J[2] = {&L.Ji[(size_t)e * 49], &L.Jj[(size_t)e * 49]};
        const int s[2] = {slot[(size_t)i], slot[(size_t)j]};
        for (int side = 0; side < 2; side++)
            if (s[side] >= 0) edge_jacobian(P.meas[(size_t)e], P.est[(size_t)i], P.est[(size_t)j], side, P.fix_scale, J[side]);
        for (int a = 0; a < 2; a++) {
            if (s[a] < 0) continue;
            for (int r = 0; r < 7; r++) {
                double g = 0;
                for (int k = 0; k < 7; k++) g += J[a][k * 7 + r] * -err[k];
                L.b[(size_t)7 * s[a] + r] += g;
            }
            for (int bb = 0; bb < 2; bb++) {
                if (s[bb] < 0) continue;
                for (int r = 0; r < 7; r++)
                    for (int c2 = 0; c2 < 7; c2++) {
                        double h = 0;
                        for (int k = 0; k < 7; k++) h += J[a][k * 7 + r] * J[bb][k * 7 + c2];
                        L.H[((size_t)7 * s[a] + r) * N + (size_t)7 * s[bb] + c2] += h;
                    }
            }
        }
    }
}

// (H + lambda I) x = b by L D L^T without pivoting; false when a pivot is not positive (x untouched)
bool solve(const std::vector<double>& H, const std::vector<double>& b, int N, double lambda, std::vector<double>& x)
{
    std::vector<double> m(H);
    for (int i = 0; i < N; i++) m[(size_t)i * N + i] += lambda;
    std::vector<double> d((size_t)N);
    for (int k = 0; k < N; k++) {
        double dk = m[(size_t)k * N + k];
        for (int j = 0; j < k; j++) dk -= m[(size_t)k * N + j] * m[(size_t)k * N + j] * d[(size_t)j];
        if (!(dk > 0) || !std::isfinite(dk)) return false;
        d[(size_t)k] = dk;
        for (int i = k + 1; i < N; i++) {
            double v = m[(size_t)i * N + k];
            for (int j = 0; j < k; j++) v -= m[(size_t)i * N + j] * m[(size_t)k * N + j] * d[(size_t)j];
            m[(size_t)i * N + k] = v / dk;
        }
    }
    std::vector<double> y(b);
    for (int i = 0; i < N; i++)
        for (int j = 0; j < i; j++) y[(size_t)i] -= m[(size_t)i * N + j] * y[(size_t)j];
    for (int i = 0; i < N; i++) y[(size_t)i] /= d[(size_t)i];
    for (int i = N - 1; i >= 0; i--)
        for (int j = i + 1; j < N; j++) y[(size_t)i] -= m[(size_t)j * N + i] * y[(size_t)j];
    x = y;
    return true;
}

double chi2_at(const Problem& P, const std::vector<Sim>& est)
{
    double chi = 0;
    for (int e = 0; e < P.ne; e++) {
        double err[7], c = 0;
        edge_error(P.meas[(size_t)e], est[(size_t)P.ei[e]], est[(size_t)P.ej[e]], err);
        for (int k = 0; k < 7; k++) c += err[k] * err[k];
        chi += c;
    }
    return chi;
}

// the free vertices in the caller's order when order is NULL
std::vector<int> slots_of(int nkf, int fixed, const int32_t* order, int& n)
{
    std::vector<int> slot((size_t)nkf, -1);
    n = 0;
    if (order) {
        for (int k = 0; k < nkf - 1; k++) slot[(size_t)order[k]] = n++;
    } else {
        for (int v = 0; v < nkf; v++)
            if (v != fixed) slot[(size_t)v] = n++;
    }
    return slot;
}

} // namespace

extern "C" {

void ref_eg_exp(const double* u, double* sim8) { sim_to8(sim_exp(u), sim8); }
void ref_eg_log(const double* sim8, double* out7) { sim_log(sim_of8(sim8), out7); }
void ref_eg_mul(const double* a8, const double* b8, double* out8) { sim_to8(sim_of8(a8) * sim_of8(b8), out8); }
void ref_eg_inverse(const double* a8, double* out8) { sim_to8(inv(sim_of8(a8)), out8); }
void ref_eg_map(const double* a8, const double* p3, double* out3) { sim_map(sim_of8(a8), p3, out3); }
void ref_eg_lu3(const double* m9, const double* b3, double* x3)
{
    double a[3][3];
    std::memcpy(a, m9, sizeof(a));
    lu_solve3(a, b3, x3);
}

// error and both numeric Jacobians of one edge
void ref_eg_edge(const double* C8, const double* vi8, const double* vj8, int fix_scale, double* err, double* Ji, double* Jj)
{
    const Sim C = sim_of8(C8), vi = sim_of8(vi8), vj = sim_of8(vj8);
    edge_error(C, vi, vj, err);
    edge_jacobian(C, vi, vj, 0, fix_scale != 0, Ji);
    edge_jacobian(C, vi, vj, 1, fix_scale != 0, Jj);
}

// one linearisation and one solve at lambda0 = 1e-16: err, Ji, Jj per edge; Hd (nkf x 49), b and x (nkf x 7) in the caller's
// positions; chi2[3] = chi2, lambda0, solved
int ref_eg_inspect(const float* Tcw, int nkf, int fixed, const int32_t* cpos, const double* csim, int nc, const int32_t* npos, const double* nsim, int nn,
                   const int32_t* ei, const int32_t* ej, const int32_t* ekind, int ne, int fix_scale, const int32_t* order, double* err, double* Ji,
                   double* Jj, double* Hd, double* b, double* chi2, double* x)
{
    Problem P;
    setup(P, Tcw, nkf, fixed, cpos, csim, nc, npos, nsim, nn, ei, ej, ekind, ne, fix_scale);
    int n;
    const std::vector<int> slot = slots_of(nkf, fixed, order, n);
    Lin L;
    linearise(P, slot, n, L);
    std::memcpy(err, L.err.data(), L.err.size() * 8);
    std::memcpy(Ji, L.Ji.data(), L.Ji.size() * 8);
    std::memcpy(Jj, L.Jj.data(), L.Jj.size() * 8);
    std::vector<double> xs((size_t)7 * n, 0.);
    const bool ok = solve(L.H, L.b, 7 * n, 1e-16, xs);
    const size_t N = (size_t)7 * n;
    for (int v = 0; v < nkf; v++)
        for (int r = 0; r < 7; r++) {
            const int s = slot[(size_t)v];
            b[v * 7 + r] = s < 0 ? 0. : L.b[(size_t)7 * s + r];
            x[v * 7 + r] = s < 0 ? 0. : xs[(size_t)7 * s + r];
            for (int c = 0; c < 7; c++) Hd[v * 49 + r * 7 + c] = s < 0 ? 0. : L.H[((size_t)7 * s + r) * N + (size_t)7 * s + c];
        }
    chi2[0] = L.chi; chi2[1] = 1e-16; chi2[2] = ok;
    return 0;
}

// the whole function.  res: iterations, trials; chi: chi2_first, chi2_last, lambda_last, and the smallest |chi2 - trial chi2| / chi2 over
// the solved trials: how far the closest accept-or-reject decision of the run was from a tie
int ref_eg_optimize(const float* Tcw, int nkf, int fixed, const int32_t* cpos, const double* csim, int nc, const int32_t* npos, const double* nsim, int nn,
                    const int32_t* ei, const int32_t* ej, const int32_t* ekind, int ne, const float* X, const int32_t* pref, int np, int iterations,
                    int fix_scale, const int32_t* order, float* Tcw_out, float* X_out, double* Siw_out, int32_t* res, double* chi)
{
    Problem P;
    setup(P, Tcw, nkf, fixed, cpos, csim, nc, npos, nsim, nn, ei, ej, ekind, ne, fix_scale);
    res[0] = res[1] = 0;
    chi[0] = chi[1] = chi[2] = 0;
    chi[3] = DBL_MAX;
    if (nkf == 1 || ne == 0) {
        std::memcpy(Tcw_out, Tcw, (size_t)nkf * 48);
        if (np) std::memcpy(X_out, X, (size_t)np * 12);
        for (int v = 0; v < nkf; v++) sim_to8(P.S0[(size_t)v], Siw_out + 8 * (size_t)v);
        return 0;
    }
    int n;
    const std::vector<int> slot = slots_of(nkf, fixed, order, n);
    Levenberg lm{};
    lm_begin(lm);
    std::vector<double> x((size_t)7 * n, 0.);
    Lin L;
    for (int it = 0; it < iterations; it++) {
        linearise(P, slot, n, L);
        lm_linearised(lm, L.chi, it == 0, 0.);
        if (it == 0) {
            lm.lambda = 1e-16;   // setUserLambdaInit
            chi[0] = L.chi;
        }
        do {
            const bool ok = solve(L.H, L.b, 7 * n, lm.lambda, x);
            std::vector<Sim> trial(P.est);
            for (int v = 0; v < nkf; v++)
                if (slot[(size_t)v] >= 0) trial[(size_t)v] = oplus(P.est[(size_t)v], &x[(size_t)7 * slot[(size_t)v]], P.fix_scale);
            const double tempChi = chi2_at(P, trial);
            double scale = 0;
            for (size_t k = 0; k < x.size(); k++) scale += x[k] * (lm.lambda * x[k] + L.b[k]);
            if (ok && lm.currentChi > 0) chi[3] = std::min(chi[3], std::fabs(lm.currentChi - tempChi) / lm.currentChi);
            if (lm_trial(lm, tempChi, ok, scale)) P.est = trial;
            res[1]++;
        } while (lm_again(lm));
        res[0] = it + 1;
        if (lm_iteration_end(lm)) break;
    }
    chi[1] = lm.currentChi;
    chi[2] = lm.lambda;
    for (int v = 0; v < nkf; v++) {
        const Sim& S = P.est[(size_t)v];
        sim_to8(S, Siw_out + 8 * (size_t)v);
        double R[3][3];
        rot_matrix(S.q, R);
        const double f = 1. / S.s;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Tcw_out[12 * (size_t)v + 4 * r + c] = (float)R[r][c];
            Tcw_out[12 * (size_t)v + 4 * r + 3] = (float)(S.t[r] * f);
        }
    }
    for (int i = 0; i < np; i++) {
        if (pref[i] < 0) {
            for (int a = 0; a < 3; a++) X_out[3 * (size_t)i + a] = X[3 * (size_t)i + a];
            continue;
        }
        const double p0[3] = {X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]};
        double p1[3], p2[3];
        sim_map(P.S0[(size_t)pref[i]], p0, p1);
        sim_map(inv(P.est[(size_t)pref[i]]), p1, p2);
        for (int a = 0; a < 3; a++) X_out[3 * (size_t)i + a] = (float)p2[a];
    }
    return 0;
}

} // extern "C"
