// sim3_opt_ref.cpp -- CPU restatement of ORB_SLAM2's Optimizer::OptimizeSim3 (src/Optimizer.cc:1544-1739 of the reference) for the
// parity tests of orbfe_optimize_sim3*.  No g2o or Eigen here: the pieces the reference runs through are restated from their
// algorithms:
//   g2o::Sim3                quaternion (never normalised) + translation + scale; product r1 r2, s1 (r1 t2) + t1, s1 s2; inverse
//                            (r', r' ((-1 / s) t), 1 / s); Sim3(Vector7d) with its four branches around eps = 1e-5 (below it the
//                            rotation is I + Omega + Omega^2 and the quaternion made of it -- Eigen's trace / largest-diagonal
//                            construction -- is not normalised)
//   the two edges            e12 = obs1 - cam_map1(project(S.map(P2c))), e21 = obs2 - cam_map2(project(S.inverse().map(P1c))),
//                            Omega = invSigma2 I (a float widened), numeric Jacobian: central differences, delta = 1e-9,
//                            through Sim3(update) * S; with a fixed scale the update's 7th component is zeroed first
//   Huber kernel             delta = (double)sqrtf(th2), in both rounds
//   Levenberg-Marquardt      the rules of tests/g2o_ref.hpp (shared by the three restatements, with the quaternion pieces and the
//   and the dense solve      Huber kernel), 7 x 7; lambda and nu start again in every optimize()
//   OptimizeSim3             optimize(5), pairs with a cached chi2 > (double)th2 removed, return 0 when fewer than 10 are left
//                            (the estimate is not written back), optimize(10 or 5) from the first round's estimate, second check
// The "cached" error a check reads is the error at the last estimate the active edges were evaluated at, which is a rejected
// trial's estimate when the round ended on rejected trials.
// Two summation orders (argument `order`): 0 = the reference's insertion order, e12(i), e21(i) by keypoint index; 1 = the device's:
// kept correspondence k goes to lane k mod 256, which sums its correspondences in index order, e12 then e21; the 64 lanes of a
// wave are combined by a butterfly (offsets 32, 16, .., 1), the four waves in wave order.
// Where the reference is undefined the library's definitions are restated: an edge with an error or a Jacobian that is not finite
// adds nothing in that pass, and a chi2 that is not finite is bad at a check.
// Built by tests/sim3_opt_build.py (g++ -O2 -ffp-contract=off) and loaded with ctypes.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "g2o_ref.hpp"

namespace {

struct KeyPoint {   // cv::KeyPoint layout
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

struct Result {     // the layout of the library's result record
    int32_t n_inliers, n_correspondences, n_bad, more_iterations;
    int32_t iterations[2];
    int32_t stale_mask;
    int32_t status;
    double s12, q12[4], t12[3];
};

constexpr int NSUM = 36;   // robust chi2, H upper triangle (28), b (7)

// ------------------------------------------------------------------------------------------ g2o::Sim3 --
struct Sim3 {
    Quat q;
    double t[3];
    double s;
};

Sim3 mul(const Sim3& a, const Sim3& b)
{
    Sim3 r;
    double qt[3];
    r.q = qmul(a.q, b.q);
    rotate(a.q, b.t, qt);
    for (int i = 0; i < 3; i++) r.t[i] = a.s * qt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

void map(const Sim3& S, const double p[3], double r[3])
{
    double qp[3];
    rotate(S.q, p, qp);
    for (int i = 0; i < 3; i++) r[i] = S.s * qp[i] + S.t[i];
}

Sim3 inverse(const Sim3& S)
{
    Sim3 r;
    r.q = Quat{-S.q.x, -S.q.y, -S.q.z, S.q.w};
    const double c = -1. / S.s;
    const double v[3] = {c * S.t[0], c * S.t[1], c * S.t[2]};
    rotate(r.q, v, r.t);
    r.s = 1. / S.s;
    return r;
}

Sim3 sim3_exp(const double u[7])
{
    const double om0 = u[0], om1 = u[1], om2 = u[2], sigma = u[6];
    const double theta = std::sqrt(om0 * om0 + om1 * om1 + om2 * om2);
    const double O[3][3] = {{0, -om2, om1}, {om2, 0, -om0}, {-om1, om0, 0}};
    double O2[3][3], R[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    Sim3 S;
    S.s = std::exp(sigma);
    const double eps = 0.00001;
    double A, B, C;
    if (theta < eps) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {
        const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
    }
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - std::cos(theta)) / theta2;
            B = (theta - std::sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double a = S.s * std::sin(theta), b = S.s * std::cos(theta);
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

// VertexSim3Expmap::oplusImpl
Sim3 oplus(const Sim3& S, double u[7], bool fix_scale)
{
    if (fix_scale) u[6] = 0;
    return mul(sim3_exp(u), S);
}

Sim3 sim3_from_floats(float s, const float* R9, const float* t3)
{
    double R[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[r][c] = R9[3 * r + c];
    Sim3 S;
    S.q = quat_from_matrix(R);
    for (int k = 0; k < 3; k++) S.t[k] = t3[k];
    S.s = s;
    return S;
}

// ------------------------------------------------------------------------------------------- edges --
struct Pair {       // one kept correspondence: its two edges
    double P1[3], P2[3], obs1[2], obs2[2], info1, info2;
    int idx;        // index in keyframe 1
    bool removed;
};

void edge_error(const Sim3& S, const double P[3], const double obs[2], const Cam& K, double err[2])
{
    double X[3];
    map(S, P, X);
    project_error(X, obs[0], obs[1], K, err);
}

// central differences over the perturbed estimates sp[2 d] (+delta), sp[2 d + 1] (-delta); false when an entry is not finite
bool edge_jacobian(const Sim3* sp, const double P[3], const double obs[2], const Cam& K, double J[2][7])
{
    const double scalar = 1.0 / (2 * 1e-9);
    bool ok = true;
    for (int d = 0; d < 7; d++) {
        double ep[2], em[2];
        edge_error(sp[2 * d], P, obs, K, ep);
        edge_error(sp[2 * d + 1], P, obs, K, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
        ok = ok && std::isfinite(J[0][d]) && std::isfinite(J[1][d]);
    }
    return ok;
}

void perturbed(const Sim3& S, bool fix_scale, Sim3 sp[14], Sim3 spi[14])
{
    for (int k = 0; k < 14; k++) {
        double u[7] = {0, 0, 0, 0, 0, 0, 0};
        u[k >> 1] = (k & 1) ? -1e-9 : 1e-9;
        sp[k] = oplus(S, u, fix_scale);
        spi[k] = inverse(sp[k]);
    }
}

void add_edge(const double err[2], const double J[2][7], double info, double rho1, double s[NSUM])
{
    const double w = rho1 * info;
    const double r0 = rho1 * -(info * err[0]), r1 = rho1 * -(info * err[1]);
    int k = 1;
    for (int a = 0; a < 7; a++)
        for (int c = a; c < 7; c++, k++) s[k] += J[0][a] * (w * J[0][c]) + J[1][a] * (w * J[1][c]);
    for (int a = 0; a < 7; a++) s[29 + a] += J[0][a] * r0 + J[1][a] * r1;
}

// ------------------------------------------------------------------------------------------ the graph --
struct Graph {
    std::vector<Pair> pairs;
    Cam K1, K2;
    double delta;
    bool fix_scale;
    int order;     // 0: insertion order, 1: the device's
    Sim3 S;        // the vertex
    Sim3 Sev;      // the estimate the active edges' cached errors belong to
};

// what one pair adds at S: the robust chi2 (s[0]) and, with sp, H and b
void add_pair(const Graph& g, const Pair& p, const Sim3& S, const Sim3& Si, const Sim3* sp, const Sim3* spi, double s[NSUM])
{
    double err[2], J[2][7], rho[2];
    edge_error(S, p.P2, p.obs1, g.K1, err);
    bool ok = std::isfinite(err[0]) && std::isfinite(err[1]);
    if (sp) ok = edge_jacobian(sp, p.P2, p.obs1, g.K1, J) && ok;
    if (ok) {
        huber(chi2_of(err, p.info1), g.delta, rho);
        s[0] += rho[0];
        if (sp) add_edge(err, J, p.info1, rho[1], s);
    }
    edge_error(Si, p.P1, p.obs2, g.K2, err);
    ok = std::isfinite(err[0]) && std::isfinite(err[1]);
    if (sp) ok = edge_jacobian(spi, p.P1, p.obs2, g.K2, J) && ok;
    if (ok) {
        huber(chi2_of(err, p.info2), g.delta, rho);
        s[0] += rho[0];
        if (sp) add_edge(err, J, p.info2, rho[1], s);
    }
}

// the sums over the active pairs at g.S, in the graph's order; nsum = 1 (chi2 alone) or NSUM
void sum_pairs(Graph& g, bool linearise, double out[NSUM])
{
    g.Sev = g.S;
    const Sim3 Si = inverse(g.S);
    Sim3 sp[14], spi[14];
    if (linearise) perturbed(g.S, g.fix_scale, sp, spi);
    const int nsum = linearise ? NSUM : 1;
    if (g.order == 0) {
        for (int k = 0; k < NSUM; k++) out[k] = 0;
        for (const Pair& p : g.pairs)
            if (!p.removed) add_pair(g, p, g.S, Si, linearise ? sp : nullptr, spi, out);
        return;
    }
    static double lanes[256][NSUM];
    std::memset(lanes, 0, sizeof(lanes));
    for (size_t k = 0; k < g.pairs.size(); k++)
        if (!g.pairs[k].removed) add_pair(g, g.pairs[k], g.S, Si, linearise ? sp : nullptr, spi, lanes[k % 256]);
    for (int k = 0; k < nsum; k++) {
        double waves[4];
        for (int w = 0; w < 4; w++) {
            double v[64], t[64];
            for (int l = 0; l < 64; l++) v[l] = lanes[w * 64 + l][k];
            for (int off = 32; off >= 1; off >>= 1) {
                for (int l = 0; l < 64; l++) t[l] = v[l] + v[l ^ off];
                std::memcpy(v, t, sizeof(v));
            }
            waves[w] = v[0];
        }
        double s = waves[0];
        for (int w = 1; w < 4; w++) s += waves[w];
        out[k] = s;
    }
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg.  Returns the iterations run (-1 without active edges);
// *stale = the last trial of the last iteration was rejected (the cached errors are that trial's).
int optimize(Graph& g, int iterations, bool* stale)
{
    *stale = false;
    bool any = false;
    for (const Pair& p : g.pairs) any = any || !p.removed;
    if (!any) return -1;
    Levenberg lm;
    lm_begin(lm);
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    int it = 0;
    while (it < iterations) {
        double s[NSUM];
        sum_pairs(g, true, s);
        double H[7][7], b[7];
        int k = 1;
        for (int r = 0; r < 7; r++)
            for (int c = r; c < 7; c++, k++) H[r][c] = H[c][r] = s[k];
        for (int r = 0; r < 7; r++) b[r] = s[29 + r];
        double md = 0;
        for (int j = 0; j < 7; j++) md = std::max(std::fabs(H[j][j]), md);
        lm_linearised(lm, s[0], it == 0, md);
        do {
            const Sim3 saved = g.S;
            double Hl[7][7];
            std::memcpy(Hl, H, sizeof(Hl));
            for (int j = 0; j < 7; j++) Hl[j][j] += lm.lambda;
            const bool ok2 = ldlt_solve<7>(Hl, b, x);
            g.S = oplus(g.S, x, g.fix_scale);
            double t[NSUM];
            sum_pairs(g, false, t);
            double scale = 0;
            for (int j = 0; j < 7; j++) scale += x[j] * (lm.lambda * x[j] + b[j]);
            *stale = !lm_trial(lm, t[0], ok2, scale);
            if (*stale) g.S = saved;
        } while (lm_again(lm));
        it++;
        if (lm_iteration_end(lm)) break;
    }
    return it;
}

// the check after a round: the cached chi2 of both edges of every active pair against (double)th2.  chi2 (2 per keypoint of
// keyframe 1, may be NULL) receives them.
int classify(Graph& g, float th2, double* chi2)
{
    const Sim3 Si = inverse(g.Sev);
    int nb = 0;
    for (Pair& p : g.pairs) {
        if (p.removed) continue;
        double e12[2], e21[2];
        edge_error(g.Sev, p.P2, p.obs1, g.K1, e12);
        edge_error(Si, p.P1, p.obs2, g.K2, e21);
        const double c12 = chi2_of(e12, p.info1), c21 = chi2_of(e21, p.info2);
        if (chi2) {
            chi2[2 * p.idx] = c12;
            chi2[2 * p.idx + 1] = c21;
        }
        if (!(c12 <= (double)th2) || !(c21 <= (double)th2)) {
            p.removed = true;
            nb++;
        }
    }
    return nb;
}

// Rkw x + tkw as a CV_32F Mat product: double sums of float products in index order, plus C, rounded once
void rigid(const float* T, const float* x, double d[3])
{
    for (int r = 0; r < 3; r++)
        d[r] = (float)((((double)T[4 * r] * x[0] + (double)T[4 * r + 1] * x[1]) + (double)T[4 * r + 2] * x[2]) + (double)T[4 * r + 3]);
}

} // namespace

// One OptimizeSim3 problem in the arguments of orbfe_optimize_sim3 plus `order` (0: insertion order, 1: the device's).  chi2_checks
// (2 checks x n1 x 2, may be NULL): the chi2 of e12 and e21 of every pair a check looked at (NaN elsewhere).  Returns 0, or -1 for
// an octave outside [0, nlevels) on a kept correspondence.
extern "C" int ref_optimize_sim3(const KeyPoint* kps1, int n1, const float* x1, const uint8_t* v1, const float* Tcw1, const float* K4_1,
                                 const KeyPoint* kps2, int n2, const float* x2, const uint8_t* v2, const float* Tcw2, const float* K4_2,
                                 const int32_t* m12, const float* inv_sigma2, int nlevels, float s12, const float* R12, const float* t12,
                                 float th2, int fix_scale, int order, int32_t* m12_out, Result* res, double* chi2_checks)
{
    std::memset(res, 0, sizeof(*res));
    if (chi2_checks)
        for (int i = 0; i < 4 * n1; i++) chi2_checks[i] = NAN;
    Graph g;
    g.K1 = Cam{K4_1[0], K4_1[1], K4_1[2], K4_1[3]};
    g.K2 = Cam{K4_2[0], K4_2[1], K4_2[2], K4_2[3]};
    g.delta = (double)sqrtf(th2);
    g.fix_scale = fix_scale != 0;
    g.order = order;
    for (int i = 0; i < n1; i++) {
        const int j = m12[i];
        if (j < 0 || j >= n2 || (v1 && (!v1[i] || !v2[j]))) continue;
        if (kps1[i].octave < 0 || kps1[i].octave >= nlevels || kps2[j].octave < 0 || kps2[j].octave >= nlevels) return -1;
        Pair p;
        rigid(Tcw1, x1 + 3 * i, p.P1);
        rigid(Tcw2, x2 + 3 * j, p.P2);
        p.obs1[0] = kps1[i].x; p.obs1[1] = kps1[i].y;
        p.obs2[0] = kps2[j].x; p.obs2[1] = kps2[j].y;
        p.info1 = inv_sigma2[kps1[i].octave];
        p.info2 = inv_sigma2[kps2[j].octave];
        p.idx = i;
        p.removed = false;
        g.pairs.push_back(p);
    }
    const int N = (int)g.pairs.size();
    const Sim3 S0 = sim3_from_floats(s12, R12, t12);
    g.S = g.Sev = S0;
    for (int i = 0; i < n1; i++) m12_out[i] = m12[i];
    res->n_correspondences = N;
    bool stale = false;
    res->iterations[0] = optimize(g, 5, &stale);
    res->stale_mask |= stale ? 1 : 0;
    const int nBad = classify(g, th2, chi2_checks);
    res->n_bad = nBad;
    const Sim3* out = &S0;
    if (N - nBad >= 10) {
        res->more_iterations = nBad > 0 ? 10 : 5;
        res->iterations[1] = optimize(g, res->more_iterations, &stale);
        res->stale_mask |= stale ? 2 : 0;
        const int nBad2 = classify(g, th2, chi2_checks ? chi2_checks + 2 * n1 : nullptr);
        res->n_inliers = N - nBad - nBad2;
        out = &g.S;
    }
    for (const Pair& p : g.pairs)
        if (p.removed) m12_out[p.idx] = -1;
    res->s12 = out->s;
    res->q12[0] = out->q.x; res->q12[1] = out->q.y; res->q12[2] = out->q.z; res->q12[3] = out->q.w;
    for (int k = 0; k < 3; k++) res->t12[k] = out->t[k];
    return 0;
}

// The numeric Jacobians of e12 (at P2) and e21 (at P1) and the two errors, at the similarity (s, R, t) given as floats.
extern "C" void ref_sim3_edge_jacobians(float s12, const float* R12, const float* t12, int fix_scale, const double* P1, const double* P2,
                                        const double* obs1, const double* obs2, const float* K4_1, const float* K4_2, double* J12,
                                        double* J21, double* err12, double* err21)
{
    const Sim3 S = sim3_from_floats(s12, R12, t12);
    Sim3 sp[14], spi[14];
    perturbed(S, fix_scale != 0, sp, spi);
    const Cam K1{K4_1[0], K4_1[1], K4_1[2], K4_1[3]}, K2{K4_2[0], K4_2[1], K4_2[2], K4_2[3]};
    double J[2][7];
    edge_jacobian(sp, P2, obs1, K1, J);
    std::memcpy(J12, J, sizeof(J));
    edge_jacobian(spi, P1, obs2, K2, J);
    std::memcpy(J21, J, sizeof(J));
    edge_error(S, P2, obs1, K1, err12);
    edge_error(inverse(S), P1, obs2, K2, err21);
}

// out = oplus(S, u): s, q (x, y, z, w), t as 8 doubles (the test of the update's convention)
extern "C" void ref_sim3_oplus(const double* u, float s12, const float* R12, const float* t12, int fix_scale, double* out)
{
    double uu[7];
    std::memcpy(uu, u, sizeof(uu));
    const Sim3 S = oplus(sim3_from_floats(s12, R12, t12), uu, fix_scale != 0);
    out[0] = S.s;
    out[1] = S.q.x; out[2] = S.q.y; out[3] = S.q.z; out[4] = S.q.w;
    for (int k = 0; k < 3; k++) out[5 + k] = S.t[k];
}
