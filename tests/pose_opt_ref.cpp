// pose_opt_ref.cpp -- CPU restatement of ORB_SLAM2's motion-only pose optimization (Optimizer::PoseOptimizationByAruco,
// src/Optimizer.cc of the reference, and PoseOptimization without its stereo branch) for the parity tests of
// orbfe_pose_optimization*.  No g2o or Eigen here: the pieces the reference runs through are restated from their algorithms.
// SE3Quat, the Huber kernel, the Levenberg-Marquardt rules and the dense LDLT (not positive -> chi2 = DBL_MAX) are those of
// tests/g2o_ref.hpp, which the three restatements share; this file's own:
//   mono edge                e = obs - pi(T Xw), Omega = invSigma2 I, analytic Jacobian of the left-multiplied increment
//   marker edge              e = obs - pi((T Twm) p), Omega = w I, numeric Jacobian: central differences, delta = 1e-9, through
//                            exp(+-delta e_d) * T (the marker vertex is fixed, so only the camera's six columns)
// Edges are summed in insertion order: mono edges by keypoint index, then the marker edges, marker by marker, corner 0..3.  The
// "cached" error an inlier's chi2 reads after a round is the error at the last pose the active edges were evaluated at, which
// is a rejected trial's pose when the round ended on rejected trials.
// Built by tests/pose_opt_build.py (g++ -O2 -ffp-contract=off) and loaded with ctypes.
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

// ------------------------------------------------------------------------------------------- edges --
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
    project_error(Xc, e.obs[0], e.obs[1], K, err);
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
    project_error(p, e.obs[0], e.obs[1], K, err);
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
    Levenberg lm;
    lm_begin(lm);
    double x[6] = {0, 0, 0, 0, 0, 0};
    int it = 0;
    while (it < iterations) {
        const double chi = active_chi2(g);
        double H[6][6], b[6];
        build_system(g, H, b);
        double md = 0;
        for (int j = 0; j < 6; j++) md = std::max(std::fabs(H[j][j]), md);
        lm_linearised(lm, chi, it == 0, md);
        do {
            const SE3 saved = g.T;
            double Hl[6][6];
            std::memcpy(Hl, H, sizeof(Hl));
            for (int j = 0; j < 6; j++) Hl[j][j] += lm.lambda;
            const bool ok2 = ldlt_solve<6>(Hl, b, x);
            g.T = mul(se3_exp(x), g.T);
            const double tempChi = active_chi2(g);
            double scale = 0;
            for (int j = 0; j < 6; j++) scale += x[j] * (lm.lambda * x[j] + b[j]);
            *stale = !lm_trial(lm, tempChi, ok2, scale);
            if (*stale) g.T = saved;
        } while (lm_again(lm));
        it++;
        if (lm_iteration_end(lm)) break;
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
