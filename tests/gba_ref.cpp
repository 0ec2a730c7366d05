// gba_ref.cpp -- CPU restatement of ORB_SLAM2's Optimizer::BundleAdjustment (src/Optimizer.cc:49-307 of the reference, behind its
// collect step, with this fork's marker poses as free SE3 vertices) for the parity tests of orbfe_global_bundle_adjustment*.
// No g2o or Eigen here; the pieces are restated from their algorithms, SE3Quat, the Huber kernel and the Levenberg-Marquardt rules in
// tests/g2o_ref.hpp (shared by the restatements), and nothing of orb_slam2_aruco_amd/csrc/ is included:
//   EdgeSE3ProjectXYZ        e = obs - pi(T Xw), Omega = invSigma2 I, g2o's analytic Jacobians; Huber with delta = (float)sqrt(5.99)
//                            when `robust`
//   EdgeMarker               e = obs - pi((Tcw Twm) p), Omega = w I, numeric Jacobians on both vertices (central differences,
//                            delta = 1e-9, through exp(+-delta e_d) * estimate; none for a fixed keyframe); always Huber
//   BlockSolver_6_3          Hpp (6 x 6 per free pose vertex), Hll (3 x 3 per point), Hpl per edge; S = Hpp - sum Hpl Hll^-1 Hpl^T with
//                            Hll^-1 by cofactors.  S is built and factored DENSE here (L L^T without pivoting, a pivot that is not
//                            positive and finite fails the solve): the second opinion on the library's sparse fronts.  The LDLT of
//                            g2o_ref.hpp has its size fixed at compile time (6, 7), so the factorisation is written out here
//   Levenberg-Marquardt      one optimize(iterations): lambda0 = 1e-5 max diagonal over pose and point blocks, up to 10 trials an
//                            iteration, rho = dchi / (sum x (lambda x + b) + 1e-3), g2o's lambda / nu and stop rules
// A point without observations is no vertex; a free keyframe or marker without an edge is not part of the system.
// Two summation orders: 0 = g2o's (every block and the chi2 summed edge by edge in insertion order, S reduced point by point),
// 1 = the device's (a point's observations in order; a pose block over contiguous runs of the vertex's edge list, one run a thread of
// 256, the threads by a butterfly inside each wave of 64 and the waves in order; a block of S the same over 64 lanes and the pair's
// items; the chi2 by waves of 64 points, then runs of those partial sums over 256 threads).
// Built by tests/gba_build.py (g++ -O2 -ffp-contract=off) and loaded with ctypes.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "g2o_ref.hpp"

namespace {

struct Result {     // the layout of orbfe_gba_result
    int32_t status, iterations, trials, n_edges_mono, n_edges_marker, n_points_left_out;
    double chi2_first, chi2_last, lambda_last;
};

void rot_of(const Quat& q, double R[3][3])
{
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

void mono_error(const SE3& T, const double Xw[3], double ox, double oy, const Cam& K, double err[2])
{
    double Xc[3];
    map(T, Xw, Xc);
    project_error(Xc, ox, oy, K, err);
}

// EdgeSE3ProjectXYZ::linearizeOplus
void mono_linearize(const SE3& T, const double Xw[3], double ox, double oy, const Cam& K, double err[2], double Jp[2][6], double Jx[2][3])
{
    double Xc[3], R[3][3];
    map(T, Xw, Xc);
    project_error(Xc, ox, oy, K, err);
    const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z;
    const double s = -1. / z;
    const double t0[3] = {s * K.fx, s * 0., s * (-x / z * K.fx)}, t1[3] = {s * 0., s * K.fy, s * (-y / z * K.fy)};
    rot_of(T.q, R);
    for (int c = 0; c < 3; c++) {
        Jx[0][c] = t0[0] * R[0][c] + t0[1] * R[1][c] + t0[2] * R[2][c];
        Jx[1][c] = t1[0] * R[0][c] + t1[1] * R[1][c] + t1[2] * R[2][c];
    }
    Jp[0][0] = x * y / z_2 * K.fx;
    Jp[0][1] = -(1 + (x * x / z_2)) * K.fx;
    Jp[0][2] = y / z * K.fx;
    Jp[0][3] = -1. / z * K.fx;
    Jp[0][4] = 0;
    Jp[0][5] = x / z_2 * K.fx;
    Jp[1][0] = (1 + y * y / z_2) * K.fy;
    Jp[1][1] = -x * y / z_2 * K.fy;
    Jp[1][2] = -x / z * K.fy;
    Jp[1][3] = 0;
    Jp[1][4] = -1. / z * K.fy;
    Jp[1][5] = y / z_2 * K.fy;
}

void marker_error(const SE3& Tc, const SE3& Tm, const double pm[3], double ox, double oy, const Cam& K, double err[2])
{
    const SE3 Tcm = mul(Tc, Tm);
    double Xc[3];
    map(Tcm, pm, Xc);
    project_error(Xc, ox, oy, K, err);
}

void marker_jacobian(const SE3& Tc, const SE3& Tm, bool camera, const double pm[3], double ox, double oy, const Cam& K, double J[2][6])
{
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    for (int d = 0; d < 6; d++) {
        double u[6] = {0, 0, 0, 0, 0, 0}, ep[2], em[2];
        u[d] = delta;
        SE3 E = se3_exp(u);
        if (camera) marker_error(mul(E, Tc), Tm, pm, ox, oy, K, ep);
        else marker_error(Tc, mul(E, Tm), pm, ox, oy, K, ep);
        u[d] = -delta;
        E = se3_exp(u);
        if (camera) marker_error(mul(E, Tc), Tm, pm, ox, oy, K, em);
        else marker_error(Tc, mul(E, Tm), pm, ox, oy, K, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
}

bool all_finite(const double* v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

void diag_block(const double J[2][6], double w, double r0, double r1, double* out)
{
    int k = 0;
    for (int a = 0; a < 6; a++)
        for (int c = a; c < 6; c++, k++) out[k] = J[0][a] * (w * J[0][c]) + J[1][a] * (w * J[1][c]);
    for (int a = 0; a < 6; a++) out[21 + a] = J[0][a] * r0 + J[1][a] * r1;
}

// ------------------------------------------------------------------------------------------ the device's sums --
double butterfly64(double* v)
{
    double t[64];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; l++) t[l] = v[l] + v[l ^ off];
        std::memcpy(v, t, sizeof(t));
    }
    return v[0];
}

double block256(double* v)   // 256 thread values: a butterfly per wave, the waves in order
{
    double s = butterfly64(v);
    for (int w = 1; w < 4; w++) s += butterfly64(v + 64 * w);
    return s;
}

// n values: a contiguous run a thread of 256, then the workgroup
double runs256(const double* x, int n)
{
    const int per = (n + 255) / 256;
    double v[256];
    for (int t = 0; t < 256; t++) {
        const int lo = std::min(t * per, n), hi = std::min(lo + per, n);
        double s = 0;
        for (int i = lo; i < hi; i++) s += x[i];
        v[t] = s;
    }
    return block256(v);
}

// ------------------------------------------------------------------------------------------ the problem --
constexpr int EB = 45, MB = 90;

struct Prob {
    int nkf, np, nobs, nma, nmobs, nme, nv, order;
    bool robust;
    const int32_t *off, *okf;
    const float* oxy;
    std::vector<double> info;
    Cam K;
    double delta, minfo;
    const float* mlocal;
    const int32_t *moff, *mkf;
    const float* mcor;
    std::vector<int> mo_marker, kf_free, v_kf, e_pt;
    std::vector<std::vector<int>> v_edges, v_medges;   // per free vertex: its monocular edges in slot order, its marker corner edges in edge order
    std::vector<uint8_t> vact;
};

struct Est {
    std::vector<SE3> pose;      // nkf keyframes, then nma markers
    std::vector<double> pt;
};

struct Lin {
    std::vector<double> Hll, bl, Hpp, bp, eblk, mblk, Dinv;
    std::vector<uint8_t> euse, muse;
    double chi, maxdiag;
};

bool pact(const Prob& P, int pi) { return P.off[pi + 1] > P.off[pi]; }

// the chi2 of a pass from the per-edge robust values: edge by edge, or the device's tree
double chi_sum(const Prob& P, const std::vector<double>& e_rho, const std::vector<double>& m_rho)
{
    if (P.order == 0) {
        double s = 0;
        for (int e = 0; e < P.nobs; e++) s += e_rho[e];
        for (int j = 0; j < P.nme; j++) s += m_rho[j];
        return s;
    }
    const int npb = (P.np + 63) / 64, nb = npb + (P.nme + 63) / 64;
    std::vector<double> part((size_t)nb, 0.);
    for (int b = 0; b < nb; b++) {
        double v[64];
        for (int l = 0; l < 64; l++) {
            double s = 0;
            if (b < npb) {
                const int pi = b * 64 + l;
                if (pi < P.np)
                    for (int e = P.off[pi]; e < P.off[pi + 1]; e++) s += e_rho[e];
            } else {
                const int j = (b - npb) * 64 + l;
                if (j < P.nme) s += m_rho[j];
            }
            v[l] = s;
        }
        part[(size_t)b] = butterfly64(v);
    }
    return runs256(part.data(), nb);
}

void linearize(const Prob& P, const Est& X, Lin& L)
{
    L.Hll.assign((size_t)P.np * 6, 0.); L.bl.assign((size_t)P.np * 3, 0.); L.Hpp.assign((size_t)P.nv * 36, 0.); L.bp.assign((size_t)P.nv * 6, 0.);
    L.eblk.assign((size_t)P.nobs * EB, 0.); L.mblk.assign((size_t)P.nme * MB, 0.);
    L.euse.assign((size_t)P.nobs, 0); L.muse.assign((size_t)P.nme, 0);
    L.Dinv.assign((size_t)P.np * 9, 0.);
    std::vector<double> e_rho((size_t)P.nobs, 0.), m_rho((size_t)P.nme, 0.);
    double md = 0;
    for (int pi = 0; pi < P.np; pi++) {
        const double* Xw = &X.pt[(size_t)pi * 3];
        double* H = &L.Hll[(size_t)pi * 6];
        double* b = &L.bl[(size_t)pi * 3];
        for (int e = P.off[pi]; e < P.off[pi + 1]; e++) {
            const int kf = P.okf[e];
            double err[2], Jp[2][6], Jx[2][3];
            mono_linearize(X.pose[(size_t)kf], Xw, P.oxy[2 * e], P.oxy[2 * e + 1], P.K, err, Jp, Jx);
            const double info = P.info[(size_t)e], ch = chi2_of(err, info);
            double rho[2] = {ch, 1.};
            if (P.robust) huber(ch, P.delta, rho);
            e_rho[e] = rho[0];
            const bool fin = all_finite(err, 2) && all_finite(&Jp[0][0], 12) && all_finite(&Jx[0][0], 6) && std::isfinite(rho[1]);
            const int vf = P.kf_free[(size_t)kf];
            L.euse[e] = fin ? (vf >= 0 ? 3 : 1) : 0;
            if (!fin) continue;
            const double w = rho[1] * info, r0 = rho[1] * -(info * err[0]), r1 = rho[1] * -(info * err[1]);
            int k = 0;
            for (int a = 0; a < 3; a++)
                for (int c = a; c < 3; c++, k++) H[k] += Jx[0][a] * (w * Jx[0][c]) + Jx[1][a] * (w * Jx[1][c]);
            for (int a = 0; a < 3; a++) b[a] += Jx[0][a] * r0 + Jx[1][a] * r1;
            if (vf >= 0) {
                double* out = &L.eblk[(size_t)e * EB];
                diag_block(Jp, w, r0, r1, out);
                for (int a = 0; a < 6; a++)
                    for (int c = 0; c < 3; c++) out[27 + a * 3 + c] = Jp[0][a] * (w * Jx[0][c]) + Jp[1][a] * (w * Jx[1][c]);
            }
        }
        if (pact(P, pi)) md = std::max(md, std::max(std::max(std::fabs(H[0]), std::fabs(H[3])), std::fabs(H[5])));
    }
    for (int j = 0; j < P.nme; j++) {
        const int o = j >> 2, k = j & 3, kf = P.mkf[o], m = P.mo_marker[(size_t)o];
        const SE3 &Tc = X.pose[(size_t)kf], &Tm = X.pose[(size_t)(P.nkf + m)];
        const double pm[3] = {P.mlocal[m * 12 + 3 * k], P.mlocal[m * 12 + 3 * k + 1], P.mlocal[m * 12 + 3 * k + 2]};
        const double ox = P.mcor[o * 8 + 2 * k], oy = P.mcor[o * 8 + 2 * k + 1];
        const bool camfree = P.kf_free[(size_t)kf] >= 0;
        double err[2], Jc[2][6] = {}, Jm[2][6], rho[2];
        marker_error(Tc, Tm, pm, ox, oy, P.K, err);
        huber(chi2_of(err, P.minfo), P.delta, rho);
        m_rho[j] = rho[0];
        if (camfree) marker_jacobian(Tc, Tm, true, pm, ox, oy, P.K, Jc);
        marker_jacobian(Tc, Tm, false, pm, ox, oy, P.K, Jm);
        const bool fin = all_finite(err, 2) && all_finite(&Jc[0][0], 12) && all_finite(&Jm[0][0], 12) && std::isfinite(rho[1]);
        L.muse[j] = fin;
        if (!fin) continue;
        const double w = rho[1] * P.minfo, r0 = rho[1] * -(P.minfo * err[0]), r1 = rho[1] * -(P.minfo * err[1]);
        double* out = &L.mblk[(size_t)j * MB];
        diag_block(Jc, w, r0, r1, out);
        diag_block(Jm, w, r0, r1, out + 27);
        for (int a = 0; a < 6; a++)
            for (int c = 0; c < 6; c++) out[54 + a * 6 + c] = Jc[0][a] * (w * Jm[0][c]) + Jc[1][a] * (w * Jm[1][c]);
    }
    L.chi = chi_sum(P, e_rho, m_rho);
    // the pose blocks
    for (int v = 0; v < P.nv; v++) {
        const std::vector<int>& ed = P.v_edges[(size_t)v];
        double s[27] = {};
        if (P.order == 0) {
            for (int e : ed) {
                if (L.euse[e] != 3) continue;
                for (int k = 0; k < 27; k++) s[k] += L.eblk[(size_t)e * EB + k];
            }
        } else {
            std::vector<double> th((size_t)256 * 27, 0.);
            const int n = (int)ed.size(), per = (n + 255) / 256;
            for (int t = 0; t < 256; t++) {
                const int lo = std::min(t * per, n), hi = std::min(lo + per, n);
                for (int it = lo; it < hi; it++) {
                    const int e = ed[(size_t)it];
                    if (L.euse[e] != 3) continue;
                    for (int k = 0; k < 27; k++) th[(size_t)k * 256 + t] += L.eblk[(size_t)e * EB + k];
                }
            }
            for (int k = 0; k < 27; k++) s[k] = block256(&th[(size_t)k * 256]);
        }
        const int side = P.v_kf[(size_t)v] < P.nkf ? 0 : 27;
        for (int j : P.v_medges[(size_t)v]) {
            if (!L.muse[j]) continue;
            for (int k = 0; k < 27; k++) s[k] += L.mblk[(size_t)j * MB + side + k];
        }
        double* H = &L.Hpp[(size_t)v * 36];
        int k = 0;
        double mv = 0;
        for (int a = 0; a < 6; a++)
            for (int c = a; c < 6; c++, k++) H[a * 6 + c] = H[c * 6 + a] = s[k];
        for (int a = 0; a < 6; a++) {
            L.bp[(size_t)v * 6 + a] = s[21 + a];
            mv = std::max(mv, std::fabs(H[a * 6 + a]));
        }
        if (P.vact[(size_t)v]) md = std::max(md, mv);
    }
    L.maxdiag = md;
}

// the reduced system of one trial, dense: S (n x n, n = 6 nv) and bs; Dinv of the points
void schur(const Prob& P, Lin& L, double lambda, std::vector<double>& S, std::vector<double>& bs)
{
    const int n = 6 * P.nv;
    S.assign((size_t)n * n, 0.);
    bs.assign((size_t)n, 0.);
    for (int pi = 0; pi < P.np; pi++) {
        if (!pact(P, pi)) continue;
        const double* H = &L.Hll[(size_t)pi * 6];
        const double m00 = H[0] + lambda, m01 = H[1], m02 = H[2], m11 = H[3] + lambda, m12 = H[4], m22 = H[5] + lambda;
        const double c00 = m11 * m22 - m12 * m12, c10 = m12 * m02 - m01 * m22, c20 = m01 * m12 - m11 * m02;
        const double det = c00 * m00 + c10 * m01 + c20 * m02, id = 1. / det;
        double* D = &L.Dinv[(size_t)pi * 9];
        D[0] = c00 * id; D[1] = c10 * id; D[2] = c20 * id;
        D[3] = D[1]; D[4] = (m00 * m22 - m02 * m02) * id; D[5] = (m02 * m01 - m00 * m12) * id;
        D[6] = D[2]; D[7] = D[5]; D[8] = (m00 * m11 - m01 * m01) * id;
    }
    auto contribution = [&](int ei, int ej, int pi, bool diag, double* acc, double* accb) {
        const double *Wi = &L.eblk[(size_t)ei * EB + 27], *Wj = &L.eblk[(size_t)ej * EB + 27], *D = &L.Dinv[(size_t)pi * 9], *bl = &L.bl[(size_t)pi * 3];
        for (int a = 0; a < 6; a++) {
            double Y[3];
            for (int c = 0; c < 3; c++) Y[c] = Wi[a * 3] * D[c] + Wi[a * 3 + 1] * D[3 + c] + Wi[a * 3 + 2] * D[6 + c];
            for (int b = 0; b < 6; b++) acc[a * 6 + b] += Y[0] * Wj[b * 3] + Y[1] * Wj[b * 3 + 1] + Y[2] * Wj[b * 3 + 2];
            if (diag) accb[a] += Y[0] * bl[0] + Y[1] * bl[1] + Y[2] * bl[2];
        }
    };
    // the items of every pair (u <= v) of free keyframes: (edge of u, edge of v) of the points both see, in point order
    const int nf = (int)std::count_if(P.v_kf.begin(), P.v_kf.end(), [&](int k) { return k < P.nkf; });
    std::vector<std::vector<int>> items((size_t)nf * nf);
    for (int pi = 0; pi < P.np; pi++)
        for (int e = P.off[pi]; e < P.off[pi + 1]; e++) {
            const int ve = P.kf_free[(size_t)P.okf[e]];
            if (ve < 0) continue;
            for (int f = e; f < P.off[pi + 1]; f++) {
                const int vf = P.kf_free[(size_t)P.okf[f]];
                if (vf < 0) continue;
                std::vector<int>& it = items[(size_t)std::min(ve, vf) * nf + std::max(ve, vf)];
                it.push_back(ve <= vf ? e : f);
                it.push_back(ve <= vf ? f : e);
            }
        }
    for (int i = 0; i < P.nv; i++)
        for (int j = i; j < P.nv; j++) {
            const int ki = P.v_kf[(size_t)i], kj = P.v_kf[(size_t)j];
            double B[36] = {}, acc[36] = {}, accb[6] = {};
            if (ki < P.nkf && kj < P.nkf) {
                const std::vector<int>& it = items[(size_t)i * nf + j];
                const int n2 = (int)it.size() / 2;
                auto usable = [&](int k) { return L.euse[it[(size_t)2 * k]] == 3 && L.euse[it[(size_t)2 * k + 1]] == 3; };
                if (P.order == 0) {
                    for (int k = 0; k < n2; k++)
                        if (usable(k)) contribution(it[(size_t)2 * k], it[(size_t)2 * k + 1], P.e_pt[(size_t)it[(size_t)2 * k]], i == j, acc, accb);
                } else if (n2 > 0) {
                    std::vector<double> th((size_t)42 * 64, 0.);
                    const int per = (n2 + 63) / 64;
                    for (int t = 0; t < 64; t++) {
                        double a36[36] = {}, a6[6] = {};
                        const int lo = std::min(t * per, n2), hi = std::min(lo + per, n2);
                        for (int k = lo; k < hi; k++)
                            if (usable(k)) contribution(it[(size_t)2 * k], it[(size_t)2 * k + 1], P.e_pt[(size_t)it[(size_t)2 * k]], i == j, a36, a6);
                        for (int k = 0; k < 36; k++) th[(size_t)k * 64 + t] = a36[k];
                        for (int k = 0; k < 6; k++) th[(size_t)(36 + k) * 64 + t] = a6[k];
                    }
                    for (int k = 0; k < 36; k++) acc[k] = butterfly64(&th[(size_t)k * 64]);
                    for (int k = 0; k < 6; k++) accb[k] = butterfly64(&th[(size_t)(36 + k) * 64]);
                }
            }
            const bool act = P.vact[(size_t)i] != 0;
            if (i == j && !act) {
                for (int a = 0; a < 6; a++) B[a * 6 + a] = 1;
            } else if (i == j) {
                for (int k = 0; k < 36; k++) B[k] = L.Hpp[(size_t)i * 36 + k];
                for (int a = 0; a < 6; a++) B[a * 6 + a] += lambda;
                for (int k = 0; k < 36; k++) B[k] -= acc[k];
            } else if (kj < P.nkf) {
                for (int k = 0; k < 36; k++) B[k] = 0. - acc[k];
            } else if (ki < P.nkf) {
                const int m = kj - P.nkf;
                for (int e = 4 * P.moff[m]; e < 4 * P.moff[m + 1]; e++) {
                    if (P.mkf[e >> 2] != ki || !L.muse[e]) continue;
                    for (int k = 0; k < 36; k++) B[k] += L.mblk[(size_t)e * MB + 54 + k];
                }
            }
            for (int a = 0; a < 6; a++)
                for (int b = 0; b < 6; b++) S[(size_t)(6 * i + a) * n + 6 * j + b] = S[(size_t)(6 * j + b) * n + 6 * i + a] = B[a * 6 + b];
            if (i == j)
                for (int a = 0; a < 6; a++) bs[(size_t)6 * i + a] = act ? L.bp[(size_t)6 * i + a] - accb[a] : 0.;
        }
}

// L L^T in place, right-looking, no pivoting; then the two substitutions.  x is untouched when a pivot fails.
bool llt_solve(std::vector<double>& S, int n, const std::vector<double>& b, double* x)
{
    for (int k = 0; k < n; k++) {
        const double d = S[(size_t)k * n + k];
        if (!(d > 0) || !std::isfinite(d)) return false;
        const double lkk = S[(size_t)k * n + k] = std::sqrt(d);
        for (int i = k + 1; i < n; i++) S[(size_t)i * n + k] /= lkk;
        for (int i = k + 1; i < n; i++) {
            const double lik = S[(size_t)i * n + k];
            if (lik == 0) continue;   // a zero adds nothing: S is block-sparse
            for (int j = k + 1; j <= i; j++) S[(size_t)i * n + j] -= lik * S[(size_t)j * n + k];
        }
    }
    std::vector<double> y(b);
    for (int k = 0; k < n; k++) {
        y[(size_t)k] /= S[(size_t)k * n + k];
        for (int i = k + 1; i < n; i++) y[(size_t)i] -= S[(size_t)i * n + k] * y[(size_t)k];
    }
    for (int k = n - 1; k >= 0; k--) {
        y[(size_t)k] /= S[(size_t)k * n + k];
        for (int i = 0; i < k; i++) y[(size_t)i] -= S[(size_t)k * n + i] * y[(size_t)k];
    }
    for (int i = 0; i < n; i++) x[i] = y[(size_t)i];
    return true;
}

// one trial: the reduced solve, the updates, the trial estimates and their chi2.  Returns ok2.
bool trial(const Prob& P, Lin& L, double lambda, const Est& X, Est& Xt, std::vector<double>& xv, std::vector<double>& xl, double& tempChi,
           double& scale)
{
    std::vector<double> S, bs;
    schur(P, L, lambda, S, bs);
    const bool ok = llt_solve(S, 6 * P.nv, bs, xv.data());
    Xt = X;
    for (int v = 0; v < P.nv; v++)
        if (P.vact[(size_t)v]) {
            const int idx = P.v_kf[(size_t)v];
            Xt.pose[(size_t)idx] = mul(se3_exp(&xv[(size_t)v * 6]), X.pose[(size_t)idx]);
        }
    std::vector<double> e_rho((size_t)P.nobs, 0.), m_rho((size_t)P.nme, 0.), sc((size_t)P.np, 0.);
    for (int pi = 0; pi < P.np; pi++) {
        if (!pact(P, pi)) continue;
        double* x = &xl[(size_t)pi * 3];
        const double* bl = &L.bl[(size_t)pi * 3];
        if (ok) {
            double r[3] = {bl[0], bl[1], bl[2]};
            for (int e = P.off[pi]; e < P.off[pi + 1]; e++) {
                if (L.euse[e] != 3) continue;
                const double* W = &L.eblk[(size_t)e * EB + 27];
                const double* xp = &xv[(size_t)P.kf_free[(size_t)P.okf[e]] * 6];
                for (int c = 0; c < 3; c++) {
                    double s = 0;
                    for (int a = 0; a < 6; a++) s += W[a * 3 + c] * xp[a];
                    r[c] -= s;
                }
            }
            const double* D = &L.Dinv[(size_t)pi * 9];
            for (int a = 0; a < 3; a++) x[a] = D[a * 3] * r[0] + D[a * 3 + 1] * r[1] + D[a * 3 + 2] * r[2];
        }
        double s = 0;
        for (int a = 0; a < 3; a++) {
            s += x[a] * (lambda * x[a] + bl[a]);
            Xt.pt[(size_t)pi * 3 + a] = X.pt[(size_t)pi * 3 + a] + x[a];
        }
        sc[(size_t)pi] = s;
        for (int e = P.off[pi]; e < P.off[pi + 1]; e++) {
            double err[2], rho[2];
            mono_error(Xt.pose[(size_t)P.okf[e]], &Xt.pt[(size_t)pi * 3], P.oxy[2 * e], P.oxy[2 * e + 1], P.K, err);
            const double ch = chi2_of(err, P.info[(size_t)e]);
            rho[0] = ch;
            if (P.robust) huber(ch, P.delta, rho);
            e_rho[e] = rho[0];
        }
    }
    for (int j = 0; j < P.nme; j++) {
        const int o = j >> 2, k = j & 3, m = P.mo_marker[(size_t)o];
        const double pm[3] = {P.mlocal[m * 12 + 3 * k], P.mlocal[m * 12 + 3 * k + 1], P.mlocal[m * 12 + 3 * k + 2]};
        double err[2], rho[2];
        marker_error(Xt.pose[(size_t)P.mkf[o]], Xt.pose[(size_t)(P.nkf + m)], pm, P.mcor[o * 8 + 2 * k], P.mcor[o * 8 + 2 * k + 1], P.K, err);
        huber(chi2_of(err, P.minfo), P.delta, rho);
        m_rho[j] = rho[0];
    }
    tempChi = chi_sum(P, e_rho, m_rho);
    std::vector<double> xs((size_t)6 * P.nv, 0.);
    for (int j = 0; j < 6 * P.nv; j++) xs[(size_t)j] = xv[(size_t)j] * (lambda * xv[(size_t)j] + (P.vact[(size_t)(j / 6)] ? L.bp[(size_t)j] : 0.));
    if (P.order == 0) {
        double s = 0;
        for (double v : xs) s += v;
        for (int pi = 0; pi < P.np; pi++) s += sc[(size_t)pi];
        scale = s;
    } else {
        const int npb = (P.np + 63) / 64, nb = npb + (P.nme + 63) / 64;
        std::vector<double> part((size_t)nb, 0.);
        for (int b = 0; b < npb; b++) {
            double v[64];
            for (int l = 0; l < 64; l++) v[l] = b * 64 + l < P.np ? sc[(size_t)(b * 64 + l)] : 0.;
            part[(size_t)b] = butterfly64(v);
        }
        const double sp = runs256(part.data(), nb);
        scale = runs256(xs.data(), 6 * P.nv) + sp;
    }
    return ok;
}

void setup(Prob& P, Est& X, const float* Tcw, const uint8_t* kf_fixed, int nkf, const float* x3Dw, int np, const int32_t* obs_offset,
           const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4, const float* inv_sigma2,
           const float* Twm, const float* marker_local, int nma, const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners,
           int nmobs, float marker_info, int use_markers, int robust, int order)
{
    static const int32_t zero2[2] = {0, 0};
    P.nkf = nkf; P.np = np; P.nobs = nobs; P.nma = nma; P.nmobs = nmobs; P.nme = use_markers ? 4 * nmobs : 0; P.order = order;
    P.robust = robust != 0;
    P.off = np ? obs_offset : zero2; P.okf = obs_kf; P.oxy = obs_xy;
    P.K = Cam{K4[0], K4[1], K4[2], K4[3]};
    P.delta = (double)(float)std::sqrt(5.99);
    P.minfo = marker_info;
    P.mlocal = marker_local; P.moff = nma ? mobs_offset : zero2; P.mkf = mobs_kf; P.mcor = mobs_corners;
    P.info.resize((size_t)nobs);
    for (int e = 0; e < nobs; e++) P.info[(size_t)e] = inv_sigma2[obs_octave[e]];
    P.mo_marker.assign((size_t)nmobs, 0);
    for (int m = 0; m < nma; m++)
        for (int o = mobs_offset[m]; o < mobs_offset[m + 1]; o++) P.mo_marker[(size_t)o] = m;
    P.kf_free.assign((size_t)nkf, -1);
    P.v_kf.clear();
    for (int k = 0; k < nkf; k++)
        if (!kf_fixed[k]) {
            P.kf_free[(size_t)k] = (int)P.v_kf.size();
            P.v_kf.push_back(k);
        }
    const int nf = (int)P.v_kf.size();
    for (int m = 0; use_markers && m < nma; m++) P.v_kf.push_back(nkf + m);
    P.nv = (int)P.v_kf.size();
    P.v_edges.assign((size_t)P.nv, {});
    P.v_medges.assign((size_t)P.nv, {});
    P.e_pt.assign((size_t)nobs, 0);
    for (int pi = 0; pi < np; pi++)
        for (int e = obs_offset[pi]; e < obs_offset[pi + 1]; e++) {
            P.e_pt[(size_t)e] = pi;
            if (P.kf_free[(size_t)obs_kf[e]] >= 0) P.v_edges[(size_t)P.kf_free[(size_t)obs_kf[e]]].push_back(e);
        }
    for (int j = 0; j < P.nme; j++) {
        if (P.kf_free[(size_t)mobs_kf[j >> 2]] >= 0) P.v_medges[(size_t)P.kf_free[(size_t)mobs_kf[j >> 2]]].push_back(j);
        P.v_medges[(size_t)(nf + P.mo_marker[(size_t)(j >> 2)])].push_back(j);
    }
    P.vact.assign((size_t)P.nv, 0);
    for (int v = 0; v < P.nv; v++) P.vact[(size_t)v] = !P.v_edges[(size_t)v].empty() || !P.v_medges[(size_t)v].empty();
    X.pose.resize((size_t)(nkf + nma));
    for (int k = 0; k < nkf; k++) X.pose[(size_t)k] = se3_from_float(Tcw + 12 * k);
    for (int m = 0; m < nma; m++) X.pose[(size_t)(nkf + m)] = se3_from_float(Twm + 12 * m);
    X.pt.resize((size_t)np * 3);
    for (int i = 0; i < 3 * np; i++) X.pt[(size_t)i] = x3Dw[i];
}

} // namespace

// Tcw, x3Dw, Twm are in / out as in the library.  iterations may exceed the library's 20: the noise-free tests give a case more.
// err_out (may be NULL): the error of every edge at the final estimates, in double before they are rounded to float: 2 per monocular
// edge, then 2 per marker corner edge.
extern "C" int ref_gba(float* Tcw, const uint8_t* kf_fixed, int nkf, float* x3Dw, int np, const int32_t* obs_offset, const int32_t* obs_kf,
                       const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4, const float* inv_sigma2, int nlevels,
                       float* Twm, const float* marker_local, int nma, const int32_t* mobs_offset, const int32_t* mobs_kf,
                       const float* mobs_corners, int nmobs, float marker_info, int use_markers, int iterations, int robust, int order, Result* res,
                       double* err_out)
{
    (void)nlevels;
    std::memset(res, 0, sizeof(*res));
    Prob P;
    Est X, Xt;
    setup(P, X, Tcw, kf_fixed, nkf, x3Dw, np, obs_offset, obs_kf, obs_xy, obs_octave, nobs, K4, inv_sigma2, Twm, marker_local, nma, mobs_offset,
          mobs_kf, mobs_corners, nmobs, marker_info, use_markers, robust, order);
    std::vector<double> xv((size_t)6 * std::max(P.nv, 1), 0.), xl((size_t)3 * std::max(np, 1), 0.);
    res->n_edges_mono = nobs;
    res->n_edges_marker = P.nme;
    for (int pi = 0; pi < np; pi++) res->n_points_left_out += !pact(P, pi);
    Levenberg c;
    lm_begin(c);
    Lin L;
    int it = 0;
    while (it < iterations) {
        linearize(P, X, L);
        lm_linearised(c, L.chi, it == 0, L.maxdiag);
        if (it == 0) res->chi2_first = L.chi;
        do {
            double tempChi, scale;
            const bool ok2 = trial(P, L, c.lambda, X, Xt, xv, xl, tempChi, scale);
            if (lm_trial(c, tempChi, ok2, scale)) X = Xt;
            res->trials++;
        } while (lm_again(c));
        it++;
        if (lm_iteration_end(c)) break;
    }
    for (int e = 0; e < nobs && err_out; e++)
        mono_error(X.pose[(size_t)obs_kf[e]], &X.pt[(size_t)P.e_pt[(size_t)e] * 3], obs_xy[2 * e], obs_xy[2 * e + 1], P.K, err_out + 2 * e);
    for (int j = 0; j < P.nme && err_out; j++) {
        const int o = j >> 2, k = j & 3, m = P.mo_marker[(size_t)o];
        const double pm[3] = {marker_local[m * 12 + 3 * k], marker_local[m * 12 + 3 * k + 1], marker_local[m * 12 + 3 * k + 2]};
        marker_error(X.pose[(size_t)mobs_kf[o]], X.pose[(size_t)(nkf + m)], pm, mobs_corners[o * 8 + 2 * k], mobs_corners[o * 8 + 2 * k + 1], P.K,
                     err_out + 2 * (nobs + j));
    }
    res->iterations = it;
    res->chi2_last = it ? c.currentChi : 0.;
    res->lambda_last = c.lambda;
    for (int v = 0; v < P.nv; v++) {
        if (!P.vact[(size_t)v]) continue;
        const int idx = P.v_kf[(size_t)v];
        to_float(X.pose[(size_t)idx], idx < nkf ? Tcw + 12 * idx : Twm + 12 * (idx - nkf));
    }
    for (int pi = 0; pi < np; pi++)
        if (pact(P, pi))
            for (int a = 0; a < 3; a++) x3Dw[3 * pi + a] = (float)X.pt[(size_t)pi * 3 + a];
    return 0;
}

// One linearisation and the first trial, as orbfe_gba_inspect.  full_H (may be NULL): the whole system with lambda0 on its diagonal,
// (6 nv + 3 np)^2 row-major, poses first; b holds its right-hand side.  A vertex without an edge and a point without observations
// hold lambda0 alone there.  S_out (may be NULL): the dense reduced system, (6 nv)^2.
extern "C" int ref_gba_inspect(const float* Tcw, const uint8_t* kf_fixed, int nkf, const float* x3Dw, int np, const int32_t* obs_offset,
                               const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                               const float* inv_sigma2, int nlevels, const float* Twm, const float* marker_local, int nma,
                               const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs, float marker_info,
                               int use_markers, int robust, int order, int32_t* nv, double* b, double* Hpp, double* Hll, double* chi2, double* x,
                               double* full_H, double* S_out)
{
    (void)nlevels;
    Prob P;
    Est X, Xt;
    setup(P, X, Tcw, kf_fixed, nkf, x3Dw, np, obs_offset, obs_kf, obs_xy, obs_octave, nobs, K4, inv_sigma2, Twm, marker_local, nma, mobs_offset,
          mobs_kf, mobs_corners, nmobs, marker_info, use_markers, robust, order);
    Lin L;
    linearize(P, X, L);
    const double lambda = 1e-5 * L.maxdiag;
    *nv = P.nv;
    chi2[0] = L.chi;
    chi2[1] = lambda;
    std::memcpy(b, L.bp.data(), (size_t)P.nv * 48);
    std::memcpy(b + 6 * P.nv, L.bl.data(), (size_t)np * 24);
    std::memcpy(Hpp, L.Hpp.data(), (size_t)P.nv * 288);
    std::memcpy(Hll, L.Hll.data(), (size_t)np * 48);
    if (full_H) {
        const int n = 6 * P.nv + 3 * np, nf = P.nv - (use_markers ? nma : 0);
        std::fill(full_H, full_H + (size_t)n * n, 0.);
        auto at = [&](int r, int c) -> double& { return full_H[(size_t)r * n + c]; };
        for (int v = 0; v < P.nv; v++)
            for (int a = 0; a < 6; a++)
                for (int c = 0; c < 6; c++) at(6 * v + a, 6 * v + c) = L.Hpp[(size_t)v * 36 + a * 6 + c] + (a == c ? lambda : 0.);
        for (int pi = 0; pi < np; pi++) {
            const double* H = &L.Hll[(size_t)pi * 6];
            const int o = 6 * P.nv + 3 * pi, idx[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 3; c++) at(o + a, o + c) = H[idx[a][c]] + (a == c ? lambda : 0.);
            for (int e = P.off[pi]; e < P.off[pi + 1]; e++) {
                if (L.euse[(size_t)e] != 3) continue;
                const int v = P.kf_free[(size_t)obs_kf[e]];
                for (int a = 0; a < 6; a++)
                    for (int c = 0; c < 3; c++) at(6 * v + a, o + c) = at(o + c, 6 * v + a) = L.eblk[(size_t)e * EB + 27 + a * 3 + c];
            }
        }
        for (int j = 0; j < P.nme; j++) {
            const int vc = P.kf_free[(size_t)mobs_kf[j >> 2]], vm = nf + P.mo_marker[(size_t)(j >> 2)];
            if (vc < 0 || !L.muse[(size_t)j]) continue;
            for (int a = 0; a < 6; a++)
                for (int c = 0; c < 6; c++) {
                    at(6 * vc + a, 6 * vm + c) += L.mblk[(size_t)j * MB + 54 + a * 6 + c];
                    at(6 * vm + c, 6 * vc + a) += L.mblk[(size_t)j * MB + 54 + a * 6 + c];
                }
        }
    }
    if (S_out) {
        std::vector<double> S, bs;
        schur(P, L, lambda, S, bs);
        std::memcpy(S_out, S.data(), S.size() * 8);
    }
    std::vector<double> xv((size_t)6 * std::max(P.nv, 1), 0.), xl((size_t)3 * std::max(np, 1), 0.);
    double tempChi, scale;
    chi2[2] = trial(P, L, lambda, X, Xt, xv, xl, tempChi, scale) ? 1. : 0.;
    std::memcpy(x, xv.data(), (size_t)P.nv * 48);
    std::memcpy(x + 6 * P.nv, xl.data(), (size_t)np * 24);
    return 0;
}

// One EdgeSE3ProjectXYZ at exp(u) * Tcw and X: the error and g2o's analytic Jacobians (pose 2 x 6, point 2 x 3)
extern "C" void ref_gba_mono_edge(const float* Tcw, const double* u, const double* X, const double* obs, const float* K4, double* err,
                                  double* Jp, double* Jx)
{
    const Cam K{K4[0], K4[1], K4[2], K4[3]};
    const SE3 T = mul(se3_exp(u), se3_from_float(Tcw));
    double e[2], jp[2][6], jx[2][3];
    mono_linearize(T, X, obs[0], obs[1], K, e, jp, jx);
    std::memcpy(err, e, sizeof(e));
    std::memcpy(Jp, jp, sizeof(jp));
    std::memcpy(Jx, jx, sizeof(jx));
}

// One EdgeMarker: the error and g2o's numeric Jacobians on the camera and on the marker vertex
extern "C" void ref_gba_marker_edge(const float* Tcw, const float* Twm, const double* p, const double* obs, const float* K4, double* err,
                                    double* Jc, double* Jm)
{
    const Cam K{K4[0], K4[1], K4[2], K4[3]};
    const SE3 Tc = se3_from_float(Tcw), Tm = se3_from_float(Twm);
    double e[2], jc[2][6], jm[2][6];
    marker_error(Tc, Tm, p, obs[0], obs[1], K, e);
    marker_jacobian(Tc, Tm, true, p, obs[0], obs[1], K, jc);
    marker_jacobian(Tc, Tm, false, p, obs[0], obs[1], K, jm);
    std::memcpy(err, e, sizeof(e));
    std::memcpy(Jc, jc, sizeof(jc));
    std::memcpy(Jm, jm, sizeof(jm));
}
