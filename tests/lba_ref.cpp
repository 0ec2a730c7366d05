// lba_ref.cpp -- CPU restatement of ORB_SLAM2's Optimizer::LocalBundleAdjustment (src/Optimizer.cc:892-1242 of the reference, behind
// its collect step, with this fork's marker poses as free SE3 vertices) for the parity tests of orbfe_local_bundle_adjustment*.
// No g2o or Eigen here; the pieces are restated from their algorithms, SE3Quat, the Huber kernel and the Levenberg-Marquardt rules in
// tests/g2o_ref.hpp (shared by the restatements), and what this one has in common with tests/gba_ref.cpp in tests/ba_ref.hpp:
//   EdgeSE3ProjectXYZ        e = obs - pi(T Xw), Omega = invSigma2 I, g2o's analytic Jacobians for the point and the pose
//   EdgeMarker               e = obs - pi((Tcw Twm) p), Omega = w I, numeric Jacobians on both vertices: central differences,
//                            delta = 1e-9, through exp(+-delta e_d) * estimate; none for a fixed keyframe
//   BlockSolver_6_3          Hpp (6 x 6 per free pose vertex), Hll (3 x 3 per point), Hpl per edge; fixed vertices have no block;
//                            S = Hpp - sum Hpl Hll^-1 Hpl^T with Hll^-1 by cofactors; S = L L^T without pivoting (a pivot that is not
//                            positive and finite fails the solve); points by back-substitution
//   Levenberg-Marquardt      lambda0 = 1e-5 max diagonal over pose and point blocks, up to 10 trials an iteration,
//                            rho = dchi / (sum x (lambda x + b) + 1e-3), g2o's lambda / nu and stop rules
//   two rounds               optimize(5) with Huber on all edges; first check (chi2 > 5.991 or depth <= 0 -> level 1); optimize(10)
//                            on level 0 without Huber; second check -> the erase flags.  The checks read the cached errors: those of
//                            the last evaluation of the edge (a rejected trial's when the round ended on one; round 1's for level 1)
// Two summation orders: 0 = g2o's (every block and the chi2 summed edge by edge in insertion order, S reduced point by point),
// 1 = the device's (a point's observations in order; a pose block over contiguous runs of points, one run a thread of 256, the
// threads by a butterfly inside each wave of 64 and the waves in order; a block of S the same over 64 threads; the chi2 by waves
// of 64 points, then runs of those partial sums over 256 threads).
// Built by tests/lba_build.py (g++ -O2 -ffp-contract=off) and loaded with ctypes.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ba_ref.hpp"

namespace {

struct Result {     // the layout of orbfe_lba_result
    int32_t n_edges_mono, n_edges_marker;
    int32_t n_level1[2];
    int32_t n_erase;
    int32_t iterations[2];
    int32_t stale_mask;
    int32_t status;
};

// ------------------------------------------------------------------------------------------ the problem --
constexpr int MAXV = 64;

struct Prob : Core {
    bool fix_points = false;   // the anchor's hook: the points are held, only pose blocks are built (what a motion-only optimization solves)
    std::vector<int> tbl;      // the edge of keyframe kf and point pi at kf * np + pi, or -1
};

struct LbaLin : Lin {   // with the activity of the round: a point with an edge at level 0, a vertex with one
    std::vector<uint8_t> pact, vact;
};

struct Cache {
    std::vector<double> e_chi2, m_chi2;
    std::vector<uint8_t> e_level, m_level;
};

void linearize(const Prob& P, const Est& X, bool robust, Cache& C, LbaLin& L)
{
    lin_clear(P, L);
    L.pact.assign((size_t)P.np, 0); L.vact.assign((size_t)P.nv, 0);
    std::vector<double> e_rho((size_t)P.nobs, 0.), m_rho((size_t)P.nme, 0.);
    double md = 0;
    for (int pi = 0; pi < P.np; pi++) {
        const double* H = &L.Hll[(size_t)pi * 6];
        int nact = 0;
        for (int e = P.off[pi]; e < P.off[pi + 1]; e++) {
            if (C.e_level[e]) continue;
            nact++;
            mono_edge_add(P, X, robust, pi, e, L, C.e_chi2[e], e_rho[e]);
        }
        L.pact[pi] = nact > 0 && !P.fix_points;
        if (L.pact[pi]) md = std::max(md, std::max(std::max(std::fabs(H[0]), std::fabs(H[3])), std::fabs(H[5])));
    }
    for (int j = 0; j < P.nme; j++)
        if (!C.m_level[j]) corner_edge_add(P, X, robust, j, L, C.m_chi2[j], m_rho[j]);
    L.chi = chi_sum(P, e_rho, m_rho, C.e_level.data(), C.m_level.data());
    // the pose blocks
    for (int v = 0; v < P.nv; v++) {
        const int kf = P.v_kf[(size_t)v];
        double s[28] = {};
        if (kf < P.nkf) {
            if (P.order == 0) {
                for (int e = 0; e < P.nobs; e++) {
                    if (P.okf[e] != kf || C.e_level[e]) continue;
                    s[27] += 1;
                    if (L.euse[e] != 3) continue;
                    for (int k = 0; k < 27; k++) s[k] += L.eblk[(size_t)e * EB + k];
                }
            } else {
                std::vector<double> th((size_t)256 * 28, 0.);
                const int per = (P.np + 255) / 256;
                for (int t = 0; t < 256; t++) {
                    const int lo = std::min(t * per, P.np), hi = std::min(lo + per, P.np);
                    for (int pi = lo; pi < hi; pi++) {
                        const int e = P.tbl[(size_t)kf * P.np + pi];
                        if (e < 0 || C.e_level[e]) continue;
                        th[(size_t)27 * 256 + t] += 1;
                        if (L.euse[e] != 3) continue;
                        for (int k = 0; k < 27; k++) th[(size_t)k * 256 + t] += L.eblk[(size_t)e * EB + k];
                    }
                }
                for (int k = 0; k < 28; k++) s[k] = block256(&th[(size_t)k * 256]);
            }
            for (int j = 0; j < P.nme; j++) {
                if (P.mkf[j >> 2] != kf || C.m_level[j]) continue;
                s[27] += 1;
                if (!L.muse[j]) continue;
                for (int k = 0; k < 27; k++) s[k] += L.mblk[(size_t)j * MB + k];
            }
        } else {
            const int m = kf - P.nkf;
            for (int j = 4 * P.moff[m]; j < 4 * P.moff[m + 1]; j++) {
                if (C.m_level[j]) continue;
                s[27] += 1;
                if (!L.muse[j]) continue;
                for (int k = 0; k < 27; k++) s[k] += L.mblk[(size_t)j * MB + 27 + k];
            }
        }
        const double mv = pose_block_store(s, v, L);
        L.vact[v] = s[27] > 0;
        if (s[27] > 0) md = std::max(md, mv);
    }
    L.maxdiag = md;
}

// the reduced system of one trial: S (n x n, n = 6 nv) and bs; Dinv of the active points
void schur(const Prob& P, const Cache& C, LbaLin& L, double lambda, std::vector<double>& S, std::vector<double>& bs)
{
    const int n = 6 * P.nv;
    S.assign((size_t)n * n, 0.);
    bs.assign((size_t)n, 0.);
    for (int pi = 0; pi < P.np; pi++)
        if (L.pact[pi]) damped_inverse(L, pi, lambda);
    for (int i = 0; i < P.nv; i++)
        for (int j = i; j < P.nv; j++) {
            const int ki = P.v_kf[(size_t)i], kj = P.v_kf[(size_t)j];
            const bool act = L.vact[i] && L.vact[j];
            double B[36] = {}, acc[36] = {}, accb[6] = {};
            if (act && ki < P.nkf && kj < P.nkf) {
                auto usable = [&](int pi, int& ei, int& ej) {
                    if (!L.pact[pi]) return false;
                    ei = P.tbl[(size_t)ki * P.np + pi];
                    ej = P.tbl[(size_t)kj * P.np + pi];
                    return ei >= 0 && ej >= 0 && !C.e_level[ei] && !C.e_level[ej] && L.euse[ei] == 3 && L.euse[ej] == 3;
                };
                if (P.order == 0) {
                    for (int pi = 0; pi < P.np; pi++) {
                        int ei, ej;
                        if (usable(pi, ei, ej)) schur_contribution(L, ei, ej, pi, i == j, acc, accb);
                    }
                } else {
                    std::vector<double> th((size_t)42 * 64, 0.);
                    const int per = (P.np + 63) / 64;
                    for (int t = 0; t < 64; t++) {
                        double a36[36] = {}, a6[6] = {};
                        const int lo = std::min(t * per, P.np), hi = std::min(lo + per, P.np);
                        for (int pi = lo; pi < hi; pi++) {
                            int ei, ej;
                            if (usable(pi, ei, ej)) schur_contribution(L, ei, ej, pi, i == j, a36, a6);
                        }
                        for (int k = 0; k < 36; k++) th[(size_t)k * 64 + t] = a36[k];
                        for (int k = 0; k < 6; k++) th[(size_t)(36 + k) * 64 + t] = a6[k];
                    }
                    lanes_sum(th, acc, accb);
                }
            }
            if (!act) {
                if (i == j)
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
                    if (P.mkf[e >> 2] != ki || C.m_level[e] || !L.muse[e]) continue;
                    for (int k = 0; k < 36; k++) B[k] += L.mblk[(size_t)e * MB + 54 + k];
                }
            }
            schur_store(P, L, i, j, B, act, accb, S, bs);
        }
}

// one trial: the reduced solve, the updates, the trial estimates and their chi2 (written to the cache).  Returns ok2.
bool trial(const Prob& P, Cache& C, LbaLin& L, double lambda, bool robust, const Est& X, Est& Xt, std::vector<double>& xv, std::vector<double>& xl,
           double& tempChi, double& scale_points)
{
    std::vector<double> S, bs;
    schur(P, C, L, lambda, S, bs);
    const bool ok = llt_solve(S, 6 * P.nv, bs, xv.data(), false);
    Xt = X;
    for (int v = 0; v < P.nv; v++)
        if (L.vact[v]) {
            const int idx = P.v_kf[(size_t)v];
            Xt.pose[(size_t)idx] = mul(se3_exp(&xv[(size_t)v * 6]), X.pose[(size_t)idx]);
        }
    std::vector<double> e_rho((size_t)P.nobs, 0.), m_rho((size_t)P.nme, 0.), sc((size_t)P.np, 0.);
    for (int pi = 0; pi < P.np; pi++) {
        if (!L.pact[pi] && !P.fix_points) continue;
        double* x = &xl[(size_t)pi * 3];
        const double* bl = &L.bl[(size_t)pi * 3];
        if (ok && L.pact[pi]) back_substitute(P, L, pi, xv, x);
        double s = 0;
        for (int a = 0; a < 3 && L.pact[pi]; a++) {
            s += x[a] * (lambda * x[a] + bl[a]);
            Xt.pt[(size_t)pi * 3 + a] = X.pt[(size_t)pi * 3 + a] + x[a];
        }
        sc[(size_t)pi] = s;
        for (int e = P.off[pi]; e < P.off[pi + 1]; e++) {
            if (C.e_level[e]) continue;
            double err[2], rho[2];
            mono_error(Xt.pose[(size_t)P.okf[e]], &Xt.pt[(size_t)pi * 3], P.oxy[2 * e], P.oxy[2 * e + 1], P.K, err);
            const double ch = chi2_of(err, P.info[(size_t)e]);
            C.e_chi2[e] = ch;
            rho[0] = ch;
            if (robust) huber(ch, P.delta, rho);
            e_rho[e] = rho[0];
        }
    }
    for (int j = 0; j < P.nme; j++) {
        if (C.m_level[j]) continue;
        double err[2], rho[2];
        corner_error(P, Xt, j, err);
        const double ch = chi2_of(err, P.minfo);
        C.m_chi2[j] = ch;
        rho[0] = ch;
        if (robust) huber(ch, P.delta, rho);
        m_rho[j] = rho[0];
    }
    tempChi = chi_sum(P, e_rho, m_rho, C.e_level.data(), C.m_level.data());
    if (P.order == 0) {
        double s = 0;
        for (int pi = 0; pi < P.np; pi++) s += sc[(size_t)pi];
        scale_points = s;
    } else {
        scale_points = points_scale_device(P, sc);
    }
    return ok;
}

// optimize(maxit): returns the iterations run; `stale` = the last trial was rejected
int optimize(const Prob& P, Cache& C, Est& X, bool robust, int maxit, std::vector<double>& xv, std::vector<double>& xl, bool& stale)
{
    Levenberg c;
    lm_begin(c);
    stale = false;
    int it = 0;
    LbaLin L;
    Est Xt;
    while (it < maxit) {
        linearize(P, X, robust, C, L);
        lm_linearised(c, L.chi, it == 0, L.maxdiag);
        do {
            double tempChi, sp;
            const bool ok2 = trial(P, C, L, c.lambda, robust, X, Xt, xv, xl, tempChi, sp);
            double scale = 0;
            for (int j = 0; j < 6 * P.nv; j++) scale += xv[(size_t)j] * (c.lambda * xv[(size_t)j] + (L.vact[j / 6] ? L.bp[(size_t)j] : 0.));
            scale += sp;
            stale = !lm_trial(c, tempChi, ok2, scale);
            if (!stale) X = Xt;
        } while (lm_again(c));
        it++;
        if (lm_iteration_end(c)) break;
    }
    return it;
}

// the Huber constant is the reference's for this optimizer, sqrt(5.991); tests/gba_ref.cpp has the reference's other one, on purpose
bool setup(Prob& P, Est& X, const Flat& f, int order)
{
    setup_core(P, X, f, order, (double)(float)std::sqrt(5.991));
    P.tbl.assign((size_t)std::max(f.nkf, 1) * std::max(f.np, 1), -1);
    for (int pi = 0; pi < f.np; pi++)
        for (int e = f.obs_offset[pi]; e < f.obs_offset[pi + 1]; e++) P.tbl[(size_t)f.obs_kf[e] * f.np + pi] = e;
    return P.nv <= MAXV;
}

void cache_clear(const Prob& P, Cache& C)
{
    C.e_chi2.assign((size_t)P.nobs, 0.); C.m_chi2.assign((size_t)P.nme, 0.); C.e_level.assign((size_t)P.nobs, 0); C.m_level.assign((size_t)P.nme, 0);
}

} // namespace

// f's Tcw, x3Dw, Twm are in / out as in the library.  chi2_checks: 2 x (nobs + 4 nmobs) doubles, the cached chi2 of every edge at the two
// checks (monocular edges, then marker edges).  Returns 0, or -4 beyond the pose bound.
extern "C" int ref_lba(const Flat* f, int order, uint8_t* erase, Result* res, double* chi2_checks)
{
    std::memset(res, 0, sizeof(*res));
    Prob P;
    Est X;
    if (!setup(P, X, *f, order)) return -4;
    Cache C;
    cache_clear(P, C);
    const int nobs = f->nobs;
    std::vector<double> xv((size_t)6 * MAXV, 0.), xl((size_t)3 * std::max(P.np, 1), 0.);
    const int ne = nobs + 4 * f->nmobs;
    bool stale;
    res->n_edges_mono = nobs;
    res->n_edges_marker = P.nme;
    res->iterations[0] = optimize(P, C, X, true, 5, xv, xl, stale);
    res->stale_mask |= stale ? 1 : 0;
    auto depth = [&](int e) {
        double Xc[3];
        map(X.pose[(size_t)P.okf[e]], &X.pt[(size_t)P.e_pt[(size_t)e] * 3], Xc);
        return Xc[2];
    };
    for (int e = 0; e < nobs; e++) {
        if (chi2_checks) chi2_checks[e] = C.e_chi2[(size_t)e];
        if (!(C.e_chi2[(size_t)e] <= 5.991) || !(depth(e) > 0.0)) {
            C.e_level[(size_t)e] = 1;
            res->n_level1[0]++;
        }
    }
    for (int j = 0; j < P.nme; j++) {
        if (chi2_checks) chi2_checks[nobs + j] = C.m_chi2[(size_t)j];
        if (!(C.m_chi2[(size_t)j] <= 5.991)) {
            C.m_level[(size_t)j] = 1;
            res->n_level1[1]++;
        }
    }
    res->iterations[1] = optimize(P, C, X, false, 10, xv, xl, stale);
    res->stale_mask |= stale ? 2 : 0;
    for (int e = 0; e < nobs; e++) {
        if (chi2_checks) chi2_checks[ne + e] = C.e_chi2[(size_t)e];
        erase[e] = !(C.e_chi2[(size_t)e] <= 5.991) || !(depth(e) > 0.0);
        res->n_erase += erase[e];
    }
    for (int j = 0; j < P.nme && chi2_checks; j++) chi2_checks[ne + nobs + j] = C.m_chi2[(size_t)j];
    for (int k = 0; k < f->nkf; k++)
        if (!f->kf_fixed[k]) to_float(X.pose[(size_t)k], f->Tcw + 12 * k);
    for (int m = 0; f->use_markers && m < f->nma; m++) to_float(X.pose[(size_t)(f->nkf + m)], f->Twm + 12 * m);
    for (int i = 0; i < 3 * f->np; i++) f->x3Dw[i] = (float)X.pt[(size_t)i];
    return 0;
}

// One linearisation (all edges, Huber) and the first trial, as orbfe_lba_inspect.  full_H (may be NULL): the whole system with lambda0
// on its diagonal, (6 nv + 3 np)^2 row-major, poses first; b holds its right-hand side.
extern "C" int ref_lba_inspect(const Flat* f, int order, int32_t* nv, double* b, double* Hpp, double* Hll, double* chi2, double* x, double* full_H)
{
    Prob P;
    Est X, Xt;
    if (!setup(P, X, *f, order)) return -4;
    Cache C;
    cache_clear(P, C);
    LbaLin L;
    linearize(P, X, true, C, L);
    const double lambda = 1e-5 * L.maxdiag;
    inspect_out(P, L, lambda, nv, b, Hpp, Hll, chi2, full_H);
    std::vector<double> xv((size_t)6 * MAXV, 0.), xl((size_t)3 * std::max(P.np, 1), 0.);
    double tempChi, sp;
    trial(P, C, L, lambda, true, X, Xt, xv, xl, tempChi, sp);
    inspect_update(P, xv, xl, x);
    return 0;
}

// The anchor to tests/pose_opt_ref.cpp: the points are held, so the problem is the motion-only one -- one optimize(maxit) with Huber
// over the same edges, from the same poses, without the markers.  f's Tcw is in / out; returns the LM iterations run.
extern "C" int ref_lba_poses_only(const Flat* f, int maxit, int order)
{
    Flat q = *f;
    q.nma = q.nmobs = q.use_markers = 0;
    Prob P;
    Est X;
    P.fix_points = true;
    if (!setup(P, X, q, order)) return -4;
    Cache C;
    cache_clear(P, C);
    std::vector<double> xv((size_t)6 * MAXV, 0.), xl((size_t)3 * std::max(P.np, 1), 0.);
    bool stale;
    const int it = optimize(P, C, X, true, maxit, xv, xl, stale);
    for (int k = 0; k < q.nkf; k++)
        if (!q.kf_fixed[k]) to_float(X.pose[(size_t)k], q.Tcw + 12 * k);
    return it;
}
