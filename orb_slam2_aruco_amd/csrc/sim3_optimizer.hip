// sim3_optimizer.hip -- the 7-DoF refinement of loop closing (Optimizer::OptimizeSim3, src/Optimizer.cc:1544-1739) on gfx950.
//
// One workgroup of 256 threads per problem, one launch per call (k_sim3_opt), whatever the number of problems, iterations and trials.
//   - prep: the kept correspondences (match12[i] = i2 >= 0, both map points valid) are compacted in index order (ballot prefix, as
//     k_sim3_prep does) and staged in LDS, 53 B each: P1c and P2c = Rkw x + tkw in the CV_32F convention of sim3_points.hpp, the two
//     observations, the two information weights, the index in keyframe 1 and a "removed" flag;
//   - a linearisation pass: lanes 0..13 compute the 14 perturbed estimates Sim3(+-1e-9 e_d) * S and their inverses once, into LDS;
//     every lane then evaluates its correspondences (slots tid, tid + 256, ...), e12 then e21 -- error, Huber weight, g2o's
//     central-difference Jacobian (14 map-and-project evaluations an edge) -- and sums the robust chi2, the 28 entries of H's upper
//     triangle and b in registers; the 36 sums go through a fixed-order butterfly inside each wave and the four wave results are
//     added in wave order by thread 0.  The order depends only on the problem, never on the batch it sits in;
//   - thread 0 does the 7 x 7 LDLT (diagonal pivoting), Sim3(update) * S and the lambda logic: the dense step is lm_dense.hpp's,
//     shared with pose_optimizer.hip, the scalar rules are lm_rules.hpp's, shared with local_ba.hip too;
//   - a trial pass per LM trial sums the robust chi2 at the trial estimate, in the same order.
// The perturbed estimates are functions of the vertex alone: g2o recomputes them for every edge and gets these bits.
// The edges' "cached" errors are not stored: they are the errors at the last estimate the active edges were evaluated at (Sev),
// recomputed bit for bit when the classification reads them.  After a round that ended on rejected trials Sev is the rejected
// trial's estimate, as the reference's stale errors are.
//
// Defined where the reference is undefined: an edge whose error or numeric Jacobian is not finite (a projected point with z = 0)
// adds nothing to chi2, H and b in that pass, and a pair with a chi2 that is not finite is classified bad (the reference's
// NaN > th2 is false); no kept correspondence: no iteration runs (iterations[0] = -1), the early return.
#include "host_stage.hpp"
#include "lm_dense.hpp"
#include "orbfe_common.hpp"
#include "ransac_sets.hpp"   // clampn
#include "sim3_group.hpp"
#include "sim3_points.hpp"
#include <cfloat>
#include <cmath>

namespace orbfe {
namespace {

constexpr int SO_MAX_LEVELS = 32;
constexpr int SO_NSUM = lm_nsum<7>;   // 36: robust chi2, H upper triangle (28), b (7)
constexpr int SO_SIM_FLOATS = 13;   // s12, R12 row-major, t12

// EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError with S or its inverse: obs - cam_map(project(S.map(P)))
__device__ __forceinline__ void edge_error(const Sim3& S, const double (&P)[3], double ox, double oy, const Cam& K, double (&err)[2])
{
    double X[3];
    map(S, P, X);
    project_error(X, ox, oy, K, err);
}

// BaseBinaryEdge::linearizeOplus for the Sim3 vertex (the point vertex is fixed): central differences over the perturbed
// estimates sp[2 d] (+delta) and sp[2 d + 1] (-delta).  Returns whether every entry is finite.
__device__ __forceinline__ bool edge_jacobian(const Sim3* sp, const double (&P)[3], double ox, double oy, const Cam& K, double (&J)[2][7])
{
    const double scalar = 1.0 / (2 * 1e-9);
    bool ok = true;
#pragma unroll
    for (int d = 0; d < 7; d++) {
        double ep[2], em[2];
        edge_error(sp[2 * d], P, ox, oy, K, ep);
        edge_error(sp[2 * d + 1], P, ox, oy, K, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
        ok = ok && isfinite(J[0][d]) && isfinite(J[1][d]);
    }
    return ok;
}

// ------------------------------------------------------------------------------------------ the kernel --
struct SimOptArgs {
    // per-frame blocks of `capacity` (x3Dw: x 3; Tcw: 12 floats a frame)
    const orbfe_keypoint* kps;
    const int32_t* nk;
    const float* x3Dw;
    const uint8_t* valid;          // may be NULL: every feature has a good map point
    const float* Tcw;
    const int32_t *pair1, *pair2;  // frames of problem p; NULL: p and p + 1
    const int32_t* m12;            // problem p at m12 + p * capacity
    int32_t* m12_out;              // may be m12
    const unsigned char* sim;      // problem p's s12, R12, t12 (13 floats) at sim + p * sim_stride
    size_t sim_stride;
    orbfe_sim3_opt_result* res;
    int capacity, nlevels, fix_scale;
    float th2;
    double delta;                  // (double)sqrtf(th2), as deltaHuber reaches RobustKernelHuber::setDelta
    float K1[4], K2[4];            // fx, fy, cx, cy
    float inv_sigma2[SO_MAX_LEVELS];
};

// thread 0's state and the prep phase's counters, in LDS
struct SoCtl {
    Sim3 S, S0, Sev, Ssave;
    double H[7][7], b[7], x[7];
    LmState lm;
    int ok2, cont, stop, nact, base, bad;
    int cnt[LM_WAVES];
    float Tcw[24];
};
static_assert(sizeof(SoCtl) == 944, "SO_FIXED and the capacity limit behind it hang on this size");

struct SoLds {
    SoCtl* c;
    double* red;
    Sim3 *sp, *spi;      // the 14 perturbed estimates and their inverses
    float4 *p1, *p2;     // P1c / P2c; .w = the information of the edge observed in that keyframe (p1.w: e12's, p2.w: e21's)
    float4* ob;          // obs1.x, obs1.y, obs2.x, obs2.y
    int32_t* idx;        // index in keyframe 1
    uint8_t* st;         // 1: the pair was removed
};

constexpr size_t SO_FIXED = al16(sizeof(SoCtl)) + al16(sizeof(double) * LM_WAVES * SO_NSUM) + 2 * 14 * sizeof(Sim3);

size_t lds_bytes(int capacity)
{
    const size_t cap = (size_t)capacity;
    return SO_FIXED + 3 * al16(cap * 16) + al16(cap * 4) + al16(cap);
}

// so_optimize, so_classify and sim3_exp are kept out of line on purpose.  With everything inlined the kernel is one 22 000-line
// function at the limit of the register file (256 VGPR + 120 AGPR, 153 SGPR spills), and that build gave wrong reduction results on
// the MI355X: thread 0 read slots of `red` that held an earlier pass's sums.  The cause was not found in its
// assembly; the out-of-line build passes every test.  Do not force these inline without rerunning them.
// The same symptom came back, here and in k_pose_opt, when the unpacking of the linearisation's sums into H and b was moved into a
// forceinline template of lm_dense.hpp (same operations, same barriers, same register and scratch figures for this kernel): stale
// slots of `red` in the counts and sums that followed.  With the unpacking written in the kernels, as below, both give the bits they
// always gave.  So that loop stays in each kernel, and any change to thread 0's code behind block_sum wants the GPU tests rerun.
//
// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg over the pairs that are not removed.  Returns the
// iterations run (-1 without an active edge); c.ok2 == 3 afterwards: the last trial was rejected.  Called by the whole workgroup.
__device__ __noinline__ int so_optimize(const SoLds& L, const SimOptArgs& a, int N, int iterations)
{
    SoCtl& c = *L.c;
    const int tid = threadIdx.x;
    const Cam K1{a.K1[0], a.K1[1], a.K1[2], a.K1[3]}, K2{a.K2[0], a.K2[1], a.K2[2], a.K2[3]};
    int cnt = 0;
    for (int i = tid; i < N; i += LM_THREADS) cnt += L.st[i] == 0;
    cnt = block_count(cnt, L.red);
    if (tid == 0) {
        c.nact = cnt;
        lm_round_start(c.lm);
        c.ok2 = 0;
        for (int j = 0; j < 7; j++) c.x[j] = 0;
    }
    __syncthreads();
    if (c.nact == 0) return -1;
    int it = 0;
    while (it < iterations) {
        // the perturbed estimates of this linearisation: oplusImpl(+-delta e_d), the scale component zeroed when it is fixed
        if (tid < 14) {
            double u[7] = {0, 0, 0, 0, 0, 0, 0};
            const int d = tid >> 1;
#pragma unroll
            for (int j = 0; j < 7; j++)
                if (j == d) u[j] = (tid & 1) ? -1e-9 : 1e-9;
            if (a.fix_scale) u[6] = 0;
            const Sim3 Sp = mul(sim3_exp(u), c.S);
            L.sp[tid] = Sp;
            L.spi[tid] = inverse(Sp);
        }
        __syncthreads();
        // linearisation pass at S: robust chi2, H, b
        {
            const Sim3 S = c.S, Si = inverse(S);
            double s[SO_NSUM];
#pragma unroll
            for (int k = 0; k < SO_NSUM; k++) s[k] = 0;
            for (int i = tid; i < N; i += LM_THREADS) {
                if (L.st[i]) continue;
                const float4 a1 = L.p1[i], a2 = L.p2[i], o = L.ob[i];
                const double P1[3] = {a1.x, a1.y, a1.z}, P2[3] = {a2.x, a2.y, a2.z};
                double err[2], J[2][7], rho[2];
                // e12: keyframe 2's point seen in keyframe 1
                edge_error(S, P2, o.x, o.y, K1, err);
                if (edge_jacobian(L.sp, P2, o.x, o.y, K1, J) && isfinite(err[0]) && isfinite(err[1])) {
                    huber(chi2_of(err, a1.w), a.delta, rho);
                    s[0] += rho[0];
                    add_edge(err, J, a1.w, rho[1], s);
                }
                // e21: keyframe 1's point seen in keyframe 2
                edge_error(Si, P1, o.z, o.w, K2, err);
                if (edge_jacobian(L.spi, P1, o.z, o.w, K2, J) && isfinite(err[0]) && isfinite(err[1])) {
                    huber(chi2_of(err, a2.w), a.delta, rho);
                    s[0] += rho[0];
                    add_edge(err, J, a2.w, rho[1], s);
                }
            }
            block_sum<SO_NSUM>(s, L.red);
            if (tid == 0) {
                c.Sev = c.S;
                int k = 1;
                for (int r = 0; r < 7; r++)
                    for (int cc = r; cc < 7; cc++, k++) c.H[r][cc] = c.H[cc][r] = s[k];
                for (int r = 0; r < 7; r++) c.b[r] = s[29 + r];
                double md = 0;
                if (it == 0)
                    for (int j = 0; j < 7; j++) md = fmax(fabs(c.H[j][j]), md);
                lm_linearised(c.lm, s[0], it == 0, md);
            }
        }
        // trials
        for (;;) {
            if (tid == 0) {
                c.Ssave = c.S;
                double x[7];
                c.ok2 = damped_solve(c.H, c.b, c.lm.lambda, c.x, x) ? 1 : 0;
                if (a.fix_scale) x[6] = 0;   // oplusImpl zeroes it in the solver's own vector
                for (int j = 0; j < 7; j++) c.x[j] = x[j];
                c.S = mul(sim3_exp(x), c.S);
            }
            __syncthreads();
            const Sim3 S = c.S, Si = inverse(S);
            double s[1] = {0};
            for (int i = tid; i < N; i += LM_THREADS) {
                if (L.st[i]) continue;
                const float4 a1 = L.p1[i], a2 = L.p2[i], o = L.ob[i];
                const double P1[3] = {a1.x, a1.y, a1.z}, P2[3] = {a2.x, a2.y, a2.z};
                double err[2], rho[2];
                edge_error(S, P2, o.x, o.y, K1, err);
                if (isfinite(err[0]) && isfinite(err[1])) {
                    huber(chi2_of(err, a1.w), a.delta, rho);
                    s[0] += rho[0];
                }
                edge_error(Si, P1, o.z, o.w, K2, err);
                if (isfinite(err[0]) && isfinite(err[1])) {
                    huber(chi2_of(err, a2.w), a.delta, rho);
                    s[0] += rho[0];
                }
            }
            block_sum<1>(s, L.red);
            if (tid == 0) {
                c.Sev = c.S;
                if (lm_judge_trial(c.lm, s[0], c.ok2 != 0, gain_scale(c.x, c.b, c.lm.lambda))) {
                    c.ok2 = 2;   // accepted
                } else {
                    c.S = c.Ssave;
                    c.ok2 = 3;   // rejected
                }
                c.cont = lm_try_again(c.lm);
            }
            __syncthreads();
            if (!c.cont) break;
        }
        it++;
        if (tid == 0) c.stop = lm_iteration_end(c.lm);
        __syncthreads();
        if (c.stop) break;
    }
    return it;
}

// the check after a round: a pair is bad when either cached chi2 exceeds (double)th2; bad pairs are removed.  The count is valid
// in thread 0.
__device__ __noinline__ int so_classify(const SoLds& L, const SimOptArgs& a, int N)
{
    const Cam K1{a.K1[0], a.K1[1], a.K1[2], a.K1[3]}, K2{a.K2[0], a.K2[1], a.K2[2], a.K2[3]};
    const Sim3 S = L.c->Sev, Si = inverse(S);
    const double th2 = (double)a.th2;
    int nb = 0;
    for (int i = threadIdx.x; i < N; i += LM_THREADS) {
        if (L.st[i]) continue;
        const float4 a1 = L.p1[i], a2 = L.p2[i], o = L.ob[i];
        const double P1[3] = {a1.x, a1.y, a1.z}, P2[3] = {a2.x, a2.y, a2.z};
        double e12[2], e21[2];
        edge_error(S, P2, o.x, o.y, K1, e12);
        edge_error(Si, P1, o.z, o.w, K2, e21);
        if (!(chi2_of(e12, a1.w) <= th2) || !(chi2_of(e21, a2.w) <= th2)) {
            L.st[i] = 1;
            nb++;
        }
    }
    return block_count(nb, L.red);
}

__global__ __launch_bounds__(LM_THREADS) void k_sim3_opt(SimOptArgs a)
{
    extern __shared__ __align__(16) unsigned char so_smem[];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cap = a.capacity;
    SoLds L;
    L.c = (SoCtl*)so_smem;
    L.red = (double*)(so_smem + al16(sizeof(SoCtl)));
    L.sp = (Sim3*)(so_smem + al16(sizeof(SoCtl)) + al16(sizeof(double) * LM_WAVES * SO_NSUM));
    L.spi = L.sp + 14;
    unsigned char* q = so_smem + SO_FIXED;
    L.p1 = (float4*)q;
    q += al16((size_t)cap * 16);
    L.p2 = (float4*)q;
    q += al16((size_t)cap * 16);
    L.ob = (float4*)q;
    q += al16((size_t)cap * 16);
    L.idx = (int32_t*)q;
    q += al16((size_t)cap * 4);
    L.st = q;
    SoCtl& c = *L.c;

    const int f1 = a.pair1 ? a.pair1[p] : p, f2 = a.pair2 ? a.pair2[p] : p + 1;
    const int n1 = clampn(a.nk[f1], cap), n2 = clampn(a.nk[f2], cap);
    const orbfe_keypoint* k1 = a.kps + (size_t)f1 * cap;
    const orbfe_keypoint* k2 = a.kps + (size_t)f2 * cap;
    const float* x1 = a.x3Dw + (size_t)f1 * cap * 3;
    const float* x2 = a.x3Dw + (size_t)f2 * cap * 3;
    const uint8_t* v1 = a.valid ? a.valid + (size_t)f1 * cap : nullptr;
    const uint8_t* v2 = a.valid ? a.valid + (size_t)f2 * cap : nullptr;
    const int32_t* m12 = a.m12 + (size_t)p * cap;
    int32_t* m12_out = a.m12_out + (size_t)p * cap;

    // prep: the kept correspondences, compacted in index order
    if (tid < 12) c.Tcw[tid] = a.Tcw[(size_t)f1 * 12 + tid];
    else if (tid < 24) c.Tcw[tid] = a.Tcw[(size_t)f2 * 12 + tid - 12];
    if (tid == 0) { c.base = 0; c.bad = 0; }
    __syncthreads();
    for (int base = 0; base < n1; base += LM_THREADS) {
        const int i1 = base + tid;
        int i2 = -1;
        bool keep = false;
        if (i1 < n1) {
            i2 = m12[i1];      // an index outside frame 2 counts as "no match"
            keep = i2 >= 0 && i2 < n2 && (!v1 || (v1[i1] != 0 && v2[i2] != 0));
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) c.cnt[wv] = __popcll(bal);
        __syncthreads();
        if (keep) {
            int idx = c.base + __popcll(bal & ((1ull << lane) - 1ull));
            for (int w = 0; w < wv; w++) idx += c.cnt[w];
            const orbfe_keypoint kp1 = k1[i1], kp2 = k2[i2];
            const bool bad = kp1.octave < 0 || kp1.octave >= a.nlevels || kp2.octave < 0 || kp2.octave >= a.nlevels;
            if (bad) c.bad = 1;
            float X[3];
            rigid(c.Tcw, x1[3 * i1], x1[3 * i1 + 1], x1[3 * i1 + 2], X);
            L.p1[idx] = make_float4(X[0], X[1], X[2], bad ? 0.f : a.inv_sigma2[kp1.octave]);   // .w: e12's information (obs1's level)
            rigid(c.Tcw + 12, x2[3 * i2], x2[3 * i2 + 1], x2[3 * i2 + 2], X);
            L.p2[idx] = make_float4(X[0], X[1], X[2], bad ? 0.f : a.inv_sigma2[kp2.octave]);   // .w: e21's information (obs2's level)
            L.ob[idx] = make_float4(kp1.x, kp1.y, kp2.x, kp2.y);
            L.idx[idx] = i1;
            L.st[idx] = 0;
        }
        __syncthreads();
        if (tid == 0) c.base += c.cnt[0] + c.cnt[1] + c.cnt[2] + c.cnt[3];
        __syncthreads();
    }
    const int N = c.base;
    if (c.bad) {
        // an octave outside [0, nlevels): the problem is skipped
        if (tid == 0) {
            orbfe_sim3_opt_result r{};
            r.status = ORBFE_ERR_INVALID;
            a.res[p] = r;
        }
        return;
    }
    if (tid == 0) {
        // g2o::Sim3(R, t, s) of the floats: Quaterniond(R), not normalised
        const float* sf = (const float*)(a.sim + (size_t)p * a.sim_stride);
        double R[3][3];
        for (int r = 0; r < 3; r++)
            for (int cc = 0; cc < 3; cc++) R[r][cc] = sf[1 + 3 * r + cc];
        Sim3 S;
        S.q = quat_from_matrix(R);
        for (int k = 0; k < 3; k++) S.t[k] = sf[10 + k];
        S.s = sf[0];
        c.S = c.S0 = c.Sev = S;
    }
    __syncthreads();

    // optimize(5), the first check
    int iters[2] = {0, 0}, stale = 0, more = 0, nbad2 = 0;
    iters[0] = so_optimize(L, a, N, 5);
    stale |= c.ok2 == 3 ? 1 : 0;
    __syncthreads();
    const int nb1 = so_classify(L, a, N);
    if (tid == 0) c.nact = N - nb1;
    __syncthreads();
    const int left = c.nact;
    const int nbad = N - left;
    const bool early = left < 10;
    if (!early) {
        // optimize again only with inliers, from the first round's estimate
        more = nbad > 0 ? 10 : 5;
        iters[1] = so_optimize(L, a, N, more);
        stale |= c.ok2 == 3 ? 2 : 0;
        __syncthreads();
        nbad2 = so_classify(L, a, N);   // valid in thread 0
    }
    __syncthreads();
    // the matches: a copy, then -1 where the pair was removed
    if (m12_out != m12)
        for (int i = tid; i < n1; i += LM_THREADS) m12_out[i] = m12[i];
    __syncthreads();
    for (int i = tid; i < N; i += LM_THREADS)
        if (L.st[i]) m12_out[L.idx[i]] = -1;
    if (tid == 0) {
        orbfe_sim3_opt_result r{};
        const Sim3& S = early ? c.S0 : c.S;   // the early return does not write the estimate back
        r.n_inliers = early ? 0 : left - nbad2;
        r.n_correspondences = N;
        r.n_bad = nbad;
        r.more_iterations = more;
        r.iterations[0] = iters[0];
        r.iterations[1] = iters[1];
        r.stale_mask = stale;
        r.status = ORBFE_OK;
        r.s12 = S.s;
        r.q12[0] = S.q.x; r.q12[1] = S.q.y; r.q12[2] = S.q.z; r.q12[3] = S.q.w;
        for (int k = 0; k < 3; k++) r.t12[k] = S.t[k];
        a.res[p] = r;
    }
}

// ------------------------------------------------------------------------------------------- host --
thread_local ThreadWorkspaces<HostStage> tl_stages;

int fill_args(SimOptArgs& a, const float* K4_1, const float* K4_2, const float* inv_sigma2, int nlevels, float th2, int fix_scale,
              const char* name)
{
    if (!K4_1 || !K4_2 || !inv_sigma2) return fail(ORBFE_ERR_INVALID, "%s: NULL K4 or inv_level_sigma2", name);
    if (nlevels <= 0 || nlevels > SO_MAX_LEVELS) return fail(ORBFE_ERR_INVALID, "%s: nlevels = %d is not in 1 .. %d", name, nlevels, SO_MAX_LEVELS);
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(K4_1[i]) || !std::isfinite(K4_2[i])) return fail(ORBFE_ERR_INVALID, "%s: K is not finite", name);
    for (int i = 0; i < nlevels; i++)
        if (!std::isfinite(inv_sigma2[i])) return fail(ORBFE_ERR_INVALID, "%s: inv_level_sigma2 is not finite", name);
    if (!(th2 > 0) || !std::isfinite(th2)) return fail(ORBFE_ERR_INVALID, "%s: th2 is not a positive finite number", name);
    for (int i = 0; i < 4; i++) { a.K1[i] = K4_1[i]; a.K2[i] = K4_2[i]; }
    for (int l = 0; l < SO_MAX_LEVELS; l++) a.inv_sigma2[l] = l < nlevels ? inv_sigma2[l] : 0.f;
    a.nlevels = nlevels;
    a.th2 = th2;
    a.delta = (double)sqrtf(th2);
    a.fix_scale = fix_scale != 0;
    return ORBFE_OK;
}

int launch(const SimOptArgs& a, int npairs, hipStream_t s, const char* name)
{
    const size_t lds = lds_bytes(a.capacity);
    if (lds > (size_t)max_lds())
        return fail(ORBFE_ERR_CAPACITY, "%s: capacity %d needs %zu B of LDS (at most %d)", name, a.capacity, lds, max_lds());
    int rc = ensure_dyn_lds((const void*)k_sim3_opt, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sim3_opt, dim3(npairs), dim3(LM_THREADS), lds, s, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

bool all_finite(const float* v, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

} // namespace
} // namespace orbfe

using namespace orbfe;

extern "C" int orbfe_optimize_sim3(const orbfe_keypoint* kps1, int n1, const float* x3Dw1, const uint8_t* valid1, const float* Tcw1,
                                   const float* K4_1, const orbfe_keypoint* kps2, int n2, const float* x3Dw2, const uint8_t* valid2,
                                   const float* Tcw2, const float* K4_2, const int32_t* match12, const float* inv_level_sigma2, int nlevels,
                                   float s12, const float* R12, const float* t12, float th2, int fix_scale, int32_t* match12_out,
                                   orbfe_sim3_opt_result* res, int device)
{
    static const char* name = "orbfe_optimize_sim3";
    if (n1 < 0 || n2 < 0 || !res || !Tcw1 || !Tcw2 || !R12 || !t12 || (n1 && (!kps1 || !match12 || !match12_out || !x3Dw1)) ||
        (n2 && (!kps2 || !x3Dw2)) || ((valid1 == nullptr) != (valid2 == nullptr)))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument (NULL pointer or negative size)", name);
    SimOptArgs a{};
    int rc = fill_args(a, K4_1, K4_2, inv_level_sigma2, nlevels, th2, fix_scale, name);
    if (rc) return rc;
    if (!std::isfinite(s12) || !all_finite(R12, 9) || !all_finite(t12, 3) || !all_finite(Tcw1, 12) || !all_finite(Tcw2, 12))
        return fail(ORBFE_ERR_INVALID, "%s: the similarity or a keyframe pose is not finite", name);
    for (int i = 0; i < n1; i++) {
        const int j = match12[i];
        if (j >= n2 || j < -1) return fail(ORBFE_ERR_INVALID, "%s: match12[%d] = %d is not in [-1, n2)", name, i, j);
        if (j < 0 || (valid1 && (!valid1[i] || !valid2[j]))) continue;
        const int o1 = kps1[i].octave, o2 = kps2[j].octave;
        if (o1 < 0 || o1 >= nlevels || o2 < 0 || o2 >= nlevels)
            return fail(ORBFE_ERR_INVALID, "%s: correspondence %d -> %d has an octave outside [0, %d)", name, i, j, nlevels);
        if (!all_finite(x3Dw1 + 3 * (size_t)i, 3) || !all_finite(x3Dw2 + 3 * (size_t)j, 3) || !std::isfinite(kps1[i].x) ||
            !std::isfinite(kps1[i].y) || !std::isfinite(kps2[j].x) || !std::isfinite(kps2[j].y))
            return fail(ORBFE_ERR_INVALID, "%s: correspondence %d -> %d has a point or an observation that is not finite", name, i, j);
    }
    a.capacity = std::max(std::max(n1, n2), 1);
    if ((rc = use_device(device))) return rc;
    HostStage& w = tl_stages.get();
    const size_t cap = (size_t)a.capacity, kb = sizeof(orbfe_keypoint);
    // device io: [kps 2 cap | n | x3Dw 2 cap x 3 | valid 2 cap | Tcw 24 | m12 cap | s12 R12 t12] [res | m12_out cap]
    IoLayout l;
    const size_t i_kps = l.take(2 * cap * kb), i_n = l.take(8), i_x = l.take(2 * cap * 12), i_v = l.take(2 * cap);
    const size_t i_T = l.take(96), i_m = l.take(cap * 4), i_s = l.take(SO_SIM_FLOATS * 4);
    l.outputs();
    const size_t o_res = l.take(sizeof(orbfe_sim3_opt_result)), o_m = l.take(cap * 4);
    if ((rc = w.begin(l))) return rc;
    const int32_t nn[2] = {n1, n2};
    w.put(i_kps, kps1, (size_t)n1 * kb);
    w.put(i_kps + cap * kb, kps2, (size_t)n2 * kb);
    w.put(i_n, nn, 8);
    w.put(i_x, x3Dw1, (size_t)n1 * 12);
    w.put(i_x + cap * 12, x3Dw2, (size_t)n2 * 12);
    if (valid1) {
        w.put(i_v, valid1, (size_t)n1);
        w.put(i_v + cap, valid2, (size_t)n2);
    }
    w.put(i_T, Tcw1, 48);
    w.put(i_T + 48, Tcw2, 48);
    w.put(i_m, match12, (size_t)n1 * 4);
    float sim[SO_SIM_FLOATS];
    sim[0] = s12;
    for (int k = 0; k < 9; k++) sim[1 + k] = R12[k];
    for (int k = 0; k < 3; k++) sim[10 + k] = t12[k];
    w.put(i_s, sim, sizeof(sim));
    if ((rc = w.upload())) return rc;
    a.kps = w.dev<const orbfe_keypoint>(i_kps); a.nk = w.dev<const int32_t>(i_n); a.x3Dw = w.dev<const float>(i_x);
    a.valid = valid1 ? w.dev<const uint8_t>(i_v) : nullptr;
    a.Tcw = w.dev<const float>(i_T); a.m12 = w.dev<const int32_t>(i_m); a.m12_out = w.dev<int32_t>(o_m);
    a.sim = w.dev<const unsigned char>(i_s); a.sim_stride = 0;
    a.res = w.dev<orbfe_sim3_opt_result>(o_res);
    if ((rc = launch(a, 1, w.stream, name)) || (rc = w.download()) || (rc = w.sync())) return rc;
    *res = *w.host<const orbfe_sim3_opt_result>(o_res);
    w.get(match12_out, o_m, (size_t)n1 * 4);
    return ORBFE_OK;
}

extern "C" int orbfe_optimize_sim3_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, const float* d_x3Dw,
                                                const uint8_t* d_valid, const float* d_Tcw, const int32_t* d_pair1, const int32_t* d_pair2,
                                                int npairs, const int32_t* d_match12, const float* K4, const float* inv_level_sigma2,
                                                int nlevels, const void* d_sim12, size_t sim12_stride, float th2, int fix_scale,
                                                int32_t* d_match12_out, orbfe_sim3_opt_result* d_res, void* stream)
{
    static const char* name = "orbfe_optimize_sim3_batch_device";
    if (!d_kps || !d_n || !d_x3Dw || !d_Tcw || !d_match12 || !d_match12_out || !d_sim12 || !d_res || capacity <= 0 || npairs <= 0 ||
        ((d_pair1 == nullptr) != (d_pair2 == nullptr)))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    if (sim12_stride < SO_SIM_FLOATS * sizeof(float) || sim12_stride % sizeof(float) || (uintptr_t)d_sim12 % sizeof(float))
        return fail(ORBFE_ERR_INVALID, "%s: the similarities need a stride of at least 52 bytes, stride and base multiples of 4", name);
    SimOptArgs a{};
    int rc = fill_args(a, K4, K4, inv_level_sigma2, nlevels, th2, fix_scale, name);
    if (rc) return rc;
    a.kps = d_kps; a.nk = d_n; a.x3Dw = d_x3Dw; a.valid = d_valid; a.Tcw = d_Tcw; a.pair1 = d_pair1; a.pair2 = d_pair2;
    a.m12 = d_match12; a.m12_out = d_match12_out;
    a.sim = (const unsigned char*)d_sim12; a.sim_stride = sim12_stride;
    a.res = d_res;
    a.capacity = capacity;
    return launch(a, npairs, (hipStream_t)stream, name);
}
