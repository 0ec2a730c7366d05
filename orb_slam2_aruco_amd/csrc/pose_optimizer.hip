// pose_optimizer.hip -- motion-only pose optimization (Optimizer::PoseOptimizationByAruco / PoseOptimization, src/Optimizer.cc) on
// gfx950.
//
// One workgroup of 256 threads per problem, one launch per batch (k_pose_opt), whatever the iteration and trial counts.  The
// observations are staged in LDS (25 B each: observation, world point, information, flags; 160 B a marker).  The whole solve runs
// in that workgroup, in double as g2o does: 4 rounds x up to 10 Levenberg-Marquardt iterations x up to 10 trials.
//   - a linearisation pass: every lane evaluates its edges (slots tid, tid + 256, ...: the monocular edges by keypoint index, then
//     the marker corners) -- error, Huber weight, Jacobian (analytic for mono edges, g2o's central differences for marker edges) --
//     and sums the robust chi2, the 21 entries of H's upper triangle and b in registers; the 28 sums go through a fixed-order
//     butterfly inside each wave and the four wave results are added in wave order by thread 0.  The order depends only on the
//     problem, never on the batch it sits in;
//   - thread 0 then does the 6 x 6 LDLT (diagonal pivoting), the exponential map and the lambda logic: the dense step is
//     lm_dense.hpp's, shared with sim3_optimizer.hip, the scalar rules are lm_rules.hpp's, shared with local_ba.hip too;
//   - a trial pass per LM trial sums the robust chi2 at the trial pose, in the same order.
// The edges' "cached" errors of g2o are not stored: they are the errors at the last pose the active edges were evaluated at (Tev),
// recomputed bit for bit when the classification reads them.  After a round that ended on rejected trials Tev is the rejected
// trial's pose, as the reference's stale errors are.
#include "ba_camera.hpp"
#include "host_stage.hpp"
#include "lm_dense.hpp"
#include "orbfe_common.hpp"
#include "se3_quat.hpp"
#include <cfloat>
#include <cmath>

namespace orbfe {
namespace {

constexpr int PO_NSUM = lm_nsum<6>;   // 28: robust chi2, H upper triangle (21), b (6)

// ------------------------------------------------------------------------------------------- edges --
// EdgeSE3ProjectXYZOnlyPose::linearizeOplus at the camera point Xc = T Xw
__device__ __forceinline__ void mono_jacobian(const double (&Xc)[3], const Cam& K, double (&J)[2][6])
{
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

// EdgeMarker::computeError: obs - pi((T Twm) p)
__device__ __forceinline__ void marker_error(const SE3& T, const SE3& Twm, const double (&p)[3], double ox, double oy, const Cam& K,
                                             double (&err)[2])
{
    const SE3 Tcm = mul(T, Twm);
    double Xc[3];
    map(Tcm, p, Xc);
    project_error(Xc, ox, oy, K, err);
}

// BaseBinaryEdge::linearizeOplus for the camera vertex: central differences through exp(+-1e-9 e_d) * T
__device__ void marker_jacobian(const SE3& T, const SE3& Twm, const double (&p)[3], double ox, double oy, const Cam& K, double (&J)[2][6])
{
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    for (int d = 0; d < 6; d++) {
        double u[6] = {0, 0, 0, 0, 0, 0}, ep[2], em[2];
        u[d] = delta;
        marker_error(mul(se3_exp(u), T), Twm, p, ox, oy, K, ep);
        u[d] = -delta;
        marker_error(mul(se3_exp(u), T), Twm, p, ox, oy, K, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
}

// ------------------------------------------------------------------------------------------ the kernel --
struct PoseArgs {
    const orbfe_keypoint* kps;
    const int32_t* n;
    const uint8_t* has_mp;
    const float* x3Dw;
    const orbfe_pose_marker* markers;
    const int32_t* nm;
    const float* Tin;
    float* Tout;
    uint8_t* outlier;
    float* chi2;
    orbfe_pose_result* res;
    int capacity, mcapacity, nlevels;
    float fx, fy, cx, cy, marker_info;
    double delta;                       // (double)(float)sqrt(5.991), as deltaMono reaches RobustKernelHuber::setDelta
    float inv_sigma2[BA_MAX_LEVELS];
};

// thread 0's state, in LDS
struct Ctl {
    SE3 T, T0, Tev, Tsave;
    double H[6][6], b[6], x[6];
    LmState lm;
    int ok2, cont, stop, nin, pad[2];
};
static_assert(sizeof(Ctl) == 712, "PO_FIXED and the capacity limits behind it hang on this size");

constexpr size_t PO_FIXED = al16(sizeof(Ctl)) + al16(sizeof(double) * LM_WAVES * PO_NSUM);

size_t lds_bytes(int capacity, int mcapacity)
{
    const size_t cap = (size_t)capacity, mc = (size_t)mcapacity;
    return PO_FIXED + al16(cap * 8) + al16(cap * 16) + al16(cap) + al16(mc * sizeof(SE3)) + al16(mc * 4 * 8) + al16(mc * 4 * 16);
}

__global__ __launch_bounds__(LM_THREADS) void k_pose_opt(PoseArgs a)
{
    extern __shared__ __align__(16) unsigned char po_smem[];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int cap = a.capacity, mcap = a.mcapacity;
    Ctl& c = *(Ctl*)po_smem;
    double* red = (double*)(po_smem + al16(sizeof(Ctl)));
    unsigned char* p = po_smem + PO_FIXED;
    float2* s_obs = (float2*)p;
    p += al16((size_t)cap * 8);
    float4* s_xw = (float4*)p;   // X, Y, Z, information
    p += al16((size_t)cap * 16);
    uint8_t* s_st = p;           // bit 0: has a map point, bit 1: outlier (level 1)
    p += al16((size_t)cap);
    SE3* s_twm = (SE3*)p;
    p += al16((size_t)mcap * sizeof(SE3));
    float2* s_cobs = (float2*)p;
    p += al16((size_t)mcap * 4 * 8);
    float4* s_cpt = (float4*)p;

    const int n = min(max(a.n[f], 0), cap);
    const int nm = a.nm ? min(max(a.nm[f], 0), mcap) : 0;
    const size_t base = (size_t)f * cap;
    const Cam K{a.fx, a.fy, a.cx, a.cy};

    // stage the problem
    int cnt = 0, badoct = 0;
    for (int i = tid; i < n; i += LM_THREADS) {
        const orbfe_keypoint kp = a.kps[base + i];
        const bool h = a.has_mp[base + i] != 0;
        const bool okoct = kp.octave >= 0 && kp.octave < a.nlevels;
        cnt += h;
        badoct += h && !okoct;
        s_obs[i] = make_float2(kp.x, kp.y);
        const float* X = a.x3Dw + (base + i) * 3;
        s_xw[i] = h ? make_float4(X[0], X[1], X[2], okoct ? a.inv_sigma2[kp.octave] : 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        s_st[i] = h ? 1 : 0;
    }
    for (int j = tid; j < 4 * nm; j += LM_THREADS) {
        const orbfe_pose_marker& mk = a.markers[(size_t)f * mcap + j / 4];
        const int k = j & 3;
        s_cobs[j] = make_float2(mk.corners[2 * k], mk.corners[2 * k + 1]);
        s_cpt[j] = make_float4(mk.local[3 * k], mk.local[3 * k + 1], mk.local[3 * k + 2], 0.f);
    }
    for (int m = tid; m < nm; m += LM_THREADS) s_twm[m] = se3_from_float(a.markers[(size_t)f * mcap + m].Twm);
    const int n_initial = block_count(cnt, red);
    const int nbadoct = block_count(badoct, red + LM_WAVES);
    if (tid == 0) {
        c.nin = n_initial;
        c.stop = nbadoct;
    }
    __syncthreads();
    const int n0 = c.nin;
    if (c.stop) {
        // an octave outside [0, nlevels): the problem is skipped
        if (tid == 0) {
            orbfe_pose_result r{};
            r.status = ORBFE_ERR_INVALID;
            a.res[f] = r;
        }
        if (tid < 12) a.Tout[(size_t)f * 12 + tid] = a.Tin[(size_t)f * 12 + tid];
        return;
    }
    if (n0 < 3) {
        for (int i = tid; i < n; i += LM_THREADS)
            if (s_st[i]) a.outlier[base + i] = 0;
        if (tid == 0) {
            orbfe_pose_result r{};
            r.n_initial = n0;
            a.res[f] = r;
        }
        if (tid < 12) a.Tout[(size_t)f * 12 + tid] = a.Tin[(size_t)f * 12 + tid];
        return;
    }
    if (tid == 0) c.T0 = se3_from_float(a.Tin + (size_t)f * 12);
    const int nedges = n0 + 4 * nm;
    int n_bad[4] = {0, 0, 0, 0}, iters[4] = {0, 0, 0, 0}, stale = 0, rounds = 0;
    __syncthreads();

    for (int round = 0; round < 4; round++) {
        const bool mono_kernel = round < 3;
        if (tid == 0) {
            c.T = c.T0;
            lm_round_start(c.lm);
            for (int j = 0; j < 6; j++) c.x[j] = 0;
        }
        __syncthreads();
        int round_iters = -1;
        bool round_stale = false;
        if (c.nin + 4 * nm > 0) {
            for (int it = 0; it < 10;) {
                // linearisation pass at T: robust chi2, H, b
                {
                    const SE3 T = c.T;
                    double s[PO_NSUM];
                    for (int k = 0; k < PO_NSUM; k++) s[k] = 0;
                    for (int i = tid; i < n; i += LM_THREADS) {
                        if (s_st[i] != 1) continue;
                        const float2 o = s_obs[i];
                        const float4 xw = s_xw[i];
                        const double Xw[3] = {xw.x, xw.y, xw.z};
                        double Xc[3], err[2], J[2][6], rho[2] = {0, 1};
                        map(T, Xw, Xc);
                        project_error(Xc, o.x, o.y, K, err);
                        mono_jacobian(Xc, K, J);
                        const double ch = chi2_of(err, xw.w);
                        if (mono_kernel) {
                            huber(ch, a.delta, rho);
                            s[0] += rho[0];
                        } else {
                            s[0] += ch;
                        }
                        add_edge(err, J, xw.w, rho[1], s);
                    }
                    for (int j = tid; j < 4 * nm; j += LM_THREADS) {
                        const float2 o = s_cobs[j];
                        const float4 pt = s_cpt[j];
                        const double pm[3] = {pt.x, pt.y, pt.z};
                        const SE3 Twm = s_twm[j >> 2];
                        double err[2], J[2][6], rho[2];
                        marker_error(T, Twm, pm, o.x, o.y, K, err);
                        marker_jacobian(T, Twm, pm, o.x, o.y, K, J);
                        huber(chi2_of(err, (double)a.marker_info), a.delta, rho);
                        s[0] += rho[0];
                        add_edge(err, J, (double)a.marker_info, rho[1], s);
                    }
                    block_sum<PO_NSUM>(s, red);
                    if (tid == 0) {
                        c.Tev = c.T;
                        // the sums as H and b, here and not in a function of lm_dense.hpp: see the note above so_optimize (sim3_optimizer.hip)
                        int k = 1;
                        for (int r = 0; r < 6; r++)
                            for (int cc = r; cc < 6; cc++, k++) c.H[r][cc] = c.H[cc][r] = s[k];
                        for (int r = 0; r < 6; r++) c.b[r] = s[22 + r];
                        double md = 0;
                        if (it == 0)
                            for (int j = 0; j < 6; j++) md = fmax(fabs(c.H[j][j]), md);
                        lm_linearised(c.lm, s[0], it == 0, md);
                    }
                }
                // trials
                for (;;) {
                    if (tid == 0) {
                        c.Tsave = c.T;
                        double x[6];
                        c.ok2 = damped_solve(c.H, c.b, c.lm.lambda, c.x, x) ? 1 : 0;
                        for (int j = 0; j < 6; j++) c.x[j] = x[j];
                        c.T = mul(se3_exp(x), c.T);
                    }
                    __syncthreads();
                    const SE3 T = c.T;
                    double s[1] = {0};
                    for (int i = tid; i < n; i += LM_THREADS) {
                        if (s_st[i] != 1) continue;
                        const float2 o = s_obs[i];
                        const float4 xw = s_xw[i];
                        const double Xw[3] = {xw.x, xw.y, xw.z};
                        double Xc[3], err[2], rho[2];
                        map(T, Xw, Xc);
                        project_error(Xc, o.x, o.y, K, err);
                        const double ch = chi2_of(err, xw.w);
                        if (mono_kernel) {
                            huber(ch, a.delta, rho);
                            s[0] += rho[0];
                        } else {
                            s[0] += ch;
                        }
                    }
                    for (int j = tid; j < 4 * nm; j += LM_THREADS) {
                        const float2 o = s_cobs[j];
                        const float4 pt = s_cpt[j];
                        const double pm[3] = {pt.x, pt.y, pt.z};
                        double err[2], rho[2];
                        marker_error(T, s_twm[j >> 2], pm, o.x, o.y, K, err);
                        huber(chi2_of(err, (double)a.marker_info), a.delta, rho);
                        s[0] += rho[0];
                    }
                    block_sum<1>(s, red);
                    if (tid == 0) {
                        c.Tev = c.T;
                        if (lm_judge_trial(c.lm, s[0], c.ok2 != 0, gain_scale(c.x, c.b, c.lm.lambda))) {
                            c.ok2 = 2;   // accepted
                        } else {
                            c.T = c.Tsave;
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
                round_iters = it;
                round_stale = c.ok2 == 3;
                if (c.stop) break;
            }
        }
        // classification: the inliers read the errors at Tev, the outliers compute theirs at T
        {
            const SE3 T = c.T, Tev = c.Tev;
            int nb = 0;
            for (int i = tid; i < n; i += LM_THREADS) {
                const uint8_t st = s_st[i];
                if (!(st & 1)) continue;
                const float2 o = s_obs[i];
                const float4 xw = s_xw[i];
                const double Xw[3] = {xw.x, xw.y, xw.z};
                double Xc[3], err[2];
                map((st & 2) ? T : Tev, Xw, Xc);
                project_error(Xc, o.x, o.y, K, err);
                const double ch = chi2_of(err, xw.w);
                const bool out = (float)ch > 5.991f;
                nb += out;
                s_st[i] = out ? 3 : 1;
                if (a.chi2) a.chi2[base + i] = (float)ch;
            }
            nb = block_count(nb, red);
            if (tid == 0) c.nin = n0 - nb;
            n_bad[round] = nb;   // valid in thread 0
        }
        iters[round] = round_iters;
        stale |= round_stale ? 1 << round : 0;
        rounds = round + 1;
        __syncthreads();
        if (nedges < 10) break;
    }
    for (int i = tid; i < n; i += LM_THREADS)
        if (s_st[i] & 1) a.outlier[base + i] = (s_st[i] & 2) ? 1 : 0;
    if (tid == 0) {
        orbfe_pose_result r{};
        r.n_initial = n0;
        r.n_marker_edges = 4 * nm;
        r.rounds = rounds;
        for (int k = 0; k < 4; k++) {
            r.n_bad[k] = k < rounds ? n_bad[k] : 0;
            r.iterations[k] = k < rounds ? iters[k] : 0;
        }
        r.n_good = n0 - n_bad[rounds - 1];
        r.stale_mask = stale;
        r.status = ORBFE_OK;
        a.res[f] = r;
        float Tf[12];
        to_float(c.T, Tf);
        for (int k = 0; k < 12; k++) a.Tout[(size_t)f * 12 + k] = Tf[k];
    }
}

// has_mp / x3Dw from mode 2's match_cur and the queries' world points
__global__ void k_pose_gather(const int32_t* match_cur, const int32_t* nk, int capacity, const float* q_x3Dw, const int32_t* nq,
                              int qcapacity, uint8_t* has_mp, float* x3Dw)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= capacity) return;
    const size_t o = (size_t)f * capacity + i;
    const int n = nk[f], nqf = min(nq[f], qcapacity);
    const int m = i < n ? match_cur[o] : -1;
    const bool h = m >= 0 && m < nqf;
    has_mp[o] = h ? 1 : 0;
    const float* X = q_x3Dw + ((size_t)f * qcapacity + (h ? m : 0)) * 3;
    x3Dw[o * 3 + 0] = h ? X[0] : 0.f;
    x3Dw[o * 3 + 1] = h ? X[1] : 0.f;
    x3Dw[o * 3 + 2] = h ? X[2] : 0.f;
}

// ------------------------------------------------------------------------------------------- host --
int fill_args(PoseArgs& a, const float* inv_sigma2, int nlevels, const float* K4, float marker_info, const char* name)
{
    BaCamera c;
    const BaCheck chk = ba_camera(c, K4, inv_sigma2, nlevels, marker_info, name);
    if (chk.err) return fail(chk.err, "%s", chk.msg);
    a.nlevels = c.nlevels;
    for (int l = 0; l < BA_MAX_LEVELS; l++) a.inv_sigma2[l] = c.inv_sigma2[l];
    a.fx = c.fx; a.fy = c.fy; a.cx = c.cx; a.cy = c.cy;
    a.marker_info = c.marker_info;
    a.delta = c.delta;
    return ORBFE_OK;
}

int launch(const PoseArgs& a, int nframes, hipStream_t s, const char* name)
{
    const size_t lds = lds_bytes(a.capacity, a.mcapacity);
    if (lds > (size_t)max_lds())
        return fail(ORBFE_ERR_CAPACITY, "%s: capacity %d / mcapacity %d need %zu B of LDS (at most %d)", name, a.capacity, a.mcapacity, lds, max_lds());
    int rc = ensure_dyn_lds((const void*)k_pose_opt, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pose_opt, dim3(nframes), dim3(LM_THREADS), lds, s, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

thread_local ThreadWorkspaces<HostStage> tl_stages;

} // namespace
} // namespace orbfe

using namespace orbfe;

extern "C" int orbfe_pose_optimization(const orbfe_keypoint* kps, int n, const uint8_t* has_mp, const float* x3Dw,
                                       const float* inv_level_sigma2, int nlevels, const float* K4, const orbfe_pose_marker* markers, int nm,
                                       float marker_info, const float* Tcw_in, float* Tcw_out, uint8_t* outlier, float* chi2,
                                       orbfe_pose_result* res, int device)
{
    static const char* name = "orbfe_pose_optimization";
    if (n < 0 || nm < 0 || !Tcw_in || !Tcw_out || !res || (n && (!kps || !has_mp || !x3Dw || !outlier)) || (nm && !markers))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    PoseArgs a{};
    int rc = fill_args(a, inv_level_sigma2, nlevels, K4, marker_info, name);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (has_mp[i] && (kps[i].octave < 0 || kps[i].octave >= nlevels))
            return fail(ORBFE_ERR_INVALID, "%s: keypoint %d has octave %d, outside [0, %d)", name, i, kps[i].octave, nlevels);
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(Tcw_in[i])) return fail(ORBFE_ERR_INVALID, "%s: Tcw_in is not finite", name);
    if ((rc = use_device(device))) return rc;
    HostStage& w = tl_stages.get();
    const size_t cap = (size_t)std::max(n, 1), mc = (size_t)std::max(nm, 1);
    // device io: [kps | has | x3Dw | markers | n, nm | Tin] [Tout | res | outlier | chi2]
    IoLayout l;
    const size_t i_kps = l.take(cap * sizeof(orbfe_keypoint)), i_has = l.take(cap), i_x = l.take(cap * 12);
    const size_t i_mk = l.take(mc * sizeof(orbfe_pose_marker)), i_n = l.take(8), i_T = l.take(48);
    l.outputs();
    const size_t o_T = l.take(48), o_res = l.take(sizeof(orbfe_pose_result)), o_out = l.take(cap), o_chi = l.take(cap * 4);
    if ((rc = w.begin(l))) return rc;
    const int32_t nn[2] = {n, nm};
    w.put(i_kps, kps, (size_t)n * sizeof(orbfe_keypoint));
    w.put(i_has, has_mp, (size_t)n);
    w.put(i_x, x3Dw, (size_t)n * 12);
    w.put(i_mk, markers, (size_t)nm * sizeof(orbfe_pose_marker));
    w.put(i_n, nn, 8);
    w.put(i_T, Tcw_in, 48);
    if ((rc = w.upload())) return rc;
    a.kps = w.dev<const orbfe_keypoint>(i_kps); a.has_mp = w.dev<const uint8_t>(i_has); a.x3Dw = w.dev<const float>(i_x);
    a.markers = w.dev<const orbfe_pose_marker>(i_mk);
    a.n = w.dev<const int32_t>(i_n); a.nm = a.n + 1; a.Tin = w.dev<const float>(i_T);
    a.Tout = w.dev<float>(o_T); a.res = w.dev<orbfe_pose_result>(o_res); a.outlier = w.dev<uint8_t>(o_out); a.chi2 = w.dev<float>(o_chi);
    a.capacity = (int)cap; a.mcapacity = (int)mc;
    if ((rc = launch(a, 1, w.stream, name)) || (rc = w.download()) || (rc = w.sync())) return rc;
    memcpy(Tcw_out, w.host<float>(o_T), 48);
    *res = *w.host<const orbfe_pose_result>(o_res);
    // only the entries with a map point were written
    const uint8_t* ho = w.host<const uint8_t>(o_out);
    const float* hc = w.host<const float>(o_chi);
    const bool classified = res->rounds > 0;
    for (int i = 0; i < n; i++)
        if (has_mp[i]) {
            outlier[i] = ho[i];
            if (chi2 && classified) chi2[i] = hc[i];
        }
    return ORBFE_OK;
}

extern "C" int orbfe_pose_optimization_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, int nframes,
                                                    const uint8_t* d_has_mp, const float* d_x3Dw, const orbfe_pose_marker* d_markers,
                                                    const int32_t* d_nm, int mcapacity, const float* inv_level_sigma2, int nlevels,
                                                    const float* K4, float marker_info, const float* d_Tcw_in, float* d_Tcw_out,
                                                    uint8_t* d_outlier, float* d_chi2, orbfe_pose_result* d_res, void* stream)
{
    static const char* name = "orbfe_pose_optimization_batch_device";
    if (!d_kps || !d_n || !d_has_mp || !d_x3Dw || !d_Tcw_in || !d_Tcw_out || !d_outlier || !d_res || capacity <= 0 || nframes <= 0 ||
        mcapacity < 0 || (mcapacity > 0 && (!d_markers || !d_nm)))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    PoseArgs a{};
    int rc = fill_args(a, inv_level_sigma2, nlevels, K4, marker_info, name);
    if (rc) return rc;
    a.kps = d_kps; a.n = d_n; a.has_mp = d_has_mp; a.x3Dw = d_x3Dw;
    a.markers = mcapacity > 0 ? d_markers : nullptr;
    a.nm = mcapacity > 0 ? d_nm : nullptr;
    a.Tin = d_Tcw_in; a.Tout = d_Tcw_out; a.outlier = d_outlier; a.chi2 = d_chi2; a.res = d_res;
    a.capacity = capacity;
    a.mcapacity = mcapacity;
    return launch(a, nframes, (hipStream_t)stream, name);
}

extern "C" int orbfe_pose_gather_device(const int32_t* d_match_cur, const int32_t* d_n, int capacity, int nframes, const float* d_q_x3Dw,
                                        const int32_t* d_nq, int qcapacity, uint8_t* d_has_mp, float* d_x3Dw, void* stream)
{
    if (!d_match_cur || !d_n || !d_q_x3Dw || !d_nq || !d_has_mp || !d_x3Dw || capacity <= 0 || nframes <= 0 || qcapacity <= 0 || nframes > 65535)
        return fail(ORBFE_ERR_INVALID, "orbfe_pose_gather_device: invalid argument");
    hipLaunchKernelGGL(k_pose_gather, dim3((capacity + 255) / 256, nframes), dim3(256), 0, (hipStream_t)stream, d_match_cur, d_n, capacity,
                       d_q_x3Dw, d_nq, qcapacity, d_has_mp, d_x3Dw);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
