// local_ba.hip -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:772-1242) behind its collect step, on gfx950: g2o's
// Levenberg-Marquardt with BlockSolver_6_3 (pose blocks 6 x 6, point blocks 3 x 3 marginalised by a Schur complement), two rounds
// (5 iterations with Huber, 10 on the edges the first check left at level 0), with the fork's marker poses as free SE3 vertices.
//
// One problem fills the chip, so the solve is a chain of small grid-wide kernels and the LM state lives on the device (LbaCtl, two
// copies of every estimate: `cur` and the trial's).  The host enqueues the same launches whatever the problem; a launch whose step
// is already decided (the round is over, the trial loop has ended, the call was refused) returns at once.
//   setup          k_lba_setup: estimates in double, the edge arrays (either observation form), the (keyframe, point) -> edge table,
//                  validation; k_lba_begin: the free-vertex numbering, bounds, the stop flag, the LM state of the round
//   an iteration   k_lba_linearize (a thread per point, then a thread per marker corner edge: errors, chi2 cache, Jacobians, the
//                  edge's blocks, Hll and bl of the point in observation order), k_lba_pose_blocks (a workgroup per free vertex:
//                  Hpp, bp over the vertex's edges in point order), k_lba_ctl_lin (chi2, lambda0)
//   a trial        k_lba_schur_points ((Hll + lambda I)^-1), k_lba_assemble (a wave per block (i, j) of S: Hpp - sum W_i D^-1 W_j^T
//                  over the points both see, in point order), k_lba_solve (one workgroup: L L^T of S in LDS, or in global memory when it does not fit, the two
//                  substitutions, the trial poses), k_lba_backsub (a thread per point: the point's update, the trial point, the
//                  trial errors and chi2), k_lba_ctl_trial (rho, accept or reject, lambda / nu, the stop rules: lm_rules.hpp's,
//                  the ones pose_optimizer.hip and sim3_optimizer.hip run)
//   a check        k_lba_check (a thread per edge: level 1 flags after round 1, the erase bytes after round 2)
//   the end        k_lba_finish (poses, points, marker poses as floats; the record)
// Sums: a thread adds its own items in their order (a point's observations; a contiguous run of points), a wave adds its lanes by a
// fixed butterfly, the waves are added in order, and the per-workgroup partial sums of a grid-wide pass are added the same way by one
// workgroup.  No floating-point atomic anywhere: the order of every sum is a function of the problem's sizes alone.
// g2o's cached edge errors are the chi2 cache e_chi2 / m_chi2: written by every pass that evaluates an edge (the linearisation and
// each trial, rejected ones included), read by the checks -- so a round that ends on a rejected trial leaves that trial's errors
// there, and an edge at level 1 keeps its value of round 1, as in the reference.
// What the entry points decide before they launch -- the validation, the scratch layout, the staging block, the launch schedule --
// is host arithmetic in lba_plan.hpp (the camera and level-table step, shared with pose_optimizer.hip, in ba_camera.hpp).
#include "ba_edges.hpp"
#include "host_stage.hpp"
#include "lba_plan.hpp"
#include "lm_dense.hpp"
#include "orbfe_common.hpp"
#include "se3_quat.hpp"
#include <cfloat>
#include <cmath>

namespace orbfe {
namespace {

constexpr int LBA_BAD_INVALID = 1, LBA_BAD_CAPACITY = 2;
static_assert(sizeof(SE3) == LBA_SE3_BYTES, "lba_plan.hpp lays the pose arrays out for this size");

struct LbaP {
    // the caller's arrays
    float* Tcw; const uint8_t* kf_fixed; float* x3Dw; const int32_t* obs_offset; const int32_t* obs_kf; const float* obs_xy;
    const int32_t* obs_oct; const int32_t* obs_feat; const orbfe_keypoint* kps;
    float* Twm; const float* mlocal; const int32_t* mobs_offset; const int32_t* mobs_kf; const float* mobs_corners;
    const uint8_t* stop; uint8_t* erase; orbfe_lba_result* res;
    int nkf, np, nobs, nma, nmobs, nme, capacity, nlevels, use_markers, npb, nb, pad;
    Cam K;
    double delta, marker_info;
    float inv_sigma2[LBA_MAX_LEVELS];
    // scratch: lba_scratch of lba_plan.hpp gives every pointer its array
    LbaCtl* ctl;
    SE3* pose[2];          // nkf keyframes, then nma markers
    double* pt[2];         // np x 3
    int32_t *e_kf, *e_pt; float *e_ox, *e_oy, *e_info; uint8_t *e_level, *e_use; double *e_chi2, *e_blk;
    int32_t* mo_marker; uint8_t *m_level, *m_use; double *m_chi2, *m_blk;
    double *Hll, *bl, *Dinv, *xl; uint8_t* p_active;
    double *Hpp, *bp, *xv, *vmax; int32_t *v_active, *v_kf, *kf_free;
    int32_t* tbl;          // nkf x np: the edge of (keyframe, point), -1 none
    double *S, *bs, *chi_part, *scale_part, *max_part;
};

// the edges, their blocks, the wave sums and the steps of the passes that global_ba.hip has too are ba_edges.hpp's

// ---------------------------------------------------------------------------------------- setup --
__global__ __launch_bounds__(256) void k_lba_setup(LbaP p)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (i < p.nkf + p.nma) {
        const bool mk = i >= p.nkf;
        const float* T = mk ? p.Twm + (size_t)(i - p.nkf) * 12 : p.Tcw + (size_t)i * 12;
        bool fin = true;
        for (int k = 0; k < 12; k++) fin = fin && finite_f(T[k]);
        if (mk)
            for (int k = 0; k < 12; k++) fin = fin && finite_f(p.mlocal[(size_t)(i - p.nkf) * 12 + k]);
        if (!fin) bad |= LBA_BAD_INVALID;
        const SE3 S = se3_from_float(T);
        p.pose[0][i] = S;
        p.pose[1][i] = S;
    }
    if (i < p.np) {
        const int lo = p.obs_offset[i], hi = p.obs_offset[i + 1];
        if ((i == 0 && lo != 0) || hi < lo || lo < 0 || hi > p.nobs || (i == p.np - 1 && hi != p.nobs)) bad |= LBA_BAD_INVALID;
        else if (hi - lo > ORBFE_LBA_MAX_OBSERVATIONS) bad |= LBA_BAD_CAPACITY;
        for (int k = 0; k < 3; k++) {
            const float v = p.x3Dw[(size_t)i * 3 + k];
            if (!finite_f(v)) bad |= LBA_BAD_INVALID;
            p.pt[0][(size_t)i * 3 + k] = v;
            p.pt[1][(size_t)i * 3 + k] = v;
        }
    }
    if (i < p.nobs) {
        const int pt = obs_point(p.obs_offset, p.np, i);
        int kf = p.obs_kf[i];
        ObsPixel o;
        if (kf < 0 || kf >= p.nkf) {
            o.ok = false;
            kf = 0;
        } else {
            o = obs_pixel(i, kf, p.obs_xy, p.obs_oct, p.obs_feat, p.kps, p.capacity, p.nlevels);
        }
        if (!o.ok) bad |= LBA_BAD_INVALID;
        p.e_kf[i] = kf; p.e_pt[i] = pt; p.e_ox[i] = o.x; p.e_oy[i] = o.y; p.e_info[i] = p.inv_sigma2[o.oct];
        if (atomicCAS(&p.tbl[(size_t)kf * p.np + pt], -1, i) != -1) bad |= LBA_BAD_INVALID;   // a keyframe observes a point once
    }
    if (i < p.nma) {
        const int lo = p.mobs_offset[i], hi = p.mobs_offset[i + 1];
        if ((i == 0 && lo != 0) || hi < lo || lo < 0 || hi > p.nmobs || (i == p.nma - 1 && hi != p.nmobs)) bad |= LBA_BAD_INVALID;
        else
            for (int o = lo; o < hi; o++) p.mo_marker[o] = i;
    }
    if (i < p.nmobs) {
        const int kf = p.mobs_kf[i];
        if (kf < 0 || kf >= p.nkf) bad |= LBA_BAD_INVALID;
        for (int k = 0; k < 8; k++)
            if (!finite_f(p.mobs_corners[(size_t)i * 8 + k])) bad |= LBA_BAD_INVALID;
    }
    if (bad) atomicOr(&p.ctl->bad, bad);
}

// round 0: the free-vertex numbering, the bounds, the stop flag at the call.  round 1: bDoMore.  One thread.
__global__ void k_lba_begin(LbaP p, int round)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    LbaCtl& c = *p.ctl;
    if (round == 0) {
        int nf = 0;
        for (int k = 0; k < p.nkf; k++) {
            const bool fr = p.kf_fixed[k] == 0;
            p.kf_free[k] = fr ? nf : -1;
            if (fr) {
                if (nf < LBA_MAXV) p.v_kf[nf] = k;
                nf++;
            }
        }
        const int nv = nf + (p.use_markers ? p.nma : 0);
        for (int m = 0; p.use_markers && m < p.nma; m++)
            if (nf + m < LBA_MAXV) p.v_kf[nf + m] = p.nkf + m;
        c.nfree_kf = nf;
        c.nv = nv;
        if (c.bad & LBA_BAD_INVALID) c.abort_status = ORBFE_ERR_INVALID;
        else if ((c.bad & LBA_BAD_CAPACITY) || nv > LBA_MAXV) c.abort_status = ORBFE_ERR_CAPACITY;
        else if (stop_set(p.stop)) c.abort_status = ORBFE_LBA_STOPPED;
        c.aborted = c.abort_status != 0;
        if (c.aborted) c.nv = 0;
        c.iter_go = !c.aborted;
    } else {
        if (c.aborted) return;
        if (stop_set(p.stop)) c.stopped = 1;
        c.iter_go = !c.stopped;
    }
    c.round = round;
    c.it = 0;
    c.trial_go = 0;
    lm_round_start(c.lm);
    c.stale = 0;
}

// ---------------------------------------------------------------------------------------- linearisation --
__global__ __launch_bounds__(LBA_PT) void k_lba_linearize(LbaP p)
{
    const LbaCtl& c = *p.ctl;
    if (c.aborted || !c.iter_go) return;
    const int cur = c.cur;
    const bool robust = c.round == 0;
    double chi = 0, md = 0;
    if ((int)blockIdx.x < p.npb) {
        const int pi = blockIdx.x * LBA_PT + threadIdx.x;
        if (pi < p.np) {
            const double Xw[3] = {p.pt[cur][(size_t)pi * 3], p.pt[cur][(size_t)pi * 3 + 1], p.pt[cur][(size_t)pi * 3 + 2]};
            double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
            int nact = 0;
            for (int e = p.obs_offset[pi]; e < p.obs_offset[pi + 1]; e++) {
                if (p.e_level[e]) {
                    p.e_use[e] = 0;
                    continue;
                }
                nact++;
                const int kf = p.e_kf[e];
                const SE3 T = p.pose[cur][kf];
                const double info = p.e_info[e];
                MonoLin L;
                lba_mono_linearize(T, Xw, p.e_ox[e], p.e_oy[e], p.K, L);
                const double ch = chi2_of(L.err, info);
                p.e_chi2[e] = ch;
                double rho[2] = {ch, 1.};
                if (robust) huber(ch, p.delta, rho);
                chi += rho[0];
                const bool fin = all_finite(L.err, 2) && all_finite(&L.Jp[0][0], 12) && all_finite(&L.Jx[0][0], 6) && isfinite(rho[1]);
                const int vf = p.kf_free[kf];
                p.e_use[e] = fin ? (vf >= 0 ? 3 : 1) : 0;
                if (!fin) continue;
                const double w = rho[1] * info;
                const double r0 = rho[1] * -(info * L.err[0]), r1 = rho[1] * -(info * L.err[1]);
                int k = 0;
                for (int a = 0; a < 3; a++)
                    for (int cc = a; cc < 3; cc++, k++) H[k] += L.Jx[0][a] * (w * L.Jx[0][cc]) + L.Jx[1][a] * (w * L.Jx[1][cc]);
                for (int a = 0; a < 3; a++) b[a] += L.Jx[0][a] * r0 + L.Jx[1][a] * r1;
                if (vf >= 0) {
                    double* out = p.e_blk + (size_t)e * LBA_EBLK;
                    lba_diag_block(L.Jp, w, r0, r1, out);
                    for (int a = 0; a < 6; a++)
                        for (int cc = 0; cc < 3; cc++) out[27 + a * 3 + cc] = L.Jp[0][a] * (w * L.Jx[0][cc]) + L.Jp[1][a] * (w * L.Jx[1][cc]);
                }
            }
            for (int k = 0; k < 6; k++) p.Hll[(size_t)pi * 6 + k] = H[k];
            for (int k = 0; k < 3; k++) p.bl[(size_t)pi * 3 + k] = b[k];
            p.p_active[pi] = nact > 0;
            if (nact > 0) md = fmax(fmax(fabs(H[0]), fabs(H[3])), fabs(H[5]));
        }
    } else {
        const int j = (blockIdx.x - p.npb) * LBA_PT + threadIdx.x;
        if (j < p.nme) {
            if (p.m_level[j]) p.m_use[j] = 0;
            else {
                const int o = j >> 2, k = j & 3, kf = p.mobs_kf[o], m = p.mo_marker[o];
                const SE3 Tc = p.pose[cur][kf], Tm = p.pose[cur][p.nkf + m];
                double ch, rho0;
                p.m_use[j] = marker_edge_linearize(Tc, Tm, marker_corner(p.mlocal, p.mobs_corners, m, o, k), p.K, p.kf_free[kf] >= 0, robust,
                                                   p.marker_info, p.delta, p.m_blk + (size_t)j * LBA_MBLK, ch, rho0);
                p.m_chi2[j] = ch;
                chi += rho0;
            }
        }
    }
    chi = wave_sum(chi);
    md = wave_max(md);
    if (threadIdx.x == 0) {
        p.chi_part[blockIdx.x] = chi;
        p.max_part[blockIdx.x] = md;
    }
}

// Hpp and bp of free vertex v: a keyframe's monocular edges in point order (each thread a contiguous run of points), then its marker
// edges in edge order; a marker's edges in edge order
__global__ __launch_bounds__(LM_THREADS) void k_lba_pose_blocks(LbaP p)
{
    __shared__ double red[LM_WAVES * 28];
    const LbaCtl& c = *p.ctl;
    const int v = blockIdx.x, tid = threadIdx.x;
    if (c.aborted || !c.iter_go || v >= c.nv) return;
    const int kf = p.v_kf[v];
    double s[28];
    for (int k = 0; k < 28; k++) s[k] = 0;
    if (kf < p.nkf)
        run_for(p.np, [&](int pi) {
            const int e = p.tbl[(size_t)kf * p.np + pi];
            if (e < 0 || p.e_level[e]) return;
            s[27] += 1;
            if (p.e_use[e] != 3) return;
            const double* blk = p.e_blk + (size_t)e * LBA_EBLK;
            for (int k = 0; k < 27; k++) s[k] += blk[k];
        });
    block_sum<28>(s, red);
    if (tid != 0) return;
    if (kf < p.nkf) {
        for (int j = 0; j < p.nme; j++) {
            if (p.mobs_kf[j >> 2] != kf || p.m_level[j]) continue;
            s[27] += 1;
            if (!p.m_use[j]) continue;
            const double* blk = p.m_blk + (size_t)j * LBA_MBLK;
            for (int k = 0; k < 27; k++) s[k] += blk[k];
        }
    } else {
        const int m = kf - p.nkf;
        for (int j = 4 * p.mobs_offset[m]; j < 4 * p.mobs_offset[m + 1]; j++) {
            if (p.m_level[j]) continue;
            s[27] += 1;
            if (!p.m_use[j]) continue;
            const double* blk = p.m_blk + (size_t)j * LBA_MBLK + 27;
            for (int k = 0; k < 27; k++) s[k] += blk[k];
        }
    }
    const double md = unpack_pose_sums(s, p.Hpp + (size_t)v * 36, p.bp + v * 6);
    p.v_active[v] = s[27] > 0;
    p.vmax[v] = s[27] > 0 ? md : 0;
}

__global__ __launch_bounds__(LM_THREADS) void k_lba_ctl_lin(LbaP p)
{
    __shared__ double red[LM_WAVES];
    __shared__ double mx[LM_THREADS];
    LbaCtl& c = *p.ctl;
    if (c.aborted || !c.iter_go) return;
    double s[1] = {run_sum(p.chi_part, p.nb)};
    double m = 0;
    for (int i = threadIdx.x; i < p.nb; i += LM_THREADS) m = fmax(m, p.max_part[i]);
    mx[threadIdx.x] = m;
    block_sum<1>(s, red);
    if (threadIdx.x != 0) return;
    double md = 0;
    if (c.it == 0) {
        for (int i = 0; i < LM_THREADS; i++) md = fmax(md, mx[i]);
        for (int v = 0; v < c.nv; v++) md = fmax(md, p.vmax[v]);
    }
    lm_linearised(c.lm, s[0], c.it == 0, md);
    if (c.it == 0) c.lambda0 = c.lm.lambda;
    c.trial_go = 1;
}

// ---------------------------------------------------------------------------------------- a trial --
// (Hll + lambda I)^-1 of every active point
__global__ __launch_bounds__(LBA_PT) void k_lba_schur_points(LbaP p)
{
    const LbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int pi = blockIdx.x * LBA_PT + threadIdx.x;
    if (pi >= p.np || !p.p_active[pi]) return;
    damped_inverse3(p.Hll + (size_t)pi * 6, c.lm.lambda, p.Dinv + (size_t)pi * 9);
}

// block (i, j), i <= j, of S and the rows i of its right-hand side; one wave
__global__ __launch_bounds__(64) void k_lba_assemble(LbaP p)
{
    const LbaCtl& c = *p.ctl;
    const int i = blockIdx.y, j = blockIdx.x, lane = threadIdx.x;
    if (c.aborted || !c.trial_go || i > j || j >= c.nv) return;
    const int ki = p.v_kf[i], kj = p.v_kf[j];
    const bool act = p.v_active[i] && p.v_active[j];
    double acc[36], accb[6];
    for (int k = 0; k < 36; k++) acc[k] = 0;
    for (int k = 0; k < 6; k++) accb[k] = 0;
    if (act && ki < p.nkf && kj < p.nkf) {
        run_for<64>(p.np, [&](int pi) {
            if (!p.p_active[pi]) return;
            const int ei = p.tbl[(size_t)ki * p.np + pi], ej = p.tbl[(size_t)kj * p.np + pi];
            if (ei < 0 || ej < 0 || p.e_level[ei] || p.e_level[ej] || p.e_use[ei] != 3 || p.e_use[ej] != 3) return;
            pair_item_add(p.e_blk + (size_t)ei * LBA_EBLK + 27, p.e_blk + (size_t)ej * LBA_EBLK + 27, p.Dinv + (size_t)pi * 9, p.bl + (size_t)pi * 3, i == j,
                          acc, accb);
        });
        for (int k = 0; k < 36; k++) acc[k] = wave_sum(acc[k]);
        if (i == j)
            for (int k = 0; k < 6; k++) accb[k] = wave_sum(accb[k]);
    }
    if (lane != 0) return;
    double B[36];
    for (int k = 0; k < 36; k++) B[k] = 0;
    if (!act) {
        // a vertex without an active edge is not part of the system: an identity block, a zero right-hand side
        if (i == j)
            for (int a = 0; a < 6; a++) B[a * 6 + a] = 1;
    } else if (i == j) {
        for (int k = 0; k < 36; k++) B[k] = p.Hpp[(size_t)i * 36 + k];
        for (int a = 0; a < 6; a++) B[a * 6 + a] += c.lm.lambda;
        for (int k = 0; k < 36; k++) B[k] -= acc[k];
    } else if (kj < p.nkf) {
        for (int k = 0; k < 36; k++) B[k] = 0. - acc[k];
    } else if (ki < p.nkf) {
        const int m = kj - p.nkf;
        for (int e = 4 * p.mobs_offset[m]; e < 4 * p.mobs_offset[m + 1]; e++) {
            if (p.mobs_kf[e >> 2] != ki || p.m_level[e] || !p.m_use[e]) continue;
            const double* blk = p.m_blk + (size_t)e * LBA_MBLK + 54;
            for (int k = 0; k < 36; k++) B[k] += blk[k];
        }
    }
    for (int a = 0; a < 6; a++)
        for (int bb = 0; bb < 6; bb++) {
            p.S[(size_t)(6 * i + a) * LBA_N + 6 * j + bb] = B[a * 6 + bb];
            p.S[(size_t)(6 * j + bb) * LBA_N + 6 * i + a] = B[a * 6 + bb];
        }
    if (i == j)
        for (int a = 0; a < 6; a++) p.bs[6 * i + a] = act ? p.bp[6 * i + a] - accb[a] : 0.;
}

// S = L L^T in place (lower triangle, right-looking, no pivoting), L y = b, L^T x = y; y holds b on entry and x on return (when the
// factorisation succeeds: the return value).  PACKED: M is the lower triangle row after row (the LDS copy), else rows of LBA_N.
template <bool PACKED> __device__ __forceinline__ bool lba_llt_solve(double* M, int n, double* y, int* fail_s)
{
    const int tid = threadIdx.x;
    auto row = [](int i) { return PACKED ? (size_t)i * (i + 1) / 2 : (size_t)i * LBA_N; };
    for (int k = 0; k < n; k++) {
        if (tid == 0) {
            const double d = M[row(k) + k];
            if (!(d > 0) || !isfinite(d)) *fail_s = 1;
            else M[row(k) + k] = sqrt(d);
        }
        __syncthreads();
        if (*fail_s) return false;
        const double lkk = M[row(k) + k];
        for (int i = k + 1 + tid; i < n; i += LM_THREADS) M[row(i) + k] /= lkk;
        __syncthreads();
        for (int i = k + 1 + (tid >> 4); i < n; i += LM_THREADS / 16) {
            const double lik = M[row(i) + k];
            for (int j = k + 1 + (tid & 15); j <= i; j += 16) M[row(i) + j] -= lik * M[row(j) + k];
        }
        __syncthreads();
    }
    for (int k = 0; k < n; k++) {
        if (tid == 0) y[k] /= M[row(k) + k];
        __syncthreads();
        const double yk = y[k];
        for (int i = k + 1 + tid; i < n; i += LM_THREADS) y[i] -= M[row(i) + k] * yk;
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; k--) {
        if (tid == 0) y[k] /= M[row(k) + k];
        __syncthreads();
        const double yk = y[k];
        for (int i = tid; i < k; i += LM_THREADS) y[i] -= M[row(k) + i] * yk;
        __syncthreads();
    }
    return true;
}

// The reduced solve and the trial poses exp(x_v) T_v.  One workgroup: the factorisation is a chain of 3 n barrier-separated steps, so
// it runs on a copy of the lower triangle in LDS when n <= lds_rows (what the launch reserved), and in global memory otherwise; the
// arithmetic and its order are the same.
__global__ __launch_bounds__(LM_THREADS) void k_lba_solve(LbaP p, int lds_rows)
{
    extern __shared__ __align__(16) double lba_tri[];
    __shared__ double y[LBA_N];
    __shared__ int fail_s;
    LbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int tid = threadIdx.x, n = 6 * c.nv, cur = c.cur;
    if (tid == 0) fail_s = 0;
    for (int i = tid; i < n; i += LM_THREADS) y[i] = p.bs[i];
    bool ok;
    if (n <= lds_rows) {
        for (int i = 0; i < n; i++)
            for (int j = tid; j <= i; j += LM_THREADS) lba_tri[(size_t)i * (i + 1) / 2 + j] = p.S[(size_t)i * LBA_N + j];
        __syncthreads();
        ok = lba_llt_solve<true>(lba_tri, n, y, &fail_s);
    } else {
        __syncthreads();
        ok = lba_llt_solve<false>(p.S, n, y, &fail_s);
    }
    if (ok)
        for (int i = tid; i < n; i += LM_THREADS) p.xv[i] = y[i];
    __syncthreads();
    if (tid == 0) c.ok2 = ok;
    if (tid < c.nv) {
        const int idx = p.v_kf[tid];
        SE3 T = p.pose[cur][idx];
        if (p.v_active[tid]) {
            double u[6];
            for (int a = 0; a < 6; a++) u[a] = p.xv[tid * 6 + a];
            T = mul(se3_exp(u), T);
        }
        p.pose[1 - cur][idx] = T;
    }
}

// the point's update xl = D^-1 (bl - sum W^T x_pose), the trial point, the trial errors of every active edge
__global__ __launch_bounds__(LBA_PT) void k_lba_backsub(LbaP p)
{
    const LbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int cur = c.cur, nxt = 1 - cur;
    const bool robust = c.round == 0;
    double chi = 0, scale = 0;
    if ((int)blockIdx.x < p.npb) {
        const int pi = blockIdx.x * LBA_PT + threadIdx.x;
        if (pi < p.np) {
            double X[3] = {p.pt[cur][(size_t)pi * 3], p.pt[cur][(size_t)pi * 3 + 1], p.pt[cur][(size_t)pi * 3 + 2]};
            if (p.p_active[pi]) {
                const int lo = p.obs_offset[pi], hi = p.obs_offset[pi + 1];
                double* xl = p.xl + (size_t)pi * 3;
                const double* bl = p.bl + (size_t)pi * 3;
                if (c.ok2) {
                    double r[3] = {bl[0], bl[1], bl[2]};
                    for (int e = lo; e < hi; e++) {
                        if (p.e_level[e] || p.e_use[e] != 3) continue;
                        point_rhs_sub(p.e_blk + (size_t)e * LBA_EBLK + 27, p.xv + (size_t)p.kf_free[p.e_kf[e]] * 6, r);
                    }
                    point_solve(p.Dinv + (size_t)pi * 9, r, xl);
                }
                for (int a = 0; a < 3; a++) {
                    scale += xl[a] * (c.lm.lambda * xl[a] + bl[a]);
                    X[a] += xl[a];
                }
                for (int e = lo; e < hi; e++) {
                    if (p.e_level[e]) continue;
                    double err[2], rho[2];
                    lba_mono_error(p.pose[nxt][p.e_kf[e]], X, p.e_ox[e], p.e_oy[e], p.K, err);
                    const double ch = chi2_of(err, (double)p.e_info[e]);
                    p.e_chi2[e] = ch;
                    rho[0] = ch;
                    if (robust) huber(ch, p.delta, rho);
                    chi += rho[0];
                }
            }
            for (int a = 0; a < 3; a++) p.pt[nxt][(size_t)pi * 3 + a] = X[a];
        }
    } else {
        const int j = (blockIdx.x - p.npb) * LBA_PT + threadIdx.x;
        if (j < p.nme && !p.m_level[j]) {
            const int o = j >> 2, k = j & 3, m = p.mo_marker[o];
            const MarkerCorner mc = marker_corner(p.mlocal, p.mobs_corners, m, o, k);
            double err[2], rho[2];
            lba_marker_error(p.pose[nxt][p.mobs_kf[o]], p.pose[nxt][p.nkf + m], mc.pm, mc.ox, mc.oy, p.K, err);
            const double ch = chi2_of(err, p.marker_info);
            p.m_chi2[j] = ch;
            rho[0] = ch;
            if (robust) huber(ch, p.delta, rho);
            chi += rho[0];
        }
    }
    chi = wave_sum(chi);
    scale = wave_sum(scale);
    if (threadIdx.x == 0) {
        p.chi_part[blockIdx.x] = chi;
        p.scale_part[blockIdx.x] = scale;
    }
}

// OptimizationAlgorithmLevenberg::solve behind the trial's chi2: rho, accept or reject, lambda and nu, the end of the iteration
__global__ __launch_bounds__(LM_THREADS) void k_lba_ctl_trial(LbaP p, int maxit)
{
    __shared__ double red[LM_WAVES * 2];
    LbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    double s[2] = {run_sum(p.chi_part, p.nb), run_sum(p.scale_part, p.nb)};
    block_sum<2>(s, red);
    if (threadIdx.x != 0) return;
    double scale = 0;
    for (int j = 0; j < 6 * c.nv; j++) scale += p.xv[j] * (c.lm.lambda * p.xv[j] + (p.v_active[j / 6] ? p.bp[j] : 0.));
    scale += s[1];
    if (lm_judge_trial(c.lm, s[0], c.ok2 != 0, scale)) {
        c.cur = 1 - c.cur;
        c.stale = 0;
    } else {
        c.stale = 1;
    }
    const bool halt = stop_set(p.stop);
    const bool cont = lm_try_again(c.lm) && !halt;
    c.trial_go = cont;
    if (cont) return;
    c.it++;
    c.iters[c.round] = c.it;
    c.stale_mask = (c.stale_mask & ~(1 << c.round)) | (c.stale << c.round);
    const bool stop = lm_iteration_end(c.lm);
    if (halt) c.stopped = 1;
    c.iter_go = !stop && !halt && c.it < maxit;
}

// ---------------------------------------------------------------------------------------- checks and the end --
__global__ __launch_bounds__(256) void k_lba_check(LbaP p, int second)
{
    LbaCtl& c = *p.ctl;
    if (c.aborted || (!second && c.stopped)) return;
    const int i = blockIdx.x * 256 + threadIdx.x, cur = c.cur;
    if (i < p.nobs) {
        const double* X = p.pt[cur] + (size_t)p.e_pt[i] * 3;
        const double Xw[3] = {X[0], X[1], X[2]};
        double Xc[3];
        map(p.pose[cur][p.e_kf[i]], Xw, Xc);
        const bool bad = !(p.e_chi2[i] <= 5.991) || !(Xc[2] > 0.0);
        if (second) {
            p.erase[i] = bad;
            if (bad) atomicAdd(&c.n_erase, 1);
        } else if (bad) {
            p.e_level[i] = 1;
            atomicAdd(&c.n_level1[0], 1);
        }
    } else if (!second && i - p.nobs < p.nme) {
        const int j = i - p.nobs;
        if (!(p.m_chi2[j] <= 5.991)) {
            p.m_level[j] = 1;
            atomicAdd(&c.n_level1[1], 1);
        }
    }
}

__global__ __launch_bounds__(256) void k_lba_finish(LbaP p)
{
    const LbaCtl& c = *p.ctl;
    const int i = blockIdx.x * 256 + threadIdx.x, cur = c.cur;
    if (i == 0) {
        orbfe_lba_result r{};
        r.status = c.abort_status;
        if (!c.aborted) {
            r.n_edges_mono = p.nobs;
            r.n_edges_marker = p.nme;
            r.n_level1[0] = c.n_level1[0]; r.n_level1[1] = c.n_level1[1];
            r.n_erase = c.n_erase;
            r.iterations[0] = c.iters[0]; r.iterations[1] = c.iters[1];
            r.stale_mask = c.stale_mask;
        }
        *p.res = r;
    }
    if (c.aborted) return;
    if (i < p.nkf && p.kf_free[i] >= 0) to_float(p.pose[cur][i], p.Tcw + (size_t)i * 12);
    if (i < p.nma && p.use_markers) to_float(p.pose[cur][p.nkf + i], p.Twm + (size_t)i * 12);
    if (i < p.np)
        for (int k = 0; k < 3; k++) p.x3Dw[(size_t)i * 3 + k] = (float)p.pt[cur][(size_t)i * 3 + k];
}

// ---------------------------------------------------------------------------------------- host --
// the launches of one call, every number from the schedule: inspect = one linearisation and one trial, nothing written to the
// caller's arrays
int lba_enqueue(LbaP& p, void* scratch, hipStream_t s, bool inspect)
{
    const LbaSizes n{p.nkf, p.np, p.nobs, p.nma, p.nmobs};
    const LbaExtent x = lba_scratch(p, n, scratch);
    const LbaSchedule k = lba_schedule(n, p.use_markers != 0, inspect, (size_t)max_lds());
    p.nme = p.use_markers ? 4 * p.nmobs : 0;
    p.npb = k.npb;
    p.nb = k.nb;
    ORBFE_HIP(hipMemsetAsync(scratch, 0, x.zero_end, s));
    ORBFE_HIP(hipMemsetAsync(p.tbl, 0xff, x.tbl_bytes, s));
    int rc = ensure_dyn_lds((const void*)k_lba_solve, k.tri_bytes);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lba_setup, dim3(k.g_setup), dim3(256), 0, s, p);
    for (int round = 0; round < k.rounds; round++) {
        hipLaunchKernelGGL(k_lba_begin, dim3(1), dim3(64), 0, s, p, round);
        if (round == 1) hipLaunchKernelGGL(k_lba_check, dim3(k.g_edges), dim3(256), 0, s, p, 0);
        for (int it = 0; it < k.maxit[round]; it++) {
            hipLaunchKernelGGL(k_lba_linearize, dim3(k.g_pass), dim3(LBA_PT), 0, s, p);
            hipLaunchKernelGGL(k_lba_pose_blocks, dim3(k.vmax), dim3(LM_THREADS), 0, s, p);
            hipLaunchKernelGGL(k_lba_ctl_lin, dim3(1), dim3(LM_THREADS), 0, s, p);
            for (int q = 0; q < k.trials; q++) {
                hipLaunchKernelGGL(k_lba_schur_points, dim3(k.g_points), dim3(LBA_PT), 0, s, p);
                hipLaunchKernelGGL(k_lba_assemble, dim3(k.vmax, k.vmax), dim3(64), 0, s, p);
                hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(LM_THREADS), k.tri_bytes, s, p, k.lds_rows);
                hipLaunchKernelGGL(k_lba_backsub, dim3(k.g_pass), dim3(LBA_PT), 0, s, p);
                if (!inspect) hipLaunchKernelGGL(k_lba_ctl_trial, dim3(1), dim3(LM_THREADS), 0, s, p, k.maxit[round]);
            }
        }
    }
    if (!inspect) {
        hipLaunchKernelGGL(k_lba_check, dim3(k.g_edges), dim3(256), 0, s, p, 1);
        hipLaunchKernelGGL(k_lba_finish, dim3(k.g_setup), dim3(256), 0, s, p);
    }
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

thread_local ThreadWorkspaces<HostStage> tl_lba_stages;

// stage a problem of host arrays as lba_host_io lays it out, send it, and point the kernels' argument at the device copy
int lba_stage(HostStage& w, LbaHostIo& io, LbaP& p, const LbaProblem& pb)
{
    const LbaSizes& n = pb.n;
    io = lba_host_io(n);
    int rc;
    if ((rc = w.begin(io.io))) return rc;
    const int32_t zero2[2] = {0, 0};
    w.put(io.fixed, pb.kf_fixed, (size_t)n.nkf);
    w.put(io.off, n.np ? (const void*)pb.obs_offset : (const void*)zero2, n.np ? (size_t)(n.np + 1) * 4 : 8);
    w.put(io.kf, pb.obs_kf, (size_t)n.nobs * 4); w.put(io.xy, pb.obs_xy, (size_t)n.nobs * 8); w.put(io.oct, pb.obs_octave, (size_t)n.nobs * 4);
    w.put(io.mloc, pb.marker_local, (size_t)n.nma * 48);
    w.put(io.moff, n.nma ? (const void*)pb.mobs_offset : (const void*)zero2, n.nma ? (size_t)(n.nma + 1) * 4 : 8);
    w.put(io.mkf, pb.mobs_kf, (size_t)n.nmobs * 4); w.put(io.mcor, pb.mobs_corners, (size_t)n.nmobs * 32);
    w.put(io.T, pb.Tcw, (size_t)n.nkf * 48); w.put(io.X, pb.x3Dw, (size_t)n.np * 12); w.put(io.M, pb.Twm, (size_t)n.nma * 48);
    if ((rc = w.upload())) return rc;
    // upload() sends [0, split): the in-out arrays lie before the split
    p.kf_fixed = w.dev<const uint8_t>(io.fixed); p.obs_offset = w.dev<const int32_t>(io.off); p.obs_kf = w.dev<const int32_t>(io.kf);
    p.obs_xy = w.dev<const float>(io.xy); p.obs_oct = w.dev<const int32_t>(io.oct); p.obs_feat = nullptr; p.kps = nullptr; p.capacity = 0;
    p.mlocal = w.dev<const float>(io.mloc); p.mobs_offset = w.dev<const int32_t>(io.moff); p.mobs_kf = w.dev<const int32_t>(io.mkf);
    p.mobs_corners = w.dev<const float>(io.mcor);
    p.Tcw = w.dev<float>(io.T); p.x3Dw = w.dev<float>(io.X); p.Twm = w.dev<float>(io.M);
    p.erase = w.dev<uint8_t>(io.erase); p.res = w.dev<orbfe_lba_result>(io.res);
    p.stop = nullptr;
    p.nkf = n.nkf; p.np = n.np; p.nobs = n.nobs; p.nma = n.nma; p.nmobs = n.nmobs;
    return ORBFE_OK;
}

// What both host calls do before they enqueue: the camera and the checks, on the host alone; then, unless the caller's stop flag is
// set already (ORBFE_LBA_STOPPED: no device touched), the device, the stage `w` of this thread with the problem sent, the scratch.
int lba_host_begin(LbaP& p, HostStage*& w, LbaHostIo& io, const LbaProblem& pb, const float* K4, const float* inv_sigma2, int nlevels,
                   float marker_info, int use_markers, const uint8_t* stop, int device, const char* name)
{
    int rc;
    if ((rc = ba_fill(p, K4, inv_sigma2, nlevels, marker_info, use_markers, 5.991, name)) || (rc = report(lba_check_host(pb, nlevels, use_markers, name))))
        return rc;
    if (stop && *stop) return ORBFE_LBA_STOPPED;
    if ((rc = use_device(device))) return rc;
    w = &tl_lba_stages.get();
    if ((rc = lba_stage(*w, io, p, pb))) return rc;
    return w->host_scratch.ensure(lba_scratch_bytes(pb.n));
}

} // namespace
} // namespace orbfe

using namespace orbfe;

extern "C" size_t orbfe_lba_scratch_bytes(int nkf, int np, int nobs, int nma, int nmobs)
{
    const LbaSizes n{nkf, np, nobs, nma, nmobs};
    return lba_sizes_ok(n) ? lba_scratch_bytes(n) : 0;
}

extern "C" int orbfe_local_bundle_adjustment(float* Tcw, const uint8_t* kf_fixed, int nkf, float* x3Dw, int np, const int32_t* obs_offset,
                                             const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                                             const float* inv_level_sigma2, int nlevels, float* Twm, const float* marker_local, int nma,
                                             const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs,
                                             float marker_info, int use_markers, const uint8_t* stop, uint8_t* erase, orbfe_lba_result* res,
                                             int device)
{
    static const char* name = "orbfe_local_bundle_adjustment";
    if (!res || (nobs > 0 && !erase)) return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    const LbaProblem pb{{nkf, np, nobs, nma, nmobs}, Tcw, kf_fixed, x3Dw, obs_offset, obs_kf, obs_xy, obs_octave, nullptr, nullptr, 0,
                        Twm, marker_local, mobs_offset, mobs_kf, mobs_corners};
    LbaP p{};
    HostStage* w = nullptr;
    LbaHostIo io;
    int rc = lba_host_begin(p, w, io, pb, K4, inv_level_sigma2, nlevels, marker_info, use_markers, stop, device, name);
    if (rc == ORBFE_LBA_STOPPED) {
        orbfe_lba_result r{};
        r.status = ORBFE_LBA_STOPPED;
        *res = r;
        return ORBFE_OK;
    }
    if (rc || (rc = lba_enqueue(p, w->host_scratch.p, w->stream, false)) || (rc = w->download()) || (rc = w->sync())) return rc;
    *res = *w->host<const orbfe_lba_result>(io.res);
    if (res->status < 0) return fail(res->status, "%s: the device refused the problem (status %d)", name, res->status);
    w->get(Tcw, io.T, (size_t)nkf * 48);
    w->get(x3Dw, io.X, (size_t)np * 12);
    if (use_markers) w->get(Twm, io.M, (size_t)nma * 48);
    w->get(erase, io.erase, (size_t)nobs);
    return ORBFE_OK;
}

extern "C" int orbfe_local_bundle_adjustment_device(float* d_Tcw, const uint8_t* d_kf_fixed, int nkf, float* d_x3Dw, int np,
                                                    const int32_t* d_obs_offset, const int32_t* d_obs_kf, const float* d_obs_xy,
                                                    const int32_t* d_obs_octave, const int32_t* d_obs_feature, const orbfe_keypoint* d_kps,
                                                    int capacity, int nobs, const float* K4, const float* inv_level_sigma2, int nlevels,
                                                    float* d_Twm, const float* d_marker_local, int nma, const int32_t* d_mobs_offset,
                                                    const int32_t* d_mobs_kf, const float* d_mobs_corners, int nmobs, float marker_info,
                                                    int use_markers, const uint8_t* d_stop, uint8_t* d_erase, orbfe_lba_result* d_res,
                                                    void* d_scratch, size_t scratch_bytes, void* stream)
{
    static const char* name = "orbfe_local_bundle_adjustment_device";
    const LbaProblem d{{nkf, np, nobs, nma, nmobs}, d_Tcw, d_kf_fixed, d_x3Dw, d_obs_offset, d_obs_kf, d_obs_xy, d_obs_octave, d_obs_feature,
                       d_kps, capacity, d_Twm, d_marker_local, d_mobs_offset, d_mobs_kf, d_mobs_corners};
    LbaP p{};
    int rc;
    if ((rc = report(lba_check_device(d, d_erase, d_res, d_scratch, name))) || (rc = report(lba_check_scratch(d.n, scratch_bytes, name))) ||
        (rc = ba_fill(p, K4, inv_level_sigma2, nlevels, marker_info, use_markers, 5.991, name)))
        return rc;
    p.Tcw = d_Tcw; p.kf_fixed = d_kf_fixed; p.x3Dw = d_x3Dw; p.obs_offset = d_obs_offset; p.obs_kf = d_obs_kf; p.obs_xy = d_obs_xy;
    p.obs_oct = d_obs_octave; p.obs_feat = d_obs_feature; p.kps = d_kps; p.capacity = capacity;
    p.Twm = d_Twm; p.mlocal = d_marker_local; p.mobs_offset = d_mobs_offset; p.mobs_kf = d_mobs_kf; p.mobs_corners = d_mobs_corners;
    p.stop = d_stop; p.erase = d_erase; p.res = d_res;
    p.nkf = nkf; p.np = np; p.nobs = nobs; p.nma = nma; p.nmobs = nmobs;
    return lba_enqueue(p, d_scratch, (hipStream_t)stream, false);
}

extern "C" int orbfe_lba_inspect(const float* Tcw, const uint8_t* kf_fixed, int nkf, const float* x3Dw, int np, const int32_t* obs_offset,
                                 const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                                 const float* inv_level_sigma2, int nlevels, const float* Twm, const float* marker_local, int nma,
                                 const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs, float marker_info,
                                 int use_markers, int32_t* nv, double* b, double* Hpp, double* Hll, double* chi2, double* x, int device)
{
    static const char* name = "orbfe_lba_inspect";
    if (!nv || !b || !Hpp || !Hll || !chi2 || !x) return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    // the estimates are read only: an inspect call fetches nothing back into them
    const LbaProblem pb{{nkf, np, nobs, nma, nmobs}, const_cast<float*>(Tcw), kf_fixed, const_cast<float*>(x3Dw), obs_offset, obs_kf, obs_xy,
                        obs_octave, nullptr, nullptr, 0, const_cast<float*>(Twm), marker_local, mobs_offset, mobs_kf, mobs_corners};
    LbaP p{};
    HostStage* w = nullptr;
    LbaHostIo io;
    int rc;
    if ((rc = lba_host_begin(p, w, io, pb, K4, inv_level_sigma2, nlevels, marker_info, use_markers, nullptr, device, name)) ||
        (rc = lba_enqueue(p, w->host_scratch.p, w->stream, true)) || (rc = w->sync()))
        return rc;
    LbaCtl c;
    ORBFE_HIP(hipMemcpy(&c, p.ctl, sizeof(c), hipMemcpyDeviceToHost));
    if (c.abort_status < 0) return fail(c.abort_status, "%s: the device refused the problem (status %d)", name, c.abort_status);
    *nv = c.nv;
    chi2[0] = c.lm.currentChi;
    chi2[1] = c.lambda0;
    if (c.nv) {
        ORBFE_HIP(hipMemcpy(b, p.bp, (size_t)c.nv * 48, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(Hpp, p.Hpp, (size_t)c.nv * 36 * 8, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(x, p.xv, (size_t)c.nv * 48, hipMemcpyDeviceToHost));
    }
    if (np) {
        ORBFE_HIP(hipMemcpy(b + 6 * c.nv, p.bl, (size_t)np * 24, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(Hll, p.Hll, (size_t)np * 48, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(x + 6 * c.nv, p.xl, (size_t)np * 24, hipMemcpyDeviceToHost));
    }
    return ORBFE_OK;
}
