// global_ba.hip -- Optimizer::BundleAdjustment (src/Optimizer.cc:49-307) behind its collect step, on gfx950: the map-wide bundle
// adjustment of the initial map and of loop closing.  One optimize(iterations) of g2o's Levenberg-Marquardt with BlockSolver_6_3 over
// keyframes, map points and the fork's marker poses; Huber on the monocular edges when `robust`, always on the marker edges.
//
// The graph of a call is on the host and fixed, so everything symbolic is host arithmetic (gba_plan.hpp): the edges of every vertex,
// the covisible pairs with their items, the elimination tree of the reduced camera system, the scratch, the schedule.  The LM state
// lives on the device (GbaCtl, two copies of every estimate), the call is a chain of launches whose number depends on the plan and not
// on the values, and a launch whose step is already decided returns at once.  No kernel's work grows with nkf x np.
//   setup          k_gba_setup (estimates in double, the edge arrays in either observation form, validation), k_gba_begin (the call's fate)
//   an iteration   k_gba_linearize (a wave per 64 points, then per 64 marker corner edges: errors, Jacobians, the edge's blocks, Hll
//                  and bl of the point in observation order), k_gba_pose_blocks (a workgroup per free vertex: Hpp, bp over the
//                  vertex's own edge list), k_gba_ctl_lin (chi2, lambda0)
//   a trial        k_gba_schur_points ((Hll + lambda I)^-1 by cofactors), k_gba_reduce (a wave per covisible pair (u, v): its block
//                  Hpp[u == v] + lambda I - sum W_u D^-1 W_v^T over the pair's items, in its own slot of the block-sparse S; bs),
//                  k_gba_front once per level, leaves first, a workgroup per front (front_solve.hpp: the front's blocks of S, the
//                  children's Schur complements left then right, the partial L L^T; a front without a boundary substitutes back at
//                  once), k_gba_back once per level downwards, k_gba_update (the trial poses exp(x_v) T_v), k_gba_backsub (the
//                  points' updates, the trial errors and chi2), k_gba_ctl_trial (lm_rules.hpp)
//   the end        k_gba_finish (poses, points, marker poses as floats; the record)
// Sums: a thread adds its own items in their order (a point's observations; a contiguous run of a list), a wave adds its lanes by a
// fixed butterfly, the waves are added in order, the per-workgroup partial sums of a grid-wide pass the same way by one workgroup; a
// front adds its own blocks first, then the left child's complement, then the right one's.  No floating-point atomic anywhere.
#include "ba_edges.hpp"
#include "front_solve.hpp"
#include "gba_plan.hpp"
#include "host_stage.hpp"
#include "lm_dense.hpp"
#include "orbfe_common.hpp"
#include "se3_quat.hpp"
#include <cfloat>
#include <cmath>
#include <cstring>

namespace orbfe {
namespace {

constexpr int GBA_BAD_INVALID = 1;
static_assert(sizeof(SE3) == GBA_SE3_BYTES, "gba_plan.hpp lays the pose arrays out for this size");

struct GbaP {
    // the caller's arrays
    float* Tcw; float* x3Dw; const float* obs_xy; const int32_t* obs_oct; const int32_t* obs_feat; const orbfe_keypoint* kps;
    float* Twm; const float* mlocal; const float* mobs_corners; const uint8_t* stop; orbfe_gba_result* res;
    int nkf, np, nobs, nma, nmobs, nme, capacity, nlevels, use_markers, robust, npb, nb, nv, npairs, maxit, n_left_out;
    Cam K;
    double delta, marker_info;
    float inv_sigma2[GBA_MAX_LEVELS];
    // scratch: gba_scratch of gba_plan.hpp gives every pointer its array
    GbaCtl* ctl;
    double *xv, *xt, *xl;
    SE3* pose[2];          // nkf keyframes, then nma markers
    double* pt[2];         // np x 3
    int32_t* e_pt; float *e_ox, *e_oy, *e_info; uint8_t* e_use; double* e_blk;
    uint8_t* m_use; double* m_blk;
    double *Hll, *bl, *Dinv, *Hpp, *bp, *vmax, *S, *bs, *chi_part, *scale_part, *max_part;
    unsigned char* tables;
    double* fronts;
    // the plan's tables: gba_tables gives every pointer its array inside `tables`
    const FrontNode* nodes; const int32_t* node_vtx; const FrontSrc* src;
    const int32_t *cmap, *level_nodes, *kf_free, *v_kf, *v_active, *diag_pair, *vtx_eoff, *vtx_eitems, *vtx_moff, *vtx_mitems, *pair_u, *pair_v,
        *pair_off, *pair_items, *pair_moff, *pair_mitems, *obs_offset, *obs_kf, *mobs_offset, *mobs_kf, *mo_marker;
};

__device__ __forceinline__ bool stop_set(const GbaP& p) { return p.stop && *(const volatile uint8_t*)p.stop != 0; }

// the sum of n doubles: each thread a contiguous run, then the workgroup (valid in thread 0 behind block_sum)
__device__ __forceinline__ double gba_run_sum(const double* v, int n)
{
    const int per = (n + LM_THREADS - 1) / LM_THREADS;
    const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
    double s = 0;
    for (int i = lo; i < hi; i++) s += v[i];
    return s;
}

// ---------------------------------------------------------------------------------------- setup --
// the graph has been checked on the host; what is left are the values
__global__ __launch_bounds__(256) void k_gba_setup(GbaP p)
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
        if (!fin) bad |= GBA_BAD_INVALID;
        const SE3 S = se3_from_float(T);
        p.pose[0][i] = S;
        p.pose[1][i] = S;
    }
    if (i < p.np) {
        for (int k = 0; k < 3; k++) {
            const float v = p.x3Dw[(size_t)i * 3 + k];
            if (!finite_f(v)) bad |= GBA_BAD_INVALID;
            p.pt[0][(size_t)i * 3 + k] = v;
            p.pt[1][(size_t)i * 3 + k] = v;
        }
    }
    if (i < p.nobs) {
        // the point of slot i: the last point whose range starts at or before i (np > 0 here)
        int lo = 0, hi = p.np - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.obs_offset[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const int kf = p.obs_kf[i];
        int oct = 0;
        float ox = 0.f, oy = 0.f;
        if (p.obs_xy) {
            ox = p.obs_xy[(size_t)i * 2];
            oy = p.obs_xy[(size_t)i * 2 + 1];
            oct = p.obs_oct[i];
        } else {
            const int f = p.obs_feat[i];
            if (f < 0 || f >= p.capacity) bad |= GBA_BAD_INVALID;
            else {
                const orbfe_keypoint kp = p.kps[(size_t)kf * p.capacity + f];
                ox = kp.x; oy = kp.y; oct = kp.octave;
            }
        }
        if (oct < 0 || oct >= p.nlevels) {
            bad |= GBA_BAD_INVALID;
            oct = 0;
        }
        if (!finite_f(ox) || !finite_f(oy)) bad |= GBA_BAD_INVALID;
        p.e_pt[i] = lo; p.e_ox[i] = ox; p.e_oy[i] = oy; p.e_info[i] = p.inv_sigma2[oct];
    }
    if (i < p.nmobs)
        for (int k = 0; k < 8; k++)
            if (!finite_f(p.mobs_corners[(size_t)i * 8 + k])) bad |= GBA_BAD_INVALID;
    if (bad) atomicOr(&p.ctl->bad, bad);
}

// the call's fate: refused, stopped at the call, or under way.  One thread.
__global__ void k_gba_begin(GbaP p)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    GbaCtl& c = *p.ctl;
    if (c.bad & GBA_BAD_INVALID) c.abort_status = ORBFE_ERR_INVALID;
    else if (stop_set(p)) c.abort_status = ORBFE_GBA_STOPPED;
    c.aborted = c.abort_status != 0;
    c.iter_go = !c.aborted && p.maxit > 0;
    c.trial_go = 0;
    lm_round_start(c.lm);
}

// ---------------------------------------------------------------------------------------- linearisation --
__global__ __launch_bounds__(GBA_PT) void k_gba_linearize(GbaP p)
{
    const GbaCtl& c = *p.ctl;
    if (c.aborted || !c.iter_go) return;
    const int cur = c.cur;
    double chi = 0, md = 0;
    if ((int)blockIdx.x < p.npb) {
        const int pi = blockIdx.x * GBA_PT + threadIdx.x;
        if (pi < p.np) {
            const double Xw[3] = {p.pt[cur][(size_t)pi * 3], p.pt[cur][(size_t)pi * 3 + 1], p.pt[cur][(size_t)pi * 3 + 2]};
            double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
            const int lo = p.obs_offset[pi], hi = p.obs_offset[pi + 1];
            for (int e = lo; e < hi; e++) {
                const int kf = p.obs_kf[e];
                const SE3 T = p.pose[cur][kf];
                const double info = p.e_info[e];
                MonoLin L;
                lba_mono_linearize(T, Xw, p.e_ox[e], p.e_oy[e], p.K, L);
                const double ch = chi2_of(L.err, info);
                double rho[2] = {ch, 1.};
                if (p.robust) huber(ch, p.delta, rho);
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
                    double* out = p.e_blk + (size_t)e * GBA_EBLK;
                    lba_diag_block(L.Jp, w, r0, r1, out);
                    for (int a = 0; a < 6; a++)
                        for (int cc = 0; cc < 3; cc++) out[27 + a * 3 + cc] = L.Jp[0][a] * (w * L.Jx[0][cc]) + L.Jp[1][a] * (w * L.Jx[1][cc]);
                }
            }
            for (int k = 0; k < 6; k++) p.Hll[(size_t)pi * 6 + k] = H[k];
            for (int k = 0; k < 3; k++) p.bl[(size_t)pi * 3 + k] = b[k];
            if (hi > lo) md = fmax(fmax(fabs(H[0]), fabs(H[3])), fabs(H[5]));
        }
    } else {
        const int j = (blockIdx.x - p.npb) * GBA_PT + threadIdx.x;
        if (j < p.nme) {
            const int o = j >> 2, k = j & 3, kf = p.mobs_kf[o], m = p.mo_marker[o];
            const SE3 Tc = p.pose[cur][kf], Tm = p.pose[cur][p.nkf + m];
            const double pm[3] = {p.mlocal[(size_t)m * 12 + 3 * k], p.mlocal[(size_t)m * 12 + 3 * k + 1], p.mlocal[(size_t)m * 12 + 3 * k + 2]};
            const double ox = p.mobs_corners[(size_t)o * 8 + 2 * k], oy = p.mobs_corners[(size_t)o * 8 + 2 * k + 1];
            const bool camfree = p.kf_free[kf] >= 0;
            double err[2], Jc[2][6], Jm[2][6], rho[2];
            lba_marker_error(Tc, Tm, pm, ox, oy, p.K, err);
            const double ch = chi2_of(err, p.marker_info);
            huber(ch, p.delta, rho);
            chi += rho[0];
            for (int a = 0; a < 6; a++) Jc[0][a] = Jc[1][a] = 0;
            if (camfree) lba_marker_jacobian(Tc, Tm, true, pm, ox, oy, p.K, Jc);
            lba_marker_jacobian(Tc, Tm, false, pm, ox, oy, p.K, Jm);
            const bool fin = all_finite(err, 2) && all_finite(&Jc[0][0], 12) && all_finite(&Jm[0][0], 12) && isfinite(rho[1]);
            p.m_use[j] = fin ? 1 : 0;
            if (fin) {
                const double w = rho[1] * p.marker_info;
                const double r0 = rho[1] * -(p.marker_info * err[0]), r1 = rho[1] * -(p.marker_info * err[1]);
                double* out = p.m_blk + (size_t)j * GBA_MBLK;
                lba_diag_block(Jc, w, r0, r1, out);
                lba_diag_block(Jm, w, r0, r1, out + 27);
                for (int a = 0; a < 6; a++)
                    for (int cc = 0; cc < 6; cc++) out[54 + a * 6 + cc] = Jc[0][a] * (w * Jm[0][cc]) + Jc[1][a] * (w * Jm[1][cc]);
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

// Hpp and bp of free vertex v over its own edge lists: the monocular edges in point order (each thread a contiguous run of the
// list), then the marker corner edges in edge order
__global__ __launch_bounds__(LM_THREADS) void k_gba_pose_blocks(GbaP p)
{
    __shared__ double red[LM_WAVES * 27];
    const GbaCtl& c = *p.ctl;
    const int v = blockIdx.x, tid = threadIdx.x;
    if (c.aborted || !c.iter_go || v >= p.nv) return;
    double s[27];
    for (int k = 0; k < 27; k++) s[k] = 0;
    {
        const int first = p.vtx_eoff[v], n = p.vtx_eoff[v + 1] - first;
        const int per = (n + LM_THREADS - 1) / LM_THREADS;
        const int lo = min(tid * per, n), hi = min(lo + per, n);
        for (int it = lo; it < hi; it++) {
            const int e = p.vtx_eitems[first + it];
            if (p.e_use[e] != 3) continue;
            const double* blk = p.e_blk + (size_t)e * GBA_EBLK;
            for (int k = 0; k < 27; k++) s[k] += blk[k];
        }
    }
    block_sum<27>(s, red);
    if (tid != 0) return;
    const int side = p.v_kf[v] < p.nkf ? 0 : 27;   // a keyframe's half of a marker edge's blocks, or the marker's
    for (int it = p.vtx_moff[v]; it < p.vtx_moff[v + 1]; it++) {
        const int j = p.vtx_mitems[it];
        if (!p.m_use[j]) continue;
        const double* blk = p.m_blk + (size_t)j * GBA_MBLK + side;
        for (int k = 0; k < 27; k++) s[k] += blk[k];
    }
    double* H = p.Hpp + (size_t)v * 36;
    int k = 0;
    double md = 0;
    for (int a = 0; a < 6; a++)
        for (int cc = a; cc < 6; cc++, k++) H[a * 6 + cc] = H[cc * 6 + a] = s[k];
    for (int a = 0; a < 6; a++) {
        p.bp[(size_t)v * 6 + a] = s[21 + a];
        md = fmax(md, fabs(H[a * 6 + a]));
    }
    p.vmax[v] = p.v_active[v] ? md : 0;
}

__global__ __launch_bounds__(LM_THREADS) void k_gba_ctl_lin(GbaP p)
{
    __shared__ double red[LM_WAVES];
    __shared__ double mx[LM_THREADS];
    GbaCtl& c = *p.ctl;
    if (c.aborted || !c.iter_go) return;
    double s[1] = {gba_run_sum(p.chi_part, p.nb)};
    double m = 0;
    if (c.it == 0) {
        for (int i = threadIdx.x; i < p.nb; i += LM_THREADS) m = fmax(m, p.max_part[i]);
        for (int v = threadIdx.x; v < p.nv; v += LM_THREADS) m = fmax(m, p.vmax[v]);
    }
    mx[threadIdx.x] = m;
    block_sum<1>(s, red);
    if (threadIdx.x != 0) return;
    double md = 0;
    if (c.it == 0)
        for (int i = 0; i < LM_THREADS; i++) md = fmax(md, mx[i]);
    lm_linearised(c.lm, s[0], c.it == 0, md);
    if (c.it == 0) {
        c.lambda0 = c.lm.lambda;
        c.chi_first = s[0];
    }
    c.trial_go = 1;
    c.fail = 0;
}

// ---------------------------------------------------------------------------------------- a trial --
// (Hll + lambda I)^-1 by cofactors (Eigen's 3 x 3 inverse)
__global__ __launch_bounds__(GBA_PT) void k_gba_schur_points(GbaP p)
{
    const GbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int pi = blockIdx.x * GBA_PT + threadIdx.x;
    if (pi >= p.np || p.obs_offset[pi + 1] == p.obs_offset[pi]) return;
    const double* H = p.Hll + (size_t)pi * 6;
    const double m00 = H[0] + c.lm.lambda, m01 = H[1], m02 = H[2], m11 = H[3] + c.lm.lambda, m12 = H[4], m22 = H[5] + c.lm.lambda;
    const double c00 = m11 * m22 - m12 * m12, c10 = m12 * m02 - m01 * m22, c20 = m01 * m12 - m11 * m02;
    const double det = c00 * m00 + c10 * m01 + c20 * m02, id = 1. / det;
    double* D = p.Dinv + (size_t)pi * 9;
    D[0] = c00 * id; D[1] = c10 * id; D[2] = c20 * id;
    D[3] = D[1]; D[4] = (m00 * m22 - m02 * m02) * id; D[5] = (m02 * m01 - m00 * m12) * id;
    D[6] = D[2]; D[7] = D[5]; D[8] = (m00 * m11 - m01 * m01) * id;
}

// the block of covisible pair q = (u, v), u <= v, in its slot of S, and on the diagonal the rows u of the right-hand side; one wave:
// each lane a contiguous run of the pair's items, the lanes by a butterfly, then lane 0 the marker corner edges between the two
__global__ __launch_bounds__(64) void k_gba_reduce(GbaP p)
{
    const GbaCtl& c = *p.ctl;
    const int q = blockIdx.x, lane = threadIdx.x;
    if (c.aborted || !c.trial_go || q >= p.npairs) return;
    const int u = p.pair_u[q], v = p.pair_v[q];
    const bool diag = u == v;
    double acc[36], accb[6];
    for (int k = 0; k < 36; k++) acc[k] = 0;
    for (int k = 0; k < 6; k++) accb[k] = 0;
    const int first = p.pair_off[q], n = p.pair_off[q + 1] - first;
    if (n > 0) {
        const int per = (n + 63) / 64;
        const int lo = min(lane * per, n), hi = min(lo + per, n);
        for (int it = lo; it < hi; it++) {
            const int ei = p.pair_items[2 * (first + it)], ej = p.pair_items[2 * (first + it) + 1];
            if (p.e_use[ei] != 3 || p.e_use[ej] != 3) continue;
            const int pi = p.e_pt[ei];
            const double* Wi = p.e_blk + (size_t)ei * GBA_EBLK + 27;
            const double* Wj = p.e_blk + (size_t)ej * GBA_EBLK + 27;
            const double* D = p.Dinv + (size_t)pi * 9;
            const double* bl = p.bl + (size_t)pi * 3;
            for (int a = 0; a < 6; a++) {
                double Y[3];
                for (int cc = 0; cc < 3; cc++) Y[cc] = Wi[a * 3] * D[cc] + Wi[a * 3 + 1] * D[3 + cc] + Wi[a * 3 + 2] * D[6 + cc];
                for (int bb = 0; bb < 6; bb++) acc[a * 6 + bb] += Y[0] * Wj[bb * 3] + Y[1] * Wj[bb * 3 + 1] + Y[2] * Wj[bb * 3 + 2];
                if (diag) accb[a] += Y[0] * bl[0] + Y[1] * bl[1] + Y[2] * bl[2];
            }
        }
        for (int k = 0; k < 36; k++) acc[k] = wave_sum(acc[k]);
        if (diag)
            for (int k = 0; k < 6; k++) accb[k] = wave_sum(accb[k]);
    }
    if (lane != 0) return;
    double B[36];
    for (int k = 0; k < 36; k++) B[k] = 0;
    if (diag && !p.v_active[u]) {
        // a vertex without an edge is not part of the system: an identity block, a zero right-hand side
        for (int a = 0; a < 6; a++) B[a * 6 + a] = 1;
    } else if (diag) {
        for (int k = 0; k < 36; k++) B[k] = p.Hpp[(size_t)u * 36 + k];
        for (int a = 0; a < 6; a++) B[a * 6 + a] += c.lm.lambda;
        for (int k = 0; k < 36; k++) B[k] -= acc[k];
    } else {
        for (int k = 0; k < 36; k++) B[k] = 0. - acc[k];
        for (int it = p.pair_moff[q]; it < p.pair_moff[q + 1]; it++) {
            const int j = p.pair_mitems[it];
            if (!p.m_use[j]) continue;
            const double* blk = p.m_blk + (size_t)j * GBA_MBLK + 54;
            for (int k = 0; k < 36; k++) B[k] += blk[k];
        }
    }
    for (int k = 0; k < 36; k++) p.S[(size_t)q * 36 + k] = B[k];
    if (diag)
        for (int a = 0; a < 6; a++) p.bs[(size_t)u * 6 + a] = p.v_active[u] ? p.bp[(size_t)u * 6 + a] - accb[a] : 0.;
}

// the fronts of one level, a workgroup each; lds_rows: the largest front (in rows) the launch reserved LDS for
__global__ __launch_bounds__(LM_THREADS) void k_gba_front(GbaP p, int first, int lds_rows)
{
    extern __shared__ __align__(16) double gba_tri[];
    __shared__ int fail_s;
    GbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int tid = threadIdx.x;
    const FrontNode nd = p.nodes[p.level_nodes[first + blockIdx.x]];
    const int n = 6 * (nd.nown + nd.nb), k = 6 * nd.nown;
    if (n == 0) return;
    double* F = p.fronts + nd.front;
    double* r = F + (size_t)n * n;
    double* w = r + n;
    if (tid == 0) fail_s = 0;
    for (size_t idx = tid; idx < (size_t)n * n + n; idx += LM_THREADS) F[idx] = 0;
    __syncthreads();
    // its blocks of S: each goes to a place of its own (r >= c: the lower triangle, a diagonal block whole)
    for (int idx = tid; idx < nd.nsrc * 42; idx += LM_THREADS) {
        const FrontSrc s = p.src[nd.src + idx / 42];
        const int t = idx % 42;
        if (t < 36) {
            const int a = t / 6, cc = t % 6;
            F[(size_t)(6 * s.r + a) * n + 6 * s.c + cc] = (s.flags & 2) ? p.S[(size_t)s.id * 36 + cc * 6 + a] : p.S[(size_t)s.id * 36 + t];
        } else if (!(s.flags & 1)) {
            r[6 * s.r + t - 36] = p.bs[(size_t)p.node_vtx[nd.vtx + s.r] * 6 + t - 36];
        }
    }
    __syncthreads();
    // the children's Schur complements, left then right
    for (int ch = 0; ch < 2; ch++) {
        if (nd.child[ch] < 0) continue;
        const FrontNode cn = p.nodes[nd.child[ch]];
        const int m = 6 * (cn.nown + cn.nb), ck = 6 * cn.nown, cb = 6 * cn.nb;
        const double* G = p.fronts + cn.front;
        const double* gr = G + (size_t)m * m;
        const int32_t* map = p.cmap + nd.cmap[ch];
        for (int idx = tid; idx < cb * cb; idx += LM_THREADS) {
            const int bi = idx / cb, bj = idx % cb;
            if (bj > bi) continue;
            int R = 6 * map[bi / 6] + bi % 6, Cc = 6 * map[bj / 6] + bj % 6;
            if (R < Cc) {
                const int t = R; R = Cc; Cc = t;
            }
            F[(size_t)R * n + Cc] += G[(size_t)(ck + bi) * m + ck + bj];
        }
        for (int bi = tid; bi < cb; bi += LM_THREADS) r[6 * map[bi / 6] + bi % 6] += gr[ck + bi];
        __syncthreads();
    }
    bool ok;
    if (n <= lds_rows) {
        for (int i = 0; i < n; i++)
            for (int j = tid; j <= i; j += LM_THREADS) gba_tri[(size_t)i * (i + 1) / 2 + j] = F[(size_t)i * n + j];
        __syncthreads();
        ok = front_partial_llt<true>(gba_tri, n, k, r, &fail_s);
        if (ok)
            for (int i = 0; i < n; i++)
                for (int j = tid; j <= i; j += LM_THREADS) F[(size_t)i * n + j] = gba_tri[(size_t)i * (i + 1) / 2 + j];
        __syncthreads();
    } else {
        ok = front_partial_llt<false>(F, n, k, r, &fail_s);
    }
    if (!ok) {
        if (tid == 0) atomicOr(&c.fail, 1);
        return;
    }
    if (nd.nb == 0) front_substitute_back<6>(nd, p.node_vtx + nd.vtx, p.xt, F, r, w);
}

// the fronts of one level that have a boundary, top-down
__global__ __launch_bounds__(LM_THREADS) void k_gba_back(GbaP p, int first)
{
    const GbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go || c.fail) return;
    const FrontNode nd = p.nodes[p.level_nodes[first + blockIdx.x]];
    const int n = 6 * (nd.nown + nd.nb);
    if (nd.nb == 0 || nd.nown == 0) return;
    const double* F = p.fronts + nd.front;
    front_substitute_back<6>(nd, p.node_vtx + nd.vtx, p.xt, F, F + (size_t)n * n, p.fronts + nd.front + (size_t)n * n + n);
}

// the trial poses exp(x_v) T_v.  When the system was not solved the update of the last solved trial stays, as in g2o.
__global__ __launch_bounds__(256) void k_gba_update(GbaP p)
{
    const GbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= p.nv) return;
    const int cur = c.cur, idx = p.v_kf[v];
    if (!c.fail)
        for (int a = 0; a < 6; a++) p.xv[(size_t)v * 6 + a] = p.xt[(size_t)v * 6 + a];
    SE3 T = p.pose[cur][idx];
    if (p.v_active[v]) {
        double u[6];
        for (int a = 0; a < 6; a++) u[a] = p.xv[(size_t)v * 6 + a];
        T = mul(se3_exp(u), T);
    }
    p.pose[1 - cur][idx] = T;
}

// the point's update xl = D^-1 (bl - sum W^T x_pose), the trial point, the trial errors of every edge
__global__ __launch_bounds__(GBA_PT) void k_gba_backsub(GbaP p)
{
    const GbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int cur = c.cur, nxt = 1 - cur;
    double chi = 0, scale = 0;
    if ((int)blockIdx.x < p.npb) {
        const int pi = blockIdx.x * GBA_PT + threadIdx.x;
        if (pi < p.np) {
            double X[3] = {p.pt[cur][(size_t)pi * 3], p.pt[cur][(size_t)pi * 3 + 1], p.pt[cur][(size_t)pi * 3 + 2]};
            const int lo = p.obs_offset[pi], hi = p.obs_offset[pi + 1];
            if (hi > lo) {
                double* xl = p.xl + (size_t)pi * 3;
                const double* bl = p.bl + (size_t)pi * 3;
                if (!c.fail) {
                    double r[3] = {bl[0], bl[1], bl[2]};
                    for (int e = lo; e < hi; e++) {
                        if (p.e_use[e] != 3) continue;
                        const double* W = p.e_blk + (size_t)e * GBA_EBLK + 27;
                        const double* x = p.xv + (size_t)p.kf_free[p.obs_kf[e]] * 6;
                        for (int cc = 0; cc < 3; cc++) {
                            double s = 0;
                            for (int a = 0; a < 6; a++) s += W[a * 3 + cc] * x[a];
                            r[cc] -= s;
                        }
                    }
                    const double* D = p.Dinv + (size_t)pi * 9;
                    for (int a = 0; a < 3; a++) xl[a] = D[a * 3] * r[0] + D[a * 3 + 1] * r[1] + D[a * 3 + 2] * r[2];
                }
                for (int a = 0; a < 3; a++) {
                    scale += xl[a] * (c.lm.lambda * xl[a] + bl[a]);
                    X[a] += xl[a];
                }
                for (int e = lo; e < hi; e++) {
                    double err[2], rho[2];
                    lba_mono_error(p.pose[nxt][p.obs_kf[e]], X, p.e_ox[e], p.e_oy[e], p.K, err);
                    const double ch = chi2_of(err, (double)p.e_info[e]);
                    rho[0] = ch;
                    if (p.robust) huber(ch, p.delta, rho);
                    chi += rho[0];
                }
            }
            for (int a = 0; a < 3; a++) p.pt[nxt][(size_t)pi * 3 + a] = X[a];
        }
    } else {
        const int j = (blockIdx.x - p.npb) * GBA_PT + threadIdx.x;
        if (j < p.nme) {
            const int o = j >> 2, k = j & 3, m = p.mo_marker[o];
            const double pm[3] = {p.mlocal[(size_t)m * 12 + 3 * k], p.mlocal[(size_t)m * 12 + 3 * k + 1], p.mlocal[(size_t)m * 12 + 3 * k + 2]};
            double err[2], rho[2];
            lba_marker_error(p.pose[nxt][p.mobs_kf[o]], p.pose[nxt][p.nkf + m], pm, p.mobs_corners[(size_t)o * 8 + 2 * k],
                             p.mobs_corners[(size_t)o * 8 + 2 * k + 1], p.K, err);
            huber(chi2_of(err, p.marker_info), p.delta, rho);
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
__global__ __launch_bounds__(LM_THREADS) void k_gba_ctl_trial(GbaP p)
{
    __shared__ double red[LM_WAVES * 3];
    GbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    // chi2 and the points' x (lambda x + b) from the passes' partial sums, the poses' over the 6 nv unknowns: each thread a
    // contiguous run, then the workgroup
    const double lambda = c.lm.lambda;
    const int n = 6 * p.nv, per = (n + LM_THREADS - 1) / LM_THREADS;
    const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
    double s[3] = {gba_run_sum(p.chi_part, p.nb), gba_run_sum(p.scale_part, p.nb), 0.};
    for (int j = lo; j < hi; j++) s[2] += p.xv[j] * (lambda * p.xv[j] + (p.v_active[j / 6] ? p.bp[j] : 0.));
    block_sum<3>(s, red);
    if (threadIdx.x != 0) return;
    if (lm_judge_trial(c.lm, s[0], c.fail == 0, s[2] + s[1])) c.cur = 1 - c.cur;
    c.trials++;
    c.fail = 0;
    const bool halt = stop_set(p);
    const bool cont = lm_try_again(c.lm) && !halt;
    c.trial_go = cont;
    if (cont) return;
    c.it++;
    const bool stop = lm_iteration_end(c.lm);
    if (halt) c.stopped = 1;
    c.iter_go = !stop && !halt && c.it < p.maxit;
}

// ---------------------------------------------------------------------------------------- the end --
__global__ __launch_bounds__(256) void k_gba_finish(GbaP p)
{
    const GbaCtl& c = *p.ctl;
    const int i = blockIdx.x * 256 + threadIdx.x, cur = c.cur;
    if (i == 0) {
        orbfe_gba_result r{};
        r.status = c.abort_status;
        if (!c.aborted) {
            r.iterations = c.it;
            r.trials = c.trials;
            r.n_edges_mono = p.nobs;
            r.n_edges_marker = p.nme;
            r.n_points_left_out = p.n_left_out;
            r.chi2_first = c.chi_first;
            r.chi2_last = c.it ? c.lm.currentChi : 0.;
            r.lambda_last = c.lm.lambda;
        }
        *p.res = r;
    }
    if (c.aborted) return;
    if (i < p.nv && p.v_active[i]) {
        const int idx = p.v_kf[i];
        to_float(p.pose[cur][idx], idx < p.nkf ? p.Tcw + (size_t)idx * 12 : p.Twm + (size_t)(idx - p.nkf) * 12);
    }
    if (i < p.np && p.obs_offset[i + 1] > p.obs_offset[i])
        for (int k = 0; k < 3; k++) p.x3Dw[(size_t)i * 3 + k] = (float)p.pt[cur][(size_t)i * 3 + k];
}

// ---------------------------------------------------------------------------------------- host --
int report(const BaCheck& c) { return c.err ? fail(c.err, "%s", c.msg) : ORBFE_OK; }

// what a call is given beside its arrays: the camera and the level table (every entry finite here), the marker weight, the switches
int gba_fill(GbaP& p, const float* K4, const float* inv_sigma2, int nlevels, float marker_info, int use_markers, int robust, const char* name)
{
    BaCamera c;
    const int rc = report(ba_camera(c, K4, inv_sigma2, nlevels, marker_info, name, 5.99));
    if (rc) return rc;
    for (int l = 0; l < nlevels; l++)
        if (!std::isfinite(inv_sigma2[l])) return fail(ORBFE_ERR_INVALID, "%s: inv_level_sigma2 is not finite", name);
    p.nlevels = nlevels;
    for (int l = 0; l < GBA_MAX_LEVELS; l++) p.inv_sigma2[l] = c.inv_sigma2[l];
    p.K = Cam{c.fx, c.fy, c.cx, c.cy};
    p.marker_info = marker_info;
    p.delta = c.delta;
    p.use_markers = use_markers != 0;
    p.robust = robust != 0;
    return ORBFE_OK;
}

// The plan's tables on their way to the device, one page-locked block per (thread, device, stream).  A call overwrites the block of
// the call before it on the same stream, so it first waits until that call's copy has left the block (an event behind the copy).
struct GbaTablesStage {
    PinnedBuf pinned;
    hipEvent_t ev = nullptr;
    bool pending = false;
    ~GbaTablesStage() { if (ev) (void)hipEventDestroy(ev); }
};
thread_local ThreadWorkspaces<GbaTablesStage> tl_gba_tables;
thread_local ThreadWorkspaces<HostStage> tl_gba_stages;

struct GbaCall {
    GbaPlan plan;
    GbaSchedule k;
    std::vector<int> level_rows;   // front_level_lds_rows
    std::vector<unsigned char> blob;
    bool scratch_from_plan = false;   // the host calls: the scratch holds this plan's tables, blocks and fronts, not the bounds
};

// the scratch pointers and the tables of one call whose plan is made; p holds the caller's value arrays already
int gba_prepare(GbaCall& cl, GbaP& p, const GbaProblem& pb, int iterations, int leaf_vertices, bool inspect, void* scratch, hipStream_t s)
{
    int rc;
    const GbaSizes& n = pb.n;
    cl.k = gba_schedule(cl.plan, iterations, inspect, (size_t)max_lds());
    p.nkf = n.nkf; p.np = n.np; p.nobs = n.nobs; p.nma = n.nma; p.nmobs = n.nmobs;
    p.nme = p.use_markers ? 4 * n.nmobs : 0;
    p.npb = cl.k.npb;
    p.nb = cl.k.nb;
    p.nv = cl.plan.nv;
    p.npairs = cl.plan.npairs;
    p.maxit = cl.k.iterations;
    p.n_left_out = cl.plan.n_left_out;
    const GbaExtent x = gba_scratch(p, n, leaf_vertices, scratch, cl.scratch_from_plan ? &cl.plan : nullptr);
    cl.level_rows = front_level_lds_rows(cl.plan, 6, cl.k.lds_rows);
    gba_pack_tables(cl.blob, cl.plan, pb);
    gba_tables(p, gba_counts(cl.plan), p.tables);
    GbaTablesStage& ts = tl_gba_tables.get(s);
    if (ts.pending) ORBFE_HIP(hipEventSynchronize(ts.ev));
    if (!ts.ev) ORBFE_HIP(hipEventCreateWithFlags(&ts.ev, hipEventDisableTiming));
    if ((rc = ts.pinned.ensure(cl.blob.size()))) return rc;
    memcpy(ts.pinned.p, cl.blob.data(), cl.blob.size());
    ORBFE_HIP(hipMemsetAsync(scratch, 0, x.zero_end, s));
    ORBFE_HIP(hipMemcpyAsync(p.tables, ts.pinned.p, cl.blob.size(), hipMemcpyHostToDevice, s));
    ORBFE_HIP(hipEventRecord(ts.ev, s));
    ts.pending = true;
    return ensure_dyn_lds((const void*)k_gba_front, cl.k.tri_bytes);
}

int gba_enqueue_setup(const GbaCall& cl, const GbaP& p, hipStream_t s)
{
    hipLaunchKernelGGL(k_gba_setup, dim3(cl.k.g_setup), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_gba_begin, dim3(1), dim3(64), 0, s, p);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int gba_enqueue_iteration(const GbaCall& cl, const GbaP& p, hipStream_t s, bool inspect)
{
    const GbaPlan& pl = cl.plan;
    hipLaunchKernelGGL(k_gba_linearize, dim3(cl.k.g_pass), dim3(GBA_PT), 0, s, p);
    hipLaunchKernelGGL(k_gba_pose_blocks, dim3(cl.k.g_vertices), dim3(LM_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_gba_ctl_lin, dim3(1), dim3(LM_THREADS), 0, s, p);
    for (int q = 0; q < cl.k.trials; q++) {
        hipLaunchKernelGGL(k_gba_schur_points, dim3(cl.k.g_points), dim3(GBA_PT), 0, s, p);
        hipLaunchKernelGGL(k_gba_reduce, dim3(cl.k.g_pairs), dim3(64), 0, s, p);
        for (int l = 0; l < pl.nlevels; l++) {
            const int rows = cl.level_rows[(size_t)l];
            hipLaunchKernelGGL(k_gba_front, dim3(pl.level_off[(size_t)l + 1] - pl.level_off[(size_t)l]), dim3(LM_THREADS),
                               (size_t)rows * (rows + 1) / 2 * 8, s, p, pl.level_off[(size_t)l], rows);
        }
        for (int l = pl.nlevels - 2; l >= 0; l--)
            hipLaunchKernelGGL(k_gba_back, dim3(pl.level_off[(size_t)l + 1] - pl.level_off[(size_t)l]), dim3(LM_THREADS), 0, s, p, pl.level_off[(size_t)l]);
        hipLaunchKernelGGL(k_gba_update, dim3(cl.k.g_update), dim3(256), 0, s, p);
        hipLaunchKernelGGL(k_gba_backsub, dim3(cl.k.g_pass), dim3(GBA_PT), 0, s, p);
        if (!inspect) hipLaunchKernelGGL(k_gba_ctl_trial, dim3(1), dim3(LM_THREADS), 0, s, p);
    }
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int gba_enqueue_finish(const GbaCall& cl, const GbaP& p, hipStream_t s)
{
    hipLaunchKernelGGL(k_gba_finish, dim3(cl.k.g_setup), dim3(256), 0, s, p);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

// What both host calls do before they enqueue: the camera and every check, on the host alone, and the plan, so that a problem that
// is refused touches no device; then, unless the caller's stop flag is set already (ORBFE_GBA_STOPPED), the device, the stage of this
// thread with the values sent, the scratch, the tables.
int gba_host_begin(GbaCall& cl, GbaP& p, HostStage*& w, GbaHostIo& io, const GbaProblem& pb, const float* K4, const float* inv_sigma2, int nlevels,
                   float marker_info, int use_markers, int iterations, int robust, const uint8_t* stop, int leaf_vertices, bool inspect, int device,
                   const char* name)
{
    const GbaSizes& n = pb.n;
    int rc;
    if ((rc = report(gba_check_sizes(n, iterations, leaf_vertices, name))) || (rc = gba_fill(p, K4, inv_sigma2, nlevels, marker_info, use_markers, robust, name)) ||
        (rc = report(gba_check_graph(pb, name))) || (rc = report(gba_check_values(pb, nlevels, name))) ||
        (rc = report(gba_make_plan(cl.plan, pb, use_markers, leaf_vertices, name))))
        return rc;
    if (stop && *stop) return ORBFE_GBA_STOPPED;
    if ((rc = use_device(device))) return rc;
    w = &tl_gba_stages.get();
    io = gba_host_io(n);
    if ((rc = w->begin(io.io))) return rc;
    w->put(io.xy, pb.obs_xy, (size_t)n.nobs * 8); w->put(io.oct, pb.obs_octave, (size_t)n.nobs * 4);
    w->put(io.mloc, pb.marker_local, (size_t)n.nma * 48); w->put(io.mcor, pb.mobs_corners, (size_t)n.nmobs * 32);
    w->put(io.T, pb.Tcw, (size_t)n.nkf * 48); w->put(io.X, pb.x3Dw, (size_t)n.np * 12); w->put(io.M, pb.Twm, (size_t)n.nma * 48);
    if ((rc = w->upload())) return rc;
    p.obs_xy = w->dev<const float>(io.xy); p.obs_oct = w->dev<const int32_t>(io.oct); p.obs_feat = nullptr; p.kps = nullptr; p.capacity = 0;
    p.mlocal = w->dev<const float>(io.mloc); p.mobs_corners = w->dev<const float>(io.mcor);
    p.Tcw = w->dev<float>(io.T); p.x3Dw = w->dev<float>(io.X); p.Twm = w->dev<float>(io.M);
    p.res = w->dev<orbfe_gba_result>(io.res);
    p.stop = nullptr;
    cl.scratch_from_plan = true;
    if ((rc = w->host_scratch.ensure(gba_scratch_bytes(n, leaf_vertices, &cl.plan)))) return rc;
    return gba_prepare(cl, p, pb, iterations, leaf_vertices, inspect, w->host_scratch.p, w->stream);
}

} // namespace
} // namespace orbfe

using namespace orbfe;

extern "C" size_t orbfe_gba_scratch_bytes(int nkf, int np, int nobs, int nma, int nmobs, int leaf_vertices)
{
    const GbaSizes n{nkf, np, nobs, nma, nmobs};
    if (gba_check_sizes(n, 1, leaf_vertices, "orbfe_gba_scratch_bytes").err) return 0;
    return gba_scratch_bytes(n, leaf_vertices);
}

extern "C" int orbfe_global_bundle_adjustment(float* Tcw, const uint8_t* kf_fixed, int nkf, float* x3Dw, int np, const int32_t* obs_offset,
                                              const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                                              const float* inv_level_sigma2, int nlevels, float* Twm, const float* marker_local, int nma,
                                              const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs,
                                              float marker_info, int use_markers, int iterations, int robust, const uint8_t* stop, int leaf_vertices,
                                              orbfe_gba_result* res, int device)
{
    static const char* name = "orbfe_global_bundle_adjustment";
    if (!res) return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    const GbaProblem pb{{nkf, np, nobs, nma, nmobs}, Tcw, kf_fixed, x3Dw, obs_offset, obs_kf, obs_xy, obs_octave, nullptr, nullptr, 0,
                        Twm, marker_local, mobs_offset, mobs_kf, mobs_corners};
    GbaCall cl;
    GbaP p{};
    HostStage* w = nullptr;
    GbaHostIo io;
    int rc = gba_host_begin(cl, p, w, io, pb, K4, inv_level_sigma2, nlevels, marker_info, use_markers, iterations, robust, stop, leaf_vertices, false,
                            device, name);
    if (rc == ORBFE_GBA_STOPPED) {
        orbfe_gba_result r{};
        r.status = ORBFE_GBA_STOPPED;
        *res = r;
        return ORBFE_OK;
    }
    if (rc || (rc = gba_enqueue_setup(cl, p, w->stream))) return rc;
    // an iteration at a time: the control block says whether another one is due.  What is enqueued is what the device call enqueues,
    // minus launches that would return at once, so the two calls give the same bits.
    GbaCtl* hc = w->host<GbaCtl>(io.ctl);
    for (int it = 0; it < cl.k.iterations; it++) {
        if ((rc = gba_enqueue_iteration(cl, p, w->stream, false))) return rc;
        ORBFE_HIP(hipMemcpyAsync(hc, p.ctl, sizeof(GbaCtl), hipMemcpyDeviceToHost, w->stream));
        if ((rc = w->sync())) return rc;
        if (!hc->iter_go) break;
    }
    if ((rc = gba_enqueue_finish(cl, p, w->stream)) || (rc = w->download()) || (rc = w->sync())) return rc;
    const orbfe_gba_result r = *w->host<const orbfe_gba_result>(io.res);
    if (r.status < 0) return fail(r.status, "%s: the device refused the problem (status %d)", name, r.status);
    *res = r;
    w->get(Tcw, io.T, (size_t)nkf * 48);
    w->get(x3Dw, io.X, (size_t)np * 12);
    if (use_markers) w->get(Twm, io.M, (size_t)nma * 48);
    return ORBFE_OK;
}

extern "C" int orbfe_global_bundle_adjustment_device(float* d_Tcw, const uint8_t* kf_fixed, int nkf, float* d_x3Dw, int np,
                                                     const int32_t* obs_offset, const int32_t* obs_kf, const float* d_obs_xy,
                                                     const int32_t* d_obs_octave, const int32_t* d_obs_feature, const orbfe_keypoint* d_kps,
                                                     int capacity, int nobs, const float* K4, const float* inv_level_sigma2, int nlevels,
                                                     float* d_Twm, const float* d_marker_local, int nma, const int32_t* mobs_offset,
                                                     const int32_t* mobs_kf, const float* d_mobs_corners, int nmobs, float marker_info,
                                                     int use_markers, int iterations, int robust, const uint8_t* d_stop, int leaf_vertices,
                                                     orbfe_gba_result* d_res, void* d_scratch, size_t scratch_bytes, void* stream)
{
    static const char* name = "orbfe_global_bundle_adjustment_device";
    const GbaProblem d{{nkf, np, nobs, nma, nmobs}, d_Tcw, kf_fixed, d_x3Dw, obs_offset, obs_kf, d_obs_xy, d_obs_octave, d_obs_feature,
                       d_kps, capacity, d_Twm, d_marker_local, mobs_offset, mobs_kf, d_mobs_corners};
    GbaCall cl;
    GbaP p{};
    int rc;
    if ((rc = report(gba_check_sizes(d.n, iterations, leaf_vertices, name))) || (rc = report(gba_check_device(d, d_res, d_scratch, name)))) return rc;
    const size_t need = gba_scratch_bytes(d.n, leaf_vertices);
    if (scratch_bytes < need) return fail(ORBFE_ERR_CAPACITY, "%s: %zu bytes of scratch, orbfe_gba_scratch_bytes asks for %zu", name, scratch_bytes, need);
    if ((rc = gba_fill(p, K4, inv_level_sigma2, nlevels, marker_info, use_markers, robust, name)) || (rc = report(gba_check_graph(d, name))) ||
        (rc = report(gba_make_plan(cl.plan, d, use_markers, leaf_vertices, name))))
        return rc;
    p.Tcw = d_Tcw; p.x3Dw = d_x3Dw; p.obs_xy = d_obs_xy; p.obs_oct = d_obs_octave; p.obs_feat = d_obs_feature; p.kps = d_kps; p.capacity = capacity;
    p.Twm = d_Twm; p.mlocal = d_marker_local; p.mobs_corners = d_mobs_corners; p.stop = d_stop; p.res = d_res;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = gba_prepare(cl, p, d, iterations, leaf_vertices, false, d_scratch, s)) || (rc = gba_enqueue_setup(cl, p, s))) return rc;
    for (int it = 0; it < cl.k.iterations; it++)
        if ((rc = gba_enqueue_iteration(cl, p, s, false))) return rc;
    return gba_enqueue_finish(cl, p, s);
}

extern "C" int orbfe_gba_inspect(const float* Tcw, const uint8_t* kf_fixed, int nkf, const float* x3Dw, int np, const int32_t* obs_offset,
                                 const int32_t* obs_kf, const float* obs_xy, const int32_t* obs_octave, int nobs, const float* K4,
                                 const float* inv_level_sigma2, int nlevels, const float* Twm, const float* marker_local, int nma,
                                 const int32_t* mobs_offset, const int32_t* mobs_kf, const float* mobs_corners, int nmobs, float marker_info,
                                 int use_markers, int robust, int leaf_vertices, int32_t* nv, double* b, double* Hpp, double* Hll, double* chi2,
                                 double* x, int32_t* tree, int device)
{
    static const char* name = "orbfe_gba_inspect";
    if (!nv || !b || !Hpp || !Hll || !chi2 || !x || !tree) return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    // the estimates are read only: an inspect call fetches nothing back into them
    const GbaProblem pb{{nkf, np, nobs, nma, nmobs}, const_cast<float*>(Tcw), kf_fixed, const_cast<float*>(x3Dw), obs_offset, obs_kf, obs_xy,
                        obs_octave, nullptr, nullptr, 0, const_cast<float*>(Twm), marker_local, mobs_offset, mobs_kf, mobs_corners};
    GbaCall cl;
    GbaP p{};
    HostStage* w = nullptr;
    GbaHostIo io;
    int rc;
    if ((rc = gba_host_begin(cl, p, w, io, pb, K4, inv_level_sigma2, nlevels, marker_info, use_markers, 1, robust, nullptr, leaf_vertices, true, device,
                             name)) ||
        (rc = gba_enqueue_setup(cl, p, w->stream)) || (rc = gba_enqueue_iteration(cl, p, w->stream, true)) || (rc = w->sync()))
        return rc;
    GbaCtl c;
    ORBFE_HIP(hipMemcpy(&c, p.ctl, sizeof(c), hipMemcpyDeviceToHost));
    if (c.abort_status < 0) return fail(c.abort_status, "%s: the device refused the problem (status %d)", name, c.abort_status);
    const GbaPlan& pl = cl.plan;
    *nv = pl.nv;
    chi2[0] = c.lm.currentChi;
    chi2[1] = c.lambda0;
    chi2[2] = c.fail ? 0. : 1.;
    if (pl.nv) {
        ORBFE_HIP(hipMemcpy(b, p.bp, (size_t)pl.nv * 48, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(Hpp, p.Hpp, (size_t)pl.nv * 288, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(x, p.xv, (size_t)pl.nv * 48, hipMemcpyDeviceToHost));
    }
    if (np) {
        ORBFE_HIP(hipMemcpy(b + 6 * pl.nv, p.bl, (size_t)np * 24, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(Hll, p.Hll, (size_t)np * 48, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(x + 6 * pl.nv, p.xl, (size_t)np * 24, hipMemcpyDeviceToHost));
    }
    // the plan: nodes, levels; per free vertex its node and its place in the elimination order; per node parent, level, own, boundary
    int32_t* t = tree;
    *t++ = (int32_t)pl.nodes.size();
    *t++ = pl.nlevels;
    for (int v = 0; v < pl.nv; v++) *t++ = pl.node_of[(size_t)v];
    for (int v = 0; v < pl.nv; v++) *t++ = pl.order_of[(size_t)v];
    for (const FrontNode& nd : pl.nodes) {
        *t++ = nd.parent; *t++ = nd.level; *t++ = nd.nown; *t++ = nd.nb;
    }
    return ORBFE_OK;
}
