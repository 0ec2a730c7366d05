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
        const ObsPixel o = obs_pixel(i, p.obs_kf[i], p.obs_xy, p.obs_oct, p.obs_feat, p.kps, p.capacity, p.nlevels);
        if (!o.ok) bad |= GBA_BAD_INVALID;
        p.e_pt[i] = obs_point(p.obs_offset, p.np, i); p.e_ox[i] = o.x; p.e_oy[i] = o.y; p.e_info[i] = p.inv_sigma2[o.oct];
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
    else if (stop_set(p.stop)) c.abort_status = ORBFE_GBA_STOPPED;
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
            double ch, rho0;
            p.m_use[j] = marker_edge_linearize(Tc, Tm, marker_corner(p.mlocal, p.mobs_corners, m, o, k), p.K, p.kf_free[kf] >= 0, true, p.marker_info,
                                               p.delta, p.m_blk + (size_t)j * GBA_MBLK, ch, rho0);
            chi += rho0;
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
    const int first = p.vtx_eoff[v];
    run_for(p.vtx_eoff[v + 1] - first, [&](int it) {
        const int e = p.vtx_eitems[first + it];
        if (p.e_use[e] != 3) return;
        const double* blk = p.e_blk + (size_t)e * GBA_EBLK;
        for (int k = 0; k < 27; k++) s[k] += blk[k];
    });
    block_sum<27>(s, red);
    if (tid != 0) return;
    const int side = p.v_kf[v] < p.nkf ? 0 : 27;   // a keyframe's half of a marker edge's blocks, or the marker's
    for (int it = p.vtx_moff[v]; it < p.vtx_moff[v + 1]; it++) {
        const int j = p.vtx_mitems[it];
        if (!p.m_use[j]) continue;
        const double* blk = p.m_blk + (size_t)j * GBA_MBLK + side;
        for (int k = 0; k < 27; k++) s[k] += blk[k];
    }
    const double md = unpack_pose_sums(s, p.Hpp + (size_t)v * 36, p.bp + (size_t)v * 6);
    p.vmax[v] = p.v_active[v] ? md : 0;
}

__global__ __launch_bounds__(LM_THREADS) void k_gba_ctl_lin(GbaP p)
{
    __shared__ double red[LM_WAVES];
    __shared__ double mx[LM_THREADS];
    GbaCtl& c = *p.ctl;
    if (c.aborted || !c.iter_go) return;
    double s[1] = {run_sum(p.chi_part, p.nb)};
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
// (Hll + lambda I)^-1 of every point that has an edge
__global__ __launch_bounds__(GBA_PT) void k_gba_schur_points(GbaP p)
{
    const GbaCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int pi = blockIdx.x * GBA_PT + threadIdx.x;
    if (pi >= p.np || p.obs_offset[pi + 1] == p.obs_offset[pi]) return;
    damped_inverse3(p.Hll + (size_t)pi * 6, c.lm.lambda, p.Dinv + (size_t)pi * 9);
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
        run_for<64>(n, [&](int it) {
            const int ei = p.pair_items[2 * (first + it)], ej = p.pair_items[2 * (first + it) + 1];
            if (p.e_use[ei] != 3 || p.e_use[ej] != 3) return;
            const int pi = p.e_pt[ei];
            pair_item_add(p.e_blk + (size_t)ei * GBA_EBLK + 27, p.e_blk + (size_t)ej * GBA_EBLK + 27, p.Dinv + (size_t)pi * 9, p.bl + (size_t)pi * 3, diag, acc,
                          accb);
        });
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
    front_merge_children<6>(nd, p.nodes, p.cmap, p.fronts, F, r);
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
    front_back<6>(p.nodes[p.level_nodes[first + blockIdx.x]], p.fronts, p.node_vtx, p.xt);
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
                        point_rhs_sub(p.e_blk + (size_t)e * GBA_EBLK + 27, p.xv + (size_t)p.kf_free[p.obs_kf[e]] * 6, r);
                    }
                    point_solve(p.Dinv + (size_t)pi * 9, r, xl);
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
            const MarkerCorner mc = marker_corner(p.mlocal, p.mobs_corners, m, o, k);
            double err[2], rho[2];
            lba_marker_error(p.pose[nxt][p.mobs_kf[o]], p.pose[nxt][p.nkf + m], mc.pm, mc.ox, mc.oy, p.K, err);
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
    double s[3] = {run_sum(p.chi_part, p.nb), run_sum(p.scale_part, p.nb), 0.};
    run_for(6 * p.nv, [&](int j) { s[2] += p.xv[j] * (lambda * p.xv[j] + (p.v_active[j / 6] ? p.bp[j] : 0.)); });
    block_sum<3>(s, red);
    if (threadIdx.x != 0) return;
    if (lm_judge_trial(c.lm, s[0], c.fail == 0, s[2] + s[1])) c.cur = 1 - c.cur;
    c.trials++;
    c.fail = 0;
    const bool halt = stop_set(p.stop);
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
thread_local ThreadWorkspaces<TablesStage> tl_gba_tables;
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
    ORBFE_HIP(hipMemsetAsync(scratch, 0, x.zero_end, s));
    if ((rc = tl_gba_tables.get(s).send(cl.blob, p.tables, s))) return rc;
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
    hipLaunchKernelGGL(k_gba_linearize, dim3(cl.k.g_pass), dim3(GBA_PT), 0, s, p);
    hipLaunchKernelGGL(k_gba_pose_blocks, dim3(cl.k.g_vertices), dim3(LM_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_gba_ctl_lin, dim3(1), dim3(LM_THREADS), 0, s, p);
    for (int q = 0; q < cl.k.trials; q++) {
        hipLaunchKernelGGL(k_gba_schur_points, dim3(cl.k.g_points), dim3(GBA_PT), 0, s, p);
        hipLaunchKernelGGL(k_gba_reduce, dim3(cl.k.g_pairs), dim3(64), 0, s, p);
        front_enqueue_levels(k_gba_front, k_gba_back, cl.plan.level_off, cl.level_rows, LM_THREADS, p, s);
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
    p.robust = robust != 0;
    if ((rc = report(gba_check_sizes(n, iterations, leaf_vertices, name))) || (rc = ba_fill(p, K4, inv_sigma2, nlevels, marker_info, use_markers, 5.99, name)) ||
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
    p.robust = robust != 0;
    if ((rc = ba_fill(p, K4, inv_level_sigma2, nlevels, marker_info, use_markers, 5.99, name)) || (rc = report(gba_check_graph(d, name))) ||
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
