// essential_graph.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1245-1542) behind its collect step, on gfx950: the
// pose graph of loop closing.  Sim3 vertices (one fixed), EdgeSim3 edges with identity information and no robust kernel, g2o's
// Levenberg-Marquardt with setUserLambdaInit(1e-16), 20 iterations; then the SE3 recovery of every keyframe and the correction of
// every map point through its reference keyframe.
//
// The sparsity pattern is fixed for a call, so everything symbolic is host arithmetic (essential_plan.hpp): the elimination tree of
// a nested dissection, the tables the kernels walk, the scratch layout, the launch schedule.  The LM state lives on the device (EgCtl,
// two copies of every estimate), the call is a chain of launches whose number depends on the plan and not on the values, and a launch
// whose step is already decided returns at once.  No kernel waits on another workgroup; every device loop has a bound from the plan.
//   setup          k_eg_setup (the similarity tables, validation), k_eg_init (vScw and the estimates, the call's fate), k_eg_measure
//                  (the measurement of every edge by its kind)
//   an iteration   k_eg_linearize (16 lanes an edge: a lane per (side, column) does the two perturbed errors of g2o's central
//                  difference, lane 14 the error itself), k_eg_blocks (a wave per vertex: H_vv = sum J^T J and b_v = -sum J^T e over
//                  the vertex's edges in edge order; a wave per pair: H_uv over the pair's edges in edge order), k_eg_ctl_lin (chi2)
//   a trial        k_eg_front once per level, leaves first, a workgroup per front: the front's blocks with lambda on the diagonal,
//                  plus the children's Schur complements (left, then right) by their scatter maps; partial Cholesky of the own
//                  columns, which leaves the boundary's Schur complement in place; the right-hand side rides along as one more column.
//                  A front without a boundary substitutes back at once; k_eg_back once per level downwards does the others.
//                  k_eg_update (the trial estimates Sim3(x) * estimate), k_eg_trial_errors, k_eg_ctl_trial (lm_rules.hpp)
//   the end        k_eg_finish (a thread per keyframe: [R t/s]; a thread per point: the two maps; the record)
// Sums: a lane adds its items in their order, a workgroup's partial sums are added in wave order (block_sum); a front adds its own
// blocks first, then the left child's complement, then the right one's.  No floating-point atomic anywhere.
// A non-positive or non-finite pivot in any front means "not solved": the trial is judged with chi2 = DBL_MAX and the update of the
// last solved trial stays, as g2o's does.
#include "essential_plan.hpp"
#include "front_solve.hpp"
#include "host_stage.hpp"
#include "lm_dense.hpp"
#include "orbfe_common.hpp"
#include "sim3_group.hpp"
#include <cfloat>
#include <cmath>
#include <cstring>

namespace orbfe {
namespace {

constexpr int EG_BAD_INVALID = 1;
static_assert(sizeof(Sim3) == EG_SIM3_BYTES, "essential_plan.hpp lays the similarity arrays out for this size");

struct EgP {
    // the caller's arrays
    const float* Tcw; const int32_t* cpos; const double* csim; const int32_t* npos; const double* nsim; const float* x3Dw; const int32_t* pref;
    float* Tcw_out; float* x3Dw_out; double* Siw_out; orbfe_eg_result* res;
    int nkf, ne, np, nc, nn, fixed, fix_scale, npairs, maxit, passthrough;
    // scratch: eg_scratch of essential_plan.hpp gives every pointer its array
    EgCtl* ctl;
    double *xv, *xt;
    int32_t *kf_nc, *kf_c;
    Sim3 *S0, *est[2], *meas;
    double *e_err, *e_chi, *Ji, *Jj, *Hd, *bv, *Hp;
    unsigned char* tables;
    double* fronts;
    // the plan's tables: eg_tables gives every pointer its array inside `tables`
    const EgNode* nodes; const int32_t* node_vtx; const EgSrc* src;
    const int32_t *cmap, *level_nodes, *pair_u, *pair_v, *pair_off, *pair_items, *vtx_off, *vtx_items, *edge_i, *edge_j, *edge_kind;
};

// ---------------------------------------------------------------------------------------- small pieces --
__device__ __forceinline__ Sim3 sim_from8(const double* v)
{
    Sim3 S;
    S.q = Quat{v[0], v[1], v[2], v[3]};
    S.t[0] = v[4]; S.t[1] = v[5]; S.t[2] = v[6];
    S.s = v[7];
    return S;
}

__device__ __forceinline__ void sim_to8(const Sim3& S, double* v)
{
    v[0] = S.q.x; v[1] = S.q.y; v[2] = S.q.z; v[3] = S.q.w;
    v[4] = S.t[0]; v[5] = S.t[1]; v[6] = S.t[2];
    v[7] = S.s;
}

// g2o::Sim3(R, t, 1.) of a 3 x 4 float pose: Eigen's matrix-to-quaternion, not normalised
__device__ Sim3 sim_from_pose(const float* Rt)
{
    double R[3][3];
    Sim3 S;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r][c] = Rt[r * 4 + c];
        S.t[r] = Rt[r * 4 + 3];
    }
    S.q = quat_from_matrix(R);
    S.s = 1.;
    return S;
}

// EdgeSim3::computeError: (C * v1 * v2^-1).log()
__device__ __noinline__ void eg_error(const Sim3& C, const Sim3& Si, const Sim3& Sj, double (&err)[7])
{
    const Sim3 E = mul(mul(C, Si), inverse(Sj));
    sim3_log(E, err);
}

// ---------------------------------------------------------------------------------------- setup --
__global__ __launch_bounds__(256) void k_eg_setup(EgP p)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    for (int which = 0; which < 2; which++) {
        const int cnt = which ? p.nn : p.nc;
        const int32_t* pos = which ? p.npos : p.cpos;
        const double* sim = which ? p.nsim : p.csim;
        int32_t* tbl = which ? p.kf_nc : p.kf_c;
        if (i >= cnt) continue;
        bool fin = true;
        for (int a = 0; a < 8; a++) fin = fin && isfinite(sim[(size_t)i * 8 + a]);
        if (!fin || !(sim[(size_t)i * 8 + 7] > 0)) bad |= EG_BAD_INVALID;
        if (pos[i] < 0 || pos[i] >= p.nkf) bad |= EG_BAD_INVALID;
        else if (atomicCAS(&tbl[pos[i]], -1, i) != -1) bad |= EG_BAD_INVALID;   // a keyframe has one entry
    }
    if (i < p.nkf)
        for (int a = 0; a < 12; a++)
            if (!isfinite(p.Tcw[(size_t)i * 12 + a])) bad |= EG_BAD_INVALID;
    if (i < p.np) {
        if (p.pref[i] < -1 || p.pref[i] >= p.nkf) bad |= EG_BAD_INVALID;
        for (int a = 0; a < 3; a++)
            if (!isfinite(p.x3Dw[(size_t)i * 3 + a])) bad |= EG_BAD_INVALID;
    }
    if (bad) atomicOr(&p.ctl->bad, bad);
}

__global__ __launch_bounds__(256) void k_eg_init(EgP p)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        EgCtl& c = *p.ctl;
        if (c.bad & EG_BAD_INVALID) c.abort_status = ORBFE_ERR_INVALID;
        c.aborted = c.abort_status != 0;
        c.iter_go = !c.aborted && !p.passthrough && p.maxit > 0;
        lm_round_start(c.lm);
    }
    if (i >= p.nkf || (p.ctl->bad & EG_BAD_INVALID)) return;
    const int k = p.kf_c[i];
    const Sim3 S = k >= 0 ? sim_from8(p.csim + (size_t)k * 8) : sim_from_pose(p.Tcw + (size_t)i * 12);
    p.S0[i] = S;
    p.est[0][i] = S;
    p.est[1][i] = S;
}

// kind 0 (LoopConnections): vScw[j] * vScw[i]^-1.  kind 1 (spanning tree, old loop edges, covisibility): the same with the
// NonCorrectedSim3 entry of a keyframe that has one.
__global__ __launch_bounds__(256) void k_eg_measure(EgP p)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (p.ctl->aborted || e >= p.ne) return;
    const int i = p.edge_i[e], j = p.edge_j[e];
    Sim3 Siw = p.S0[i], Sjw = p.S0[j];
    if (p.edge_kind[e] == 1) {
        if (p.kf_nc[i] >= 0) Siw = sim_from8(p.nsim + (size_t)p.kf_nc[i] * 8);
        if (p.kf_nc[j] >= 0) Sjw = sim_from8(p.nsim + (size_t)p.kf_nc[j] * 8);
    }
    p.meas[e] = mul(Sjw, inverse(Siw));
}

// ---------------------------------------------------------------------------------------- linearisation --
// BaseBinaryEdge::linearizeOplus: column d of the Jacobian of a free vertex is (e(+) - e(-)) / 2e-9 with the vertex at
// Sim3(+-1e-9 e_d) * estimate (update[6] = 0 under fix_scale, VertexSim3Expmap::oplusImpl); the fixed vertex has none.
__global__ __launch_bounds__(256) void k_eg_linearize(EgP p)
{
    const EgCtl& c = *p.ctl;
    if (c.aborted || !c.iter_go) return;
    const int g = blockIdx.x * 256 + threadIdx.x, e = g >> 4, l = g & 15;
    if (e >= p.ne || l == 15) return;
    const int i = p.edge_i[e], j = p.edge_j[e];
    const Sim3 Si = p.est[c.cur][i], Sj = p.est[c.cur][j], C = p.meas[e];
    if (l == 14) {
        double err[7], chi = 0;
        eg_error(C, Si, Sj, err);
        for (int k = 0; k < 7; k++) {
            p.e_err[(size_t)e * 7 + k] = err[k];
            chi += err[k] * err[k];
        }
        p.e_chi[e] = chi;
        return;
    }
    const int side = l / 7, d = l % 7;
    double* J = (side ? p.Jj : p.Ji) + (size_t)e * 49;
    if ((side ? j : i) == p.fixed) {
        for (int k = 0; k < 7; k++) J[k * 7 + d] = 0;
        return;
    }
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    double ep[7], em[7];
    for (int sgn = 0; sgn < 2; sgn++) {
        double u[7] = {0, 0, 0, 0, 0, 0, 0};
        u[d] = sgn ? -delta : delta;
        if (p.fix_scale) u[6] = 0;
        const Sim3 E = sim3_exp(u);
        const Sim3 Sp = mul(E, side ? Sj : Si);
        if (side) eg_error(C, Si, Sp, sgn ? em : ep);
        else eg_error(C, Sp, Sj, sgn ? em : ep);
    }
    for (int k = 0; k < 7; k++) J[k * 7 + d] = scalar * (ep[k] - em[k]);
}

// a wave per vertex (blocks 0 .. nkf - 1), then per pair: lane a * 7 + c one entry of the 7 x 7 block, lanes 49 .. 55 the vertex's b
__global__ __launch_bounds__(64) void k_eg_blocks(EgP p)
{
    const EgCtl& c = *p.ctl;
    if (c.aborted || !c.iter_go) return;
    const int t = threadIdx.x;
    if ((int)blockIdx.x < p.nkf) {
        const int v = blockIdx.x;
        if (t >= 56) return;
        const int a = t < 49 ? t / 7 : t - 49, cc = t % 7;
        double s = 0;
        for (int it = p.vtx_off[v]; it < p.vtx_off[v + 1]; it++) {
            const int e = p.vtx_items[it] >> 1;
            const double* J = ((p.vtx_items[it] & 1) ? p.Jj : p.Ji) + (size_t)e * 49;
            double q = 0;
            if (t < 49)
                for (int k = 0; k < 7; k++) q += J[k * 7 + a] * J[k * 7 + cc];
            else
                for (int k = 0; k < 7; k++) q += J[k * 7 + a] * -p.e_err[(size_t)e * 7 + k];
            s += q;
        }
        if (t < 49) p.Hd[(size_t)v * 49 + t] = s;
        else p.bv[(size_t)v * 7 + a] = s;
    } else {
        const int q = blockIdx.x - p.nkf;
        if (q >= p.npairs || t >= 49) return;
        const int a = t / 7, cc = t % 7;
        double s = 0;
        for (int it = p.pair_off[q]; it < p.pair_off[q + 1]; it++) {
            const int e = p.pair_items[it] >> 1, flip = p.pair_items[it] & 1;
            const double* Ju = (flip ? p.Jj : p.Ji) + (size_t)e * 49;
            const double* Jv = (flip ? p.Ji : p.Jj) + (size_t)e * 49;
            double r = 0;
            for (int k = 0; k < 7; k++) r += Ju[k * 7 + a] * Jv[k * 7 + cc];
            s += r;
        }
        p.Hp[(size_t)q * 49 + t] = s;
    }
}

__global__ __launch_bounds__(LM_THREADS) void k_eg_ctl_lin(EgP p)
{
    __shared__ double red[LM_WAVES];
    EgCtl& c = *p.ctl;
    if (c.aborted || !c.iter_go) return;
    double s[1] = {run_sum(p.e_chi, p.ne)};
    block_sum<1>(s, red);
    if (threadIdx.x != 0) return;
    lm_linearised_user(c.lm, s[0], c.it == 0, EG_LAMBDA_INIT);
    if (c.it == 0) {
        c.lambda0 = c.lm.lambda;
        c.chi_first = s[0];
    }
    c.trial_go = 1;
    c.fail = 0;
}

// ---------------------------------------------------------------------------------------- a trial --
// The partial Cholesky factorisation of a front and its substitution back are front_solve.hpp's, shared with global_ba.hip.
// the fronts of one level, a workgroup each; lds_rows: the largest front (in rows) the launch reserved LDS for
__global__ __launch_bounds__(LM_THREADS) void k_eg_front(EgP p, int first, int lds_rows)
{
    extern __shared__ __align__(16) double eg_tri[];
    __shared__ int fail_s;
    EgCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int tid = threadIdx.x;
    const EgNode nd = p.nodes[p.level_nodes[first + blockIdx.x]];
    const int n = 7 * (nd.nown + nd.nb), k = 7 * nd.nown;
    if (n == 0) return;
    double* F = p.fronts + nd.front;
    double* r = F + (size_t)n * n;
    double* w = r + n;
    const double lambda = c.lm.lambda;
    if (tid == 0) fail_s = 0;
    for (size_t idx = tid; idx < (size_t)n * n + n; idx += LM_THREADS) F[idx] = 0;
    __syncthreads();
    // its blocks of the linearised system: each goes to a place of its own
    for (int idx = tid; idx < nd.nsrc * 56; idx += LM_THREADS) {
        const EgSrc s = p.src[nd.src + idx / 56];
        const int t = idx % 56;
        if (t < 49) {
            const int a = t / 7, cc = t % 7;
            double v;
            if (s.flags & 1) v = (s.flags & 2) ? p.Hp[(size_t)s.id * 49 + cc * 7 + a] : p.Hp[(size_t)s.id * 49 + t];
            else v = p.Hd[(size_t)s.id * 49 + t] + (a == cc ? lambda : 0.);
            F[(size_t)(7 * s.r + a) * n + 7 * s.c + cc] = v;
        } else if (!(s.flags & 1)) {
            r[7 * s.r + t - 49] = p.bv[(size_t)s.id * 7 + t - 49];
        }
    }
    __syncthreads();
    front_merge_children<7>(nd, p.nodes, p.cmap, p.fronts, F, r);
    bool ok;
    if (n <= lds_rows) {
        for (int i = 0; i < n; i++)
            for (int j = tid; j <= i; j += LM_THREADS) eg_tri[(size_t)i * (i + 1) / 2 + j] = F[(size_t)i * n + j];
        __syncthreads();
        ok = front_partial_llt<true>(eg_tri, n, k, r, &fail_s);
        if (ok)
            for (int i = 0; i < n; i++)
                for (int j = tid; j <= i; j += LM_THREADS) F[(size_t)i * n + j] = eg_tri[(size_t)i * (i + 1) / 2 + j];
        __syncthreads();
    } else {
        ok = front_partial_llt<false>(F, n, k, r, &fail_s);
    }
    if (!ok) {
        if (tid == 0) atomicOr(&c.fail, 1);
        return;
    }
    if (nd.nb == 0) front_substitute_back<7>(nd, p.node_vtx + nd.vtx, p.xt, F, r, w);
}

// the fronts of one level that have a boundary, top-down
__global__ __launch_bounds__(LM_THREADS) void k_eg_back(EgP p, int first)
{
    const EgCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go || c.fail) return;
    front_back<7>(p.nodes[p.level_nodes[first + blockIdx.x]], p.fronts, p.node_vtx, p.xt);
}

// the trial estimates: VertexSim3Expmap::oplusImpl.  When the system was not solved the update of the last solved trial stays.
__global__ __launch_bounds__(256) void k_eg_update(EgP p)
{
    const EgCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= p.nkf) return;
    const int cur = c.cur;
    if (!c.fail)
        for (int a = 0; a < 7; a++) p.xv[(size_t)v * 7 + a] = v == p.fixed ? 0. : p.xt[(size_t)v * 7 + a];
    Sim3 S = p.est[cur][v];
    if (v != p.fixed) {
        double u[7];
        for (int a = 0; a < 7; a++) u[a] = p.xv[(size_t)v * 7 + a];
        if (p.fix_scale) u[6] = 0;
        S = mul(sim3_exp(u), S);
    }
    p.est[1 - cur][v] = S;
}

__global__ __launch_bounds__(256) void k_eg_trial_errors(EgP p)
{
    const EgCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.ne) return;
    double err[7], chi = 0;
    eg_error(p.meas[e], p.est[1 - c.cur][p.edge_i[e]], p.est[1 - c.cur][p.edge_j[e]], err);
    for (int k = 0; k < 7; k++) chi += err[k] * err[k];
    p.e_chi[e] = chi;
}

// OptimizationAlgorithmLevenberg::solve behind the trial's chi2: rho, accept or reject, lambda and nu, the end of the iteration
__global__ __launch_bounds__(LM_THREADS) void k_eg_ctl_trial(EgP p)
{
    __shared__ double red[LM_WAVES * 2];
    EgCtl& c = *p.ctl;
    if (c.aborted || !c.trial_go) return;
    // chi2 over the edges and x (lambda x + b) over the 7 nkf unknowns: each thread a contiguous run, then the workgroup
    const double lambda = c.lm.lambda;
    double s[2] = {run_sum(p.e_chi, p.ne), 0.};
    run_for(7 * p.nkf, [&](int j) { s[1] += p.xv[j] * (lambda * p.xv[j] + p.bv[j]); });
    block_sum<2>(s, red);
    if (threadIdx.x != 0) return;
    if (lm_judge_trial(c.lm, s[0], c.fail == 0, s[1])) c.cur = 1 - c.cur;
    c.trials++;
    c.fail = 0;
    const bool cont = lm_try_again(c.lm);
    c.trial_go = cont;
    if (cont) return;
    c.it++;
    const bool stop = lm_iteration_end(c.lm);
    c.iter_go = !stop && c.it < p.maxit;
}

// ---------------------------------------------------------------------------------------- the end --
__global__ __launch_bounds__(256) void k_eg_finish(EgP p)
{
    const EgCtl& c = *p.ctl;
    const int i = blockIdx.x * 256 + threadIdx.x, cur = c.cur;
    if (i == 0) {
        orbfe_eg_result r{};
        r.status = c.abort_status;
        if (!c.aborted) {
            r.iterations = c.it;
            r.trials = c.trials;
            r.chi2_first = c.chi_first;
            r.chi2_last = c.it ? c.lm.currentChi : 0.;
            r.lambda_last = c.lm.lambda;
        }
        *p.res = r;
    }
    if (c.aborted) return;
    if (i < p.nkf) {
        const Sim3 S = p.passthrough ? p.S0[i] : p.est[cur][i];
        if (p.Siw_out) sim_to8(S, p.Siw_out + (size_t)i * 8);
        if (p.passthrough) {
            for (int a = 0; a < 12; a++) p.Tcw_out[(size_t)i * 12 + a] = p.Tcw[(size_t)i * 12 + a];
        } else {
            // [sR t] -> [R t/s]: toRotationMatrix, eigt *= 1. / s, Converter::toCvSE3's casts
            double R[3][3];
            rot_of(S.q, R);
            const double is = 1. / S.s;
            for (int r = 0; r < 3; r++) {
                for (int cc = 0; cc < 3; cc++) p.Tcw_out[(size_t)i * 12 + r * 4 + cc] = (float)R[r][cc];
                p.Tcw_out[(size_t)i * 12 + r * 4 + 3] = (float)(S.t[r] * is);
            }
        }
    }
    if (i < p.np) {
        const int ref = p.pref[i];
        if (p.passthrough || ref < 0) {
            for (int a = 0; a < 3; a++) p.x3Dw_out[(size_t)i * 3 + a] = p.x3Dw[(size_t)i * 3 + a];
        } else {
            const double P[3] = {p.x3Dw[(size_t)i * 3], p.x3Dw[(size_t)i * 3 + 1], p.x3Dw[(size_t)i * 3 + 2]};
            double Pr[3], Pw[3];
            map(p.S0[ref], P, Pr);
            map(inverse(p.est[cur][ref]), Pr, Pw);
            for (int a = 0; a < 3; a++) p.x3Dw_out[(size_t)i * 3 + a] = (float)Pw[a];
        }
    }
}

// ---------------------------------------------------------------------------------------- host --
thread_local ThreadWorkspaces<TablesStage> tl_eg_tables;
thread_local ThreadWorkspaces<HostStage> tl_eg_stages;

struct EgCall {
    EgPlan plan;
    EgSchedule k;
    std::vector<int> level_rows;   // eg_level_lds_rows
    std::vector<unsigned char> blob;
    bool scratch_from_plan = false;   // the host calls: the scratch holds this plan's tables and fronts, not the bounds
};

// the scratch pointers and the tables of one call whose plan is made; p holds the caller's arrays and sizes already
int eg_prepare(EgCall& cl, EgP& p, const EgSizes& n, const int32_t* edge_i, const int32_t* edge_j, const int32_t* edge_kind, int iterations,
               int leaf_vertices, bool inspect, void* scratch, hipStream_t s)
{
    int rc;
    cl.k = eg_schedule(cl.plan, iterations, inspect, (size_t)max_lds());
    p.npairs = cl.plan.npairs;
    p.maxit = cl.k.iterations;
    p.passthrough = cl.plan.passthrough;
    const EgExtent x = eg_scratch(p, n, leaf_vertices, scratch, cl.scratch_from_plan ? &cl.plan : nullptr);
    cl.level_rows = eg_level_lds_rows(cl.plan, cl.k.lds_rows);
    eg_pack_tables(cl.blob, cl.plan, edge_i, edge_j, edge_kind);
    eg_tables(p, eg_counts(cl.plan), p.tables);
    ORBFE_HIP(hipMemsetAsync(scratch, 0, x.zero_end, s));
    ORBFE_HIP(hipMemsetAsync((unsigned char*)scratch + x.ff_begin, 0xff, x.ff_end - x.ff_begin, s));
    if ((rc = tl_eg_tables.get(s).send(cl.blob, p.tables, s))) return rc;
    return ensure_dyn_lds((const void*)k_eg_front, cl.k.tri_bytes);
}

int eg_enqueue_setup(const EgCall& cl, const EgP& p, hipStream_t s)
{
    hipLaunchKernelGGL(k_eg_setup, dim3(std::max(cl.k.g_setup, cl.k.g_finish)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_eg_init, dim3(cl.k.g_kf), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_eg_measure, dim3(cl.k.g_edges), dim3(256), 0, s, p);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int eg_enqueue_iteration(const EgCall& cl, const EgP& p, hipStream_t s, bool inspect)
{
    hipLaunchKernelGGL(k_eg_linearize, dim3(cl.k.g_lin), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_eg_blocks, dim3(cl.k.g_blocks), dim3(64), 0, s, p);
    hipLaunchKernelGGL(k_eg_ctl_lin, dim3(1), dim3(LM_THREADS), 0, s, p);
    for (int q = 0; q < cl.k.trials; q++) {
        front_enqueue_levels(k_eg_front, k_eg_back, cl.plan.level_off, cl.level_rows, LM_THREADS, p, s);
        hipLaunchKernelGGL(k_eg_update, dim3(cl.k.g_kf), dim3(256), 0, s, p);
        if (!inspect) {
            hipLaunchKernelGGL(k_eg_trial_errors, dim3(cl.k.g_edges), dim3(256), 0, s, p);
            hipLaunchKernelGGL(k_eg_ctl_trial, dim3(1), dim3(LM_THREADS), 0, s, p);
        }
    }
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int eg_enqueue_finish(const EgCall& cl, const EgP& p, hipStream_t s)
{
    hipLaunchKernelGGL(k_eg_finish, dim3(cl.k.g_finish), dim3(256), 0, s, p);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

struct EgHostArgs {
    const int32_t* kf_id; const float* Tcw; int nkf, fixed; const int32_t* corrected_pos; const double* corrected; int nc;
    const int32_t* noncorrected_pos; const double* noncorrected; int nn; const int32_t *edge_i, *edge_j, *edge_kind; int ne;
    const float* x3Dw; const int32_t* point_ref; int np, iterations, fix_scale, leaf_vertices;
};

// What both host calls do before they enqueue: the checks, on the host alone; then the device, the stage of this thread with the
// problem sent, the scratch, the plan
int eg_host_begin(EgCall& cl, EgP& p, HostStage*& w, EgHostIo& io, const EgHostArgs& a, bool inspect, int device, const char* name)
{
    const EgSizes n{a.nkf, a.ne, a.np, a.nc, a.nn};
    int rc;
    if ((rc = report(eg_check_sizes(n, a.fixed, a.iterations, a.leaf_vertices, name))) ||
        (rc = report(eg_check_edges(n, a.edge_i, a.edge_j, a.edge_kind, a.kf_id, name))) ||
        (rc = report(eg_check_values(n, a.Tcw, a.corrected_pos, a.corrected, a.noncorrected_pos, a.noncorrected, a.x3Dw, a.point_ref, name))))
        return rc;
    // the plan once here, before any device work, so that a graph whose fronts do not fit is refused with nothing touched
    if ((rc = report(eg_make_plan(cl.plan, n, a.fixed, a.edge_i, a.edge_j, a.leaf_vertices, name)))) return rc;
    if ((rc = use_device(device))) return rc;
    w = &tl_eg_stages.get();
    io = eg_host_io(n);
    if ((rc = w->begin(io.io))) return rc;
    w->put(io.Tcw, a.Tcw, (size_t)n.nkf * 48);
    w->put(io.cpos, a.corrected_pos, (size_t)n.nc * 4); w->put(io.csim, a.corrected, (size_t)n.nc * 64);
    w->put(io.npos, a.noncorrected_pos, (size_t)n.nn * 4); w->put(io.nsim, a.noncorrected, (size_t)n.nn * 64);
    w->put(io.X, a.x3Dw, (size_t)n.np * 12); w->put(io.pref, a.point_ref, (size_t)n.np * 4);
    if ((rc = w->upload())) return rc;
    p.Tcw = w->dev<const float>(io.Tcw); p.cpos = w->dev<const int32_t>(io.cpos); p.csim = w->dev<const double>(io.csim);
    p.npos = w->dev<const int32_t>(io.npos); p.nsim = w->dev<const double>(io.nsim); p.x3Dw = w->dev<const float>(io.X);
    p.pref = w->dev<const int32_t>(io.pref);
    p.Tcw_out = w->dev<float>(io.Tout); p.x3Dw_out = w->dev<float>(io.Xout); p.Siw_out = w->dev<double>(io.Siw);
    p.res = w->dev<orbfe_eg_result>(io.res);
    p.nkf = n.nkf; p.ne = n.ne; p.np = n.np; p.nc = n.nc; p.nn = n.nn; p.fixed = a.fixed; p.fix_scale = a.fix_scale != 0;
    cl.scratch_from_plan = true;
    if ((rc = w->host_scratch.ensure(eg_scratch_bytes(n, a.leaf_vertices, &cl.plan)))) return rc;
    return eg_prepare(cl, p, n, a.edge_i, a.edge_j, a.edge_kind, a.iterations, a.leaf_vertices, inspect, w->host_scratch.p, w->stream);
}

} // namespace
} // namespace orbfe

using namespace orbfe;

extern "C" size_t orbfe_essential_graph_scratch_bytes(int nkf, int nedges, int npoints, int leaf_vertices)
{
    const EgSizes n{nkf, nedges, npoints, 0, 0};
    if (nkf < 1 || nkf > EG_MAXKF || nedges < 0 || nedges > EG_MAXE || npoints < 0 || leaf_vertices < 0) return 0;
    return eg_scratch_bytes(n, leaf_vertices);
}

extern "C" int orbfe_optimize_essential_graph(const int32_t* kf_id, const float* Tcw, int nkf, int fixed, const int32_t* corrected_pos,
                                              const double* corrected, int nc, const int32_t* noncorrected_pos, const double* noncorrected, int nn,
                                              const int32_t* edge_i, const int32_t* edge_j, const int32_t* edge_kind, int ne, const float* x3Dw,
                                              const int32_t* point_ref, int np, int iterations, int fix_scale, int leaf_vertices, float* Tcw_out,
                                              float* x3Dw_out, double* Siw_out, orbfe_eg_result* res, int device)
{
    static const char* name = "orbfe_optimize_essential_graph";
    if (!res || !Tcw_out || (np > 0 && !x3Dw_out)) return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    const EgHostArgs a{kf_id, Tcw, nkf, fixed, corrected_pos, corrected, nc, noncorrected_pos, noncorrected, nn, edge_i, edge_j, edge_kind, ne,
                       x3Dw, point_ref, np, iterations, fix_scale, leaf_vertices};
    EgCall cl;
    EgP p{};
    HostStage* w = nullptr;
    EgHostIo io;
    int rc;
    if ((rc = eg_host_begin(cl, p, w, io, a, false, device, name)) || (rc = eg_enqueue_setup(cl, p, w->stream))) return rc;
    // an iteration at a time: the control block says whether another one is due.  What is enqueued is what the device call enqueues,
    // minus launches that would return at once, so the two calls give the same bits.
    EgCtl* hc = w->host<EgCtl>(io.ctl);
    for (int it = 0; it < cl.k.iterations; it++) {
        if ((rc = eg_enqueue_iteration(cl, p, w->stream, false))) return rc;
        ORBFE_HIP(hipMemcpyAsync(hc, p.ctl, sizeof(EgCtl), hipMemcpyDeviceToHost, w->stream));
        if ((rc = w->sync())) return rc;
        if (!hc->iter_go) break;
    }
    if ((rc = eg_enqueue_finish(cl, p, w->stream)) || (rc = w->download()) || (rc = w->sync())) return rc;
    const orbfe_eg_result r = *w->host<const orbfe_eg_result>(io.res);
    if (r.status < 0) return fail(r.status, "%s: the device refused the problem (status %d)", name, r.status);
    *res = r;
    w->get(Tcw_out, io.Tout, (size_t)nkf * 48);
    w->get(x3Dw_out, io.Xout, (size_t)np * 12);
    w->get(Siw_out, io.Siw, (size_t)nkf * 64);
    return ORBFE_OK;
}

extern "C" int orbfe_optimize_essential_graph_device(const int32_t* kf_id, const float* d_Tcw, int nkf, int fixed, const int32_t* d_corrected_pos,
                                                     const double* d_corrected, int nc, const int32_t* d_noncorrected_pos,
                                                     const double* d_noncorrected, int nn, const int32_t* edge_i, const int32_t* edge_j,
                                                     const int32_t* edge_kind, int ne, const float* d_x3Dw, const int32_t* d_point_ref, int np,
                                                     int iterations, int fix_scale, int leaf_vertices, float* d_Tcw_out, float* d_x3Dw_out,
                                                     double* d_Siw_out, orbfe_eg_result* d_res, void* d_scratch, size_t scratch_bytes, void* stream)
{
    static const char* name = "orbfe_optimize_essential_graph_device";
    const EgSizes n{nkf, ne, np, nc, nn};
    int rc;
    if ((rc = report(eg_check_sizes(n, fixed, iterations, leaf_vertices, name))) || (rc = report(eg_check_edges(n, edge_i, edge_j, edge_kind, kf_id, name))))
        return rc;
    if (!d_Tcw || !d_Tcw_out || !d_res || !d_scratch || ((uintptr_t)d_scratch & 255) || (nc && (!d_corrected_pos || !d_corrected)) ||
        (nn && (!d_noncorrected_pos || !d_noncorrected)) || (np && (!d_x3Dw || !d_point_ref || !d_x3Dw_out)))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    const size_t need = eg_scratch_bytes(n, leaf_vertices);
    if (scratch_bytes < need)
        return fail(ORBFE_ERR_CAPACITY, "%s: %zu bytes of scratch, orbfe_essential_graph_scratch_bytes asks for %zu", name, scratch_bytes, need);
    EgCall cl;
    EgP p{};
    p.Tcw = d_Tcw; p.cpos = d_corrected_pos; p.csim = d_corrected; p.npos = d_noncorrected_pos; p.nsim = d_noncorrected; p.x3Dw = d_x3Dw;
    p.pref = d_point_ref; p.Tcw_out = d_Tcw_out; p.x3Dw_out = d_x3Dw_out; p.Siw_out = d_Siw_out; p.res = d_res;
    p.nkf = nkf; p.ne = ne; p.np = np; p.nc = nc; p.nn = nn; p.fixed = fixed; p.fix_scale = fix_scale != 0;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = report(eg_make_plan(cl.plan, n, fixed, edge_i, edge_j, leaf_vertices, name))) ||
        (rc = eg_prepare(cl, p, n, edge_i, edge_j, edge_kind, iterations, leaf_vertices, false, d_scratch, s)) || (rc = eg_enqueue_setup(cl, p, s)))
        return rc;
    for (int it = 0; it < cl.k.iterations; it++)
        if ((rc = eg_enqueue_iteration(cl, p, s, false))) return rc;
    return eg_enqueue_finish(cl, p, s);
}

extern "C" int orbfe_essential_graph_inspect(const int32_t* kf_id, const float* Tcw, int nkf, int fixed, const int32_t* corrected_pos,
                                             const double* corrected, int nc, const int32_t* noncorrected_pos, const double* noncorrected, int nn,
                                             const int32_t* edge_i, const int32_t* edge_j, const int32_t* edge_kind, int ne, int fix_scale,
                                             int leaf_vertices, double* err, double* Ji, double* Jj, double* Hd, double* b, double* chi2, double* x,
                                             int32_t* tree, int device)
{
    static const char* name = "orbfe_essential_graph_inspect";
    if (!err || !Ji || !Jj || !Hd || !b || !chi2 || !x || !tree) return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    const EgHostArgs a{kf_id, Tcw, nkf, fixed, corrected_pos, corrected, nc, noncorrected_pos, noncorrected, nn, edge_i, edge_j, edge_kind, ne,
                       nullptr, nullptr, 0, 1, fix_scale, leaf_vertices};
    EgCall cl;
    EgP p{};
    HostStage* w = nullptr;
    EgHostIo io;
    int rc;
    if ((rc = eg_host_begin(cl, p, w, io, a, true, device, name)) || (rc = eg_enqueue_setup(cl, p, w->stream))) return rc;
    if (cl.k.iterations && (rc = eg_enqueue_iteration(cl, p, w->stream, true))) return rc;
    if ((rc = w->sync())) return rc;
    EgCtl c;
    ORBFE_HIP(hipMemcpy(&c, p.ctl, sizeof(c), hipMemcpyDeviceToHost));
    if (c.abort_status < 0) return fail(c.abort_status, "%s: the device refused the problem (status %d)", name, c.abort_status);
    chi2[0] = c.lm.currentChi;
    chi2[1] = c.lambda0;
    chi2[2] = cl.k.iterations && !c.fail ? 1. : 0.;
    memset(err, 0, (size_t)ne * 56); memset(Ji, 0, (size_t)ne * 392); memset(Jj, 0, (size_t)ne * 392);
    memset(Hd, 0, (size_t)nkf * 392); memset(b, 0, (size_t)nkf * 56); memset(x, 0, (size_t)nkf * 56);
    if (cl.k.iterations) {
        ORBFE_HIP(hipMemcpy(err, p.e_err, (size_t)ne * 56, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(Ji, p.Ji, (size_t)ne * 392, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(Jj, p.Jj, (size_t)ne * 392, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(Hd, p.Hd, (size_t)nkf * 392, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(b, p.bv, (size_t)nkf * 56, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(x, p.xv, (size_t)nkf * 56, hipMemcpyDeviceToHost));
    }
    // the plan: nodes, levels; per vertex its node and its place in the elimination order; per node parent, level, own, boundary
    const EgPlan& pl = cl.plan;
    int32_t* t = tree;
    *t++ = (int32_t)pl.nodes.size();
    *t++ = pl.nlevels;
    for (int v = 0; v < nkf; v++) *t++ = pl.node_of[(size_t)v];
    for (int v = 0; v < nkf; v++) *t++ = pl.order_of[(size_t)v];
    for (const EgNode& nd : pl.nodes) {
        *t++ = nd.parent; *t++ = nd.level; *t++ = nd.nown; *t++ = nd.nb;
    }
    return ORBFE_OK;
}
