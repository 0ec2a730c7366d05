// essential_plan.hpp -- what the entry points of OptimizeEssentialGraph (csrc/essential_graph.hip) decide before they launch.  The
// sparsity pattern of the pose graph is fixed for a call, so everything symbolic happens here, once, on the host: the validation, the
// free-vertex numbering, the elimination plan (nested dissection on the caller's order, a tree of fronts), the tables the kernels
// walk, the scratch layout and the launch schedule.  Pure host arithmetic, no HIP: tests/essential_plan_driver.cpp compiles this
// header with g++.
//
// The elimination plan.  The fixed vertex is no unknown.  The tree of fronts over the free vertices is front_plan.hpp's (which says
// how it is made), with 7 rows a vertex and no vertex held back for the root; the bundle adjustment of gba_plan.hpp shares it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"
#include "ba_camera.hpp"    // BaCheck, ba_fail
#include "front_plan.hpp"   // the elimination tree and its fronts
#include "host_stage.hpp"   // IoLayout
#include "lm_rules.hpp"     // LmState

namespace orbfe {

constexpr int EG_MAXKF = ORBFE_EG_MAX_KEYFRAMES, EG_MAXE = ORBFE_EG_MAX_EDGES;
constexpr int EG_LEAF_DEFAULT = 8;                       // leaf_vertices = 0
constexpr size_t EG_FRONT_BUDGET = (size_t)768 << 20;    // bytes of scratch the fronts of one call may take
constexpr size_t EG_SIM3_BYTES = 64;                     // sizeof(Sim3) of sim3_group.hpp, a device header; essential_graph.hip asserts it
constexpr size_t EG_SOLVE_LDS = 1024;                    // what k_eg_front holds in LDS beside a front, rounded up
constexpr int EG_ITERATIONS = 20, EG_TRIALS = 10;        // optimize(20); g2o's _maxTrialsAfterFailure
constexpr double EG_LAMBDA_INIT = 1e-16;                 // setUserLambdaInit

struct EgCtl {
    LmState lm;
    double lambda0, chi_first;
    int it, ok2, iter_go, trial_go, cur, fail, aborted, abort_status, bad, trials, pad0, pad1;
};
static_assert(sizeof(EgCtl) == 112, "the scratch layout pins this size");

struct EgSizes {
    int nkf, ne, np, nc, nn;   // keyframes, edges, points, entries of CorrectedSim3 and of NonCorrectedSim3
};

// a node of the elimination tree and a block's place in its front, as the kernels read them (front_plan.hpp)
using EgNode = FrontNode;
using EgSrc = FrontSrc;

inline int eg_leaf(int leaf_vertices) { return leaf_vertices > 0 ? leaf_vertices : EG_LEAF_DEFAULT; }

// ---------------------------------------------------------------------------------------- validation --
inline BaCheck eg_check_sizes(const EgSizes& n, int fixed, int iterations, int leaf_vertices, const char* name)
{
    if (n.nkf < 1 || n.ne < 0 || n.np < 0 || n.nc < 0 || n.nn < 0) return ba_fail(ORBFE_ERR_INVALID, "%s: a negative size, or no keyframe", name);
    if (n.nkf > EG_MAXKF) return ba_fail(ORBFE_ERR_CAPACITY, "%s: %d keyframes, at most ORBFE_EG_MAX_KEYFRAMES = %d", name, n.nkf, EG_MAXKF);
    if (n.ne > EG_MAXE) return ba_fail(ORBFE_ERR_CAPACITY, "%s: %d edges, at most ORBFE_EG_MAX_EDGES = %d", name, n.ne, EG_MAXE);
    if (n.nc > n.nkf || n.nn > n.nkf) return ba_fail(ORBFE_ERR_INVALID, "%s: more similarities than keyframes", name);
    if (fixed < 0 || fixed >= n.nkf) return ba_fail(ORBFE_ERR_INVALID, "%s: fixed = %d, outside [0, %d)", name, fixed, n.nkf);
    if (iterations < 0 || iterations > EG_ITERATIONS) return ba_fail(ORBFE_ERR_INVALID, "%s: iterations = %d, outside [0, %d]", name, iterations, EG_ITERATIONS);
    if (leaf_vertices < 0) return ba_fail(ORBFE_ERR_INVALID, "%s: leaf_vertices = %d", name, leaf_vertices);
    return BaCheck{};
}

// the graph: both calls have it on the host
inline BaCheck eg_check_edges(const EgSizes& n, const int32_t* edge_i, const int32_t* edge_j, const int32_t* edge_kind, const int32_t* kf_id,
                              const char* name)
{
    if (n.ne && (!edge_i || !edge_j || !edge_kind)) return ba_fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    for (int e = 0; e < n.ne; e++) {
        const int i = edge_i[e], j = edge_j[e];
        if (i < 0 || i >= n.nkf || j < 0 || j >= n.nkf)
            return ba_fail(ORBFE_ERR_INVALID, "%s: edge %d joins positions %d and %d of %d keyframes", name, e, i, j, n.nkf);
        if (i == j) return ba_fail(ORBFE_ERR_INVALID, "%s: edge %d joins keyframe %d (position %d) with itself", name, e, kf_id ? kf_id[i] : i, i);
        if (edge_kind[e] != 0 && edge_kind[e] != 1) return ba_fail(ORBFE_ERR_INVALID, "%s: edge %d has kind %d", name, e, edge_kind[e]);
    }
    return BaCheck{};
}

// a list of positions with its similarities (quaternion x y z w, t, s)
inline BaCheck eg_check_sims(int nkf, const int32_t* pos, const double* sim, int count, const char* what, const char* name)
{
    if (count && (!pos || !sim)) return ba_fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    std::vector<char> seen((size_t)nkf, 0);
    for (int k = 0; k < count; k++) {
        if (pos[k] < 0 || pos[k] >= nkf) return ba_fail(ORBFE_ERR_INVALID, "%s: %s_pos[%d] = %d, outside [0, %d)", name, what, k, pos[k], nkf);
        if (seen[(size_t)pos[k]]) return ba_fail(ORBFE_ERR_INVALID, "%s: %s_pos names position %d twice", name, what, pos[k]);
        seen[(size_t)pos[k]] = 1;
        for (int a = 0; a < 8; a++)
            if (!std::isfinite(sim[(size_t)k * 8 + a])) return ba_fail(ORBFE_ERR_INVALID, "%s: %s[%d] is not finite", name, what, k);
        if (!(sim[(size_t)k * 8 + 7] > 0)) return ba_fail(ORBFE_ERR_INVALID, "%s: %s[%d] has scale %g", name, what, k, sim[(size_t)k * 8 + 7]);
    }
    return BaCheck{};
}

// the values of the host call (the device call leaves them to k_eg_setup)
inline BaCheck eg_check_values(const EgSizes& n, const float* Tcw, const int32_t* corrected_pos, const double* corrected,
                               const int32_t* noncorrected_pos, const double* noncorrected, const float* x3Dw, const int32_t* point_ref, const char* name)
{
    if (!Tcw || (n.np && (!x3Dw || !point_ref))) return ba_fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    for (size_t i = 0; i < (size_t)n.nkf * 12; i++)
        if (!std::isfinite(Tcw[i])) return ba_fail(ORBFE_ERR_INVALID, "%s: the pose at position %d is not finite", name, (int)(i / 12));
    BaCheck c = eg_check_sims(n.nkf, corrected_pos, corrected, n.nc, "corrected", name);
    if (c.err) return c;
    c = eg_check_sims(n.nkf, noncorrected_pos, noncorrected, n.nn, "noncorrected", name);
    if (c.err) return c;
    for (int i = 0; i < n.np; i++) {
        if (point_ref[i] < -1 || point_ref[i] >= n.nkf) return ba_fail(ORBFE_ERR_INVALID, "%s: point_ref[%d] = %d, outside [-1, %d)", name, i, point_ref[i], n.nkf);
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(x3Dw[(size_t)i * 3 + a])) return ba_fail(ORBFE_ERR_INVALID, "%s: point %d is not finite", name, i);
    }
    return BaCheck{};
}

// ---------------------------------------------------------------------------------------- the elimination plan --
// A bound on the doubles of all fronts that holds for every graph of nfree free vertices, from the sizes alone (front_plan.hpp)
inline double eg_front_bound(int r, int anc, int leaf) { return front_bound(r, anc, leaf, 7); }

// doubles of the scratch set aside for fronts: the bound above where it is smaller than the budget
inline size_t eg_front_cap(int nkf, int leaf_vertices)
{
    const int nfree = std::max(nkf - 1, 0);
    const double bound = nfree ? eg_front_bound(nfree, 0, eg_leaf(leaf_vertices)) : 0.;
    return (size_t)std::min(bound, (double)(EG_FRONT_BUDGET / 8)) + 1;
}

// the tree, the order, the fronts and their blocks are front_plan.hpp's (7 rows a vertex, no vertex eliminated last)
struct EgPlan : FrontTree {
    EgSizes n{};
    int fixed = 0, nfree = 0, leaf = 0, npairs = 0;
    bool passthrough = false;               // nkf == 1 or ne == 0: the call returns its inputs
    std::vector<int> pair_u, pair_v, pair_off, pair_items;   // unique pairs of free vertices u < v; items: edge * 2 + (the edge's vertex 0 is v), edge order
    std::vector<int> vtx_off, vtx_items;                     // per vertex: edge * 2 + (the vertex is the edge's vertex 1), edge order; none for the fixed one
    size_t front_doubles = 0;
};

// The plan of one call.  edge_i / edge_j have passed eg_check_edges.  Returns ORBFE_ERR_CAPACITY when the fronts of this graph do not
// fit the scratch orbfe_essential_graph_scratch_bytes sets aside for them.
inline BaCheck eg_make_plan(EgPlan& p, const EgSizes& n, int fixed, const int32_t* edge_i, const int32_t* edge_j, int leaf_vertices, const char* name)
{
    p = EgPlan{};
    p.n = n;
    p.fixed = fixed;
    p.leaf = eg_leaf(leaf_vertices);
    p.nfree = n.nkf - 1;
    p.passthrough = n.nkf == 1 || n.ne == 0;
    const size_t K = (size_t)n.nkf;
    p.node_of.assign(K, -1);
    p.order_of.assign(K, -1);
    p.vtx_off.assign(K + 1, 0);
    p.pair_off.assign(1, 0);
    p.level_off.assign(1, 0);
    if (p.passthrough) return BaCheck{};

    std::vector<int> free_list, fidx(K, -1);
    for (int v = 0; v < n.nkf; v++)
        if (v != fixed) {
            fidx[(size_t)v] = (int)free_list.size();
            free_list.push_back(v);
        }
    std::vector<std::vector<int>> adj((size_t)p.nfree);
    for (int e = 0; e < n.ne; e++) {
        const int a = fidx[(size_t)edge_i[e]], b = fidx[(size_t)edge_j[e]];
        if (a < 0 || b < 0) continue;
        adj[(size_t)a].push_back(b);
        adj[(size_t)b].push_back(a);
    }
    const double total = front_build_tree(p, n.nkf, free_list, adj, adj, p.nfree, p.leaf, 7);
    if (total + 1 > (double)eg_front_cap(n.nkf, leaf_vertices))
        return ba_fail(ORBFE_ERR_CAPACITY, "%s: the fronts of this graph take %.0f MB of scratch, the budget is %zu MB", name, total * 8 / 1048576.,
                       EG_FRONT_BUDGET >> 20);
    p.front_doubles = (size_t)total;

    // the edges of every vertex and of every pair, in edge order
    for (int e = 0; e < n.ne; e++) {
        if (edge_i[e] != fixed) p.vtx_off[(size_t)edge_i[e] + 1]++;
        if (edge_j[e] != fixed) p.vtx_off[(size_t)edge_j[e] + 1]++;
    }
    for (size_t v = 0; v < K; v++) p.vtx_off[v + 1] += p.vtx_off[v];
    p.vtx_items.assign((size_t)p.vtx_off[K], 0);
    {
        std::vector<int> at(p.vtx_off.begin(), p.vtx_off.end() - 1);
        for (int e = 0; e < n.ne; e++) {
            if (edge_i[e] != fixed) p.vtx_items[(size_t)at[(size_t)edge_i[e]]++] = 2 * e;
            if (edge_j[e] != fixed) p.vtx_items[(size_t)at[(size_t)edge_j[e]]++] = 2 * e + 1;
        }
    }
    std::vector<int> pe;   // edges between free vertices, by (u, v, edge)
    for (int e = 0; e < n.ne; e++)
        if (edge_i[e] != fixed && edge_j[e] != fixed) pe.push_back(e);
    auto lo_of = [&](int e) { return std::min(edge_i[e], edge_j[e]); };
    auto hi_of = [&](int e) { return std::max(edge_i[e], edge_j[e]); };
    std::stable_sort(pe.begin(), pe.end(), [&](int a, int b) { return lo_of(a) != lo_of(b) ? lo_of(a) < lo_of(b) : hi_of(a) < hi_of(b); });
    for (size_t k = 0; k < pe.size(); k++) {
        const int e = pe[k];
        if (k == 0 || lo_of(e) != lo_of(pe[k - 1]) || hi_of(e) != hi_of(pe[k - 1])) {
            p.pair_u.push_back(lo_of(e));
            p.pair_v.push_back(hi_of(e));
            p.pair_off.push_back(p.pair_off.back());
        }
        p.pair_items.push_back(2 * e + (edge_i[e] == hi_of(e) ? 1 : 0));
        p.pair_off.back()++;
    }
    p.npairs = (int)p.pair_u.size();

    // every node's blocks and the children's scatter maps
    const long long lost = front_place_blocks(p, n.nkf, p.pair_u, p.pair_v);
    if (lost < 0 && -1 - lost < p.npairs)
        return ba_fail(ORBFE_ERR_INVALID, "%s: the elimination plan lost the pair (%d, %d)", name, p.pair_u[(size_t)(-1 - lost)], p.pair_v[(size_t)(-1 - lost)]);
    if (lost < 0) return ba_fail(ORBFE_ERR_INVALID, "%s: the elimination plan lost a boundary vertex of node %d", name, (int)(-1 - lost - p.npairs));
    return BaCheck{};
}

// ---------------------------------------------------------------------------------------- the tables and the scratch --
// what the plan sends to the device, one block: counts of the arrays
struct EgCounts {
    size_t nkf, ne, nnodes, nvtx, nsrc, ncmap, npairs, npair_items, nvtx_items;
};
inline EgCounts eg_counts(const EgPlan& p)
{
    return EgCounts{(size_t)p.n.nkf, (size_t)p.n.ne, p.nodes.size(), p.node_vtx.size(), p.src.size(), p.cmap.size(), (size_t)p.npairs,
                    p.pair_items.size(), p.vtx_items.size()};
}
// the most each can be for a problem of these sizes: a node of m vertices takes 49 m^2 doubles of the fronts at least
inline EgCounts eg_counts_cap(const EgSizes& n, int leaf_vertices)
{
    const size_t K = (size_t)std::max(n.nkf, 1), E = (size_t)std::max(n.ne, 0), V = eg_front_cap(n.nkf, leaf_vertices) / 49 + 2 * K + 2;
    return EgCounts{K, E, 2 * K + 2, V, K + E, V, E, E, 2 * E};
}

struct EgTables {
    size_t nodes, node_vtx, src, cmap, level_nodes, pair_u, pair_v, pair_off, pair_items, vtx_off, vtx_items, edge_i, edge_j, edge_kind;
};
struct EgTake {
    IoLayout o;
    unsigned char* base = nullptr;
    void operator()(size_t& f, size_t bytes) { f = o.take(bytes); }
    template <class T> void operator()(T*& f, size_t bytes) { f = (T*)(base + o.take(bytes)); }
};
// THE list of the tables; returns the bytes of the block
template <class A> size_t eg_tables(A& a, const EgCounts& c, void* base = nullptr)
{
    EgTake take;
    take.base = (unsigned char*)base;
    take(a.nodes, c.nnodes * sizeof(EgNode)); take(a.node_vtx, c.nvtx * 4); take(a.src, c.nsrc * sizeof(EgSrc)); take(a.cmap, c.ncmap * 4);
    take(a.level_nodes, c.nnodes * 4); take(a.pair_u, c.npairs * 4); take(a.pair_v, c.npairs * 4); take(a.pair_off, (c.npairs + 1) * 4);
    take(a.pair_items, c.npair_items * 4); take(a.vtx_off, (c.nkf + 1) * 4); take(a.vtx_items, c.nvtx_items * 4);
    take(a.edge_i, c.ne * 4); take(a.edge_j, c.ne * 4); take(a.edge_kind, c.ne * 4);
    return take.o.end();
}

// the block as bytes, laid out by eg_tables for the plan's own counts
inline void eg_pack_tables(std::vector<unsigned char>& blob, const EgPlan& p, const int32_t* edge_i, const int32_t* edge_j, const int32_t* edge_kind)
{
    EgTables t;
    const EgCounts c = eg_counts(p);
    blob.assign(eg_tables(t, c), 0);
    auto put = [&](size_t off, const void* src, size_t bytes) {
        if (bytes) memcpy(blob.data() + off, src, bytes);
    };
    put(t.nodes, p.nodes.data(), c.nnodes * sizeof(EgNode)); put(t.node_vtx, p.node_vtx.data(), c.nvtx * 4); put(t.src, p.src.data(), c.nsrc * sizeof(EgSrc));
    put(t.cmap, p.cmap.data(), c.ncmap * 4); put(t.level_nodes, p.level_nodes.data(), c.nnodes * 4); put(t.pair_u, p.pair_u.data(), c.npairs * 4);
    put(t.pair_v, p.pair_v.data(), c.npairs * 4); put(t.pair_off, p.pair_off.data(), p.pair_off.size() * 4); put(t.pair_items, p.pair_items.data(), c.npair_items * 4);
    put(t.vtx_off, p.vtx_off.data(), p.vtx_off.size() * 4); put(t.vtx_items, p.vtx_items.data(), c.nvtx_items * 4);
    put(t.edge_i, edge_i, c.ne * 4); put(t.edge_j, edge_j, c.ne * 4); put(t.edge_kind, edge_kind, c.ne * 4);
}

// the offsets of the scratch arrays, named as the kernels' argument (EgP of essential_graph.hip) names its pointers
struct EgLayout {
    size_t ctl, xv, xt, kf_nc, kf_c, S0, est[2], meas, e_err, e_chi, Ji, Jj, Hd, bv, Hp, tables, fronts;
};
struct EgExtent {
    size_t zero_end, ff_begin, ff_end, end;   // [0, zero_end) is zeroed and [ff_begin, ff_end) set to -1 at every call
};
// plan: the host call has made its plan before it asks for scratch and takes what that plan's tables and fronts need; the device call's
// scratch is sized by the caller from the sizes alone (plan = nullptr: the bounds)
template <class A> EgExtent eg_scratch(A& a, const EgSizes& n, int leaf_vertices, void* base = nullptr, const EgPlan* plan = nullptr)
{
    EgTake take;
    take.base = (unsigned char*)base;
    EgExtent x;
    const size_t K = (size_t)std::max(n.nkf, 1), E = (size_t)std::max(n.ne, 1);
    EgTables t;
    take(a.ctl, sizeof(EgCtl));
    take(a.xv, K * 56);                    // the update, 7 a vertex, caller's positions; it stays when a solve fails
    take(a.xt, K * 56);                    // the trial's solution, written front by front
    x.zero_end = take.o.end();
    x.ff_begin = take.o.end();
    take(a.kf_nc, K * 4);                  // the vertex's entry of NonCorrectedSim3 and of CorrectedSim3, -1 none
    take(a.kf_c, K * 4);
    x.ff_end = take.o.end();
    take(a.S0, K * EG_SIM3_BYTES);         // vScw
    for (int k = 0; k < 2; k++) take(a.est[k], K * EG_SIM3_BYTES);
    take(a.meas, E * EG_SIM3_BYTES);
    take(a.e_err, E * 56); take(a.e_chi, E * 8); take(a.Ji, E * 392); take(a.Jj, E * 392);
    take(a.Hd, K * 392); take(a.bv, K * 56); take(a.Hp, E * 392);
    take(a.tables, eg_tables(t, plan ? eg_counts(*plan) : eg_counts_cap(n, leaf_vertices)));
    take(a.fronts, (plan ? plan->front_doubles + 1 : eg_front_cap(n.nkf, leaf_vertices)) * 8);
    x.end = take.o.end();
    return x;
}

inline size_t eg_scratch_bytes(const EgSizes& n, int leaf_vertices, const EgPlan* plan = nullptr)
{
    EgLayout l;
    return eg_scratch(l, n, leaf_vertices, nullptr, plan).end;
}

// ---------------------------------------------------------------------------------------- the host call's staging block --
struct EgHostIo {
    IoLayout io;
    size_t Tcw, cpos, csim, npos, nsim, X, pref;   // inputs
    size_t Tout, Xout, Siw, res, ctl;              // outputs; ctl: where the host call reads the control block between iterations
};
inline EgHostIo eg_host_io(const EgSizes& n)
{
    const size_t K = (size_t)std::max(n.nkf, 1), P = (size_t)std::max(n.np, 1), C = (size_t)std::max(n.nc, 1), N = (size_t)std::max(n.nn, 1);
    EgHostIo l;
    IoLayout& o = l.io;
    l.Tcw = o.take(K * 48); l.cpos = o.take(C * 4); l.csim = o.take(C * 64); l.npos = o.take(N * 4); l.nsim = o.take(N * 64);
    l.X = o.take(P * 12); l.pref = o.take(P * 4);
    o.outputs();
    l.Tout = o.take(K * 48); l.Xout = o.take(P * 12); l.Siw = o.take(K * 64); l.res = o.take(sizeof(orbfe_eg_result)); l.ctl = o.take(sizeof(EgCtl));
    return l;
}

// ---------------------------------------------------------------------------------------- the launch schedule --
// setup (k_eg_setup, k_eg_init, k_eg_measure); an iteration: k_eg_linearize, k_eg_blocks, k_eg_ctl_lin and `trials` trials, each k_eg_front once
// per level upwards, k_eg_back once per level below the top downwards (a node without a boundary, the root among them, substitutes
// back inside k_eg_front), k_eg_update, k_eg_trial_errors, k_eg_ctl_trial; k_eg_finish after.  The number of launches is a function of
// the plan; an inspect call is setup, one iteration of one trial without k_eg_ctl_trial, and no finish.
struct EgSchedule {
    int g_kf;          // 256 threads over the keyframes
    int g_setup;       // k_eg_setup: over the longest of keyframes and similarities
    int g_lin;         // k_eg_linearize: 16 lanes an edge
    int g_edges;       // 256 threads over the edges
    int g_blocks;      // k_eg_blocks: a wave per vertex, then per pair
    int g_finish;      // k_eg_finish: over keyframes and points
    int nlevels, back_levels;
    int lds_rows;      // rows of a front k_eg_front factors in LDS at most; each level reserves what its own fronts need (eg_level_lds_rows)
    size_t tri_bytes;
    int iterations, trials;
    int launches_iteration, launches_trial, launches;
};
inline EgSchedule eg_schedule(const EgPlan& p, int iterations, bool inspect, size_t lds_limit)
{
    EgSchedule s;
    const EgSizes& n = p.n;
    s.g_kf = std::max((n.nkf + 255) / 256, 1);
    s.g_setup = std::max((std::max(n.nkf, std::max(n.nc, n.nn)) + 255) / 256, 1);
    s.g_lin = std::max((n.ne * 16 + 255) / 256, 1);
    s.g_edges = std::max((n.ne + 255) / 256, 1);
    s.g_blocks = std::max(n.nkf + p.npairs, 1);
    s.g_finish = std::max((std::max(n.nkf, n.np) + 255) / 256, 1);
    s.nlevels = p.nlevels;
    s.back_levels = std::max(p.nlevels - 1, 0);
    s.lds_rows = p.max_rows;
    while (s.lds_rows > 0 && (size_t)s.lds_rows * (s.lds_rows + 1) / 2 * 8 + EG_SOLVE_LDS > lds_limit) s.lds_rows -= 7;
    s.lds_rows = std::max(s.lds_rows, 0);
    s.tri_bytes = (size_t)s.lds_rows * (s.lds_rows + 1) / 2 * 8;
    s.iterations = p.passthrough ? 0 : inspect ? 1 : iterations;
    s.trials = inspect ? 1 : EG_TRIALS;
    s.launches_trial = s.nlevels + s.back_levels + (inspect ? 1 : 3);
    s.launches_iteration = 3 + s.trials * s.launches_trial;
    s.launches = 3 + s.iterations * s.launches_iteration + (inspect ? 0 : 1);
    return s;
}

// The rows k_eg_front reserves LDS for at each level (front_plan.hpp)
inline std::vector<int> eg_level_lds_rows(const EgPlan& p, int lds_rows) { return front_level_lds_rows(p, 7, lds_rows); }

} // namespace orbfe
