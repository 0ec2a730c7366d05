// gba_plan.hpp -- what the entry points of the map-wide bundle adjustment (csrc/global_ba.hip) decide before they launch.  The graph
// of a call -- which keyframe sees which point and which marker -- is fixed and on the host, so everything symbolic happens here,
// once: the validation, the free-vertex numbering, the lists the kernels walk instead of a dense (keyframe, point) table (the edges of
// every vertex, the covisible pairs with their items: exactly the nonzero blocks of the reduced camera system S), the elimination
// tree of S (front_plan.hpp, 6 rows a vertex, the markers eliminated last), the scratch as one list, the staging block and the launch
// schedule.  Pure host arithmetic, no HIP: tests/gba_plan_driver.cpp compiles this header with g++.
//
// No list grows with nkf x np: a point of k observations from free keyframes gives k (k + 1) / 2 pair items, a marker observation 4.
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

constexpr int GBA_MAXV = ORBFE_GBA_MAX_POSES, GBA_MAX_OBS = ORBFE_GBA_MAX_OBSERVATIONS;
constexpr int GBA_MAX_ITERATIONS = 20, GBA_TRIALS = 10;  // the reference passes 10 or 20; g2o's _maxTrialsAfterFailure
constexpr int GBA_LEAF_DEFAULT = 8;                      // leaf_vertices = 0
constexpr size_t GBA_FRONT_BUDGET = (size_t)768 << 20;   // bytes of scratch the fronts of one call may take
constexpr int GBA_PT = 64;                               // threads of the per-point kernels: one wave
constexpr int GBA_MAX_LEVELS = BA_MAX_LEVELS;
constexpr int GBA_EBLK = 45;                             // doubles of a monocular edge's blocks: A = Jp^T w Jp (21), b (6), W = Jp^T w Jx (6 x 3)
constexpr int GBA_MBLK = 90;                             // of a marker edge: Acc (21), bc (6), Amm (21), bm (6), Acm (36)
constexpr size_t GBA_SE3_BYTES = 64;                     // sizeof(SE3) of se3_quat.hpp, a device header; global_ba.hip asserts it
constexpr size_t GBA_SOLVE_LDS = 1024;                   // what k_gba_front holds in LDS beside a front, rounded up

struct GbaCtl {
    LmState lm;
    double lambda0, chi_first;
    int it, fail, iter_go, trial_go, cur, aborted, abort_status, bad, trials, stopped, pad0, pad1;
};
static_assert(sizeof(GbaCtl) == 112, "the scratch layout pins this size");

struct GbaSizes {
    int nkf, np, nobs, nma, nmobs;
};

// The problem as the caller gives it.  The graph (kf_fixed, obs_offset, obs_kf, mobs_offset, mobs_kf) is on the host in every call;
// the values are host pointers or device pointers.  The observations are values (obs_xy, obs_octave) or, in the device call only,
// features of resident keypoint blocks (obs_feature, kps, capacity).
struct GbaProblem {
    GbaSizes n;
    float* Tcw; const uint8_t* kf_fixed; float* x3Dw; const int32_t* obs_offset; const int32_t* obs_kf; const float* obs_xy;
    const int32_t* obs_octave; const int32_t* obs_feature; const orbfe_keypoint* kps; int capacity;
    float* Twm; const float* marker_local; const int32_t* mobs_offset; const int32_t* mobs_kf; const float* mobs_corners;
};

inline int gba_leaf(int leaf_vertices) { return leaf_vertices > 0 ? leaf_vertices : GBA_LEAF_DEFAULT; }

// ---------------------------------------------------------------------------------------- validation --
inline BaCheck gba_check_sizes(const GbaSizes& n, int iterations, int leaf_vertices, const char* name)
{
    if (n.nkf < 0 || n.np < 0 || n.nobs < 0 || n.nma < 0 || n.nmobs < 0 || n.nmobs >= (1 << 24)) return ba_fail(ORBFE_ERR_INVALID, "%s: a size out of range", name);
    if ((long long)n.nkf + n.nma > GBA_MAXV)
        return ba_fail(ORBFE_ERR_CAPACITY, "%s: %d keyframes and %d markers, at most ORBFE_GBA_MAX_POSES = %d together", name, n.nkf, n.nma, GBA_MAXV);
    if (iterations < 1 || iterations > GBA_MAX_ITERATIONS) return ba_fail(ORBFE_ERR_INVALID, "%s: iterations = %d, outside [1, %d]", name, iterations, GBA_MAX_ITERATIONS);
    if (leaf_vertices < 0) return ba_fail(ORBFE_ERR_INVALID, "%s: leaf_vertices = %d", name, leaf_vertices);
    return BaCheck{};
}

// the graph: both calls have it on the host
inline BaCheck gba_check_graph(const GbaProblem& pb, const char* name)
{
    const int nkf = pb.n.nkf, np = pb.n.np, nobs = pb.n.nobs, nma = pb.n.nma, nmobs = pb.n.nmobs;
    if ((nkf && !pb.kf_fixed) || (np && !pb.obs_offset) || (nobs && (!pb.obs_kf || !np)) || (nma && !pb.mobs_offset) || (nmobs && (!pb.mobs_kf || !nma)))
        return ba_fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    const int32_t *off = pb.obs_offset, *moff = pb.mobs_offset;
    if (np && (off[0] != 0 || off[np] != nobs)) return ba_fail(ORBFE_ERR_INVALID, "%s: obs_offset does not span [0, nobs]", name);
    for (int i = 0; i < np; i++)
        if (off[i + 1] < off[i]) return ba_fail(ORBFE_ERR_INVALID, "%s: obs_offset decreases at point %d", name, i);
    if (nma && (moff[0] != 0 || moff[nma] != nmobs)) return ba_fail(ORBFE_ERR_INVALID, "%s: mobs_offset does not span [0, nmobs]", name);
    for (int i = 0; i < nma; i++)
        if (moff[i + 1] < moff[i]) return ba_fail(ORBFE_ERR_INVALID, "%s: mobs_offset decreases at marker %d", name, i);
    for (int e = 0; e < nobs; e++)
        if (pb.obs_kf[e] < 0 || pb.obs_kf[e] >= nkf)
            return ba_fail(ORBFE_ERR_INVALID, "%s: observation %d names keyframe %d of %d", name, e, pb.obs_kf[e], nkf);
    for (int e = 0; e < nmobs; e++)
        if (pb.mobs_kf[e] < 0 || pb.mobs_kf[e] >= nkf)
            return ba_fail(ORBFE_ERR_INVALID, "%s: marker observation %d names keyframe %d of %d", name, e, pb.mobs_kf[e], nkf);
    std::vector<int> seen((size_t)std::max(nkf, 1), -1);
    for (int i = 0; i < np; i++)
        for (int e = off[i]; e < off[i + 1]; e++) {
            if (seen[(size_t)pb.obs_kf[e]] == i) return ba_fail(ORBFE_ERR_INVALID, "%s: keyframe %d observes point %d twice", name, pb.obs_kf[e], i);
            seen[(size_t)pb.obs_kf[e]] = i;
        }
    for (int i = 0; i < np; i++)
        if (off[i + 1] - off[i] > GBA_MAX_OBS)
            return ba_fail(ORBFE_ERR_CAPACITY, "%s: point %d has %d observations, at most ORBFE_GBA_MAX_OBSERVATIONS = %d", name, i, off[i + 1] - off[i], GBA_MAX_OBS);
    return BaCheck{};
}

// the values of the host call (the device call leaves them to k_gba_setup)
inline BaCheck gba_check_values(const GbaProblem& pb, int nlevels, const char* name)
{
    const int nkf = pb.n.nkf, np = pb.n.np, nobs = pb.n.nobs, nma = pb.n.nma, nmobs = pb.n.nmobs;
    if ((nkf && !pb.Tcw) || (np && !pb.x3Dw) || (nobs && (!pb.obs_xy || !pb.obs_octave)) || (nma && (!pb.Twm || !pb.marker_local)) || (nmobs && !pb.mobs_corners))
        return ba_fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    auto fin = [](const float* v, size_t n) {
        for (size_t i = 0; i < n; i++)
            if (!std::isfinite(v[i])) return false;
        return true;
    };
    if (!fin(pb.Tcw, (size_t)nkf * 12) || !fin(pb.x3Dw, (size_t)np * 3) || !fin(pb.obs_xy, (size_t)nobs * 2) || !fin(pb.Twm, (size_t)nma * 12) ||
        !fin(pb.marker_local, (size_t)nma * 12) || !fin(pb.mobs_corners, (size_t)nmobs * 8))
        return ba_fail(ORBFE_ERR_INVALID, "%s: an input is not finite", name);
    for (int e = 0; e < nobs; e++)
        if (pb.obs_octave[e] < 0 || pb.obs_octave[e] >= nlevels)
            return ba_fail(ORBFE_ERR_INVALID, "%s: observation %d has octave %d, outside [0, %d)", name, e, pb.obs_octave[e], nlevels);
    return BaCheck{};
}

// the value pointers of the device call: which each observation form needs, the alignment of the scratch.  Nothing is read.
inline BaCheck gba_check_device(const GbaProblem& d, const void* d_res, const void* d_scratch, const char* name)
{
    const GbaSizes& n = d.n;
    const bool form_xy = d.obs_xy != nullptr;
    if (!d_res || !d_scratch || ((uintptr_t)d_scratch & 255) || (n.nkf && !d.Tcw) || (n.np && !d.x3Dw) || (n.nobs && form_xy && !d.obs_octave) ||
        (n.nobs && !form_xy && (!d.obs_feature || !d.kps || d.capacity <= 0)) || (n.nma && (!d.Twm || !d.marker_local)) || (n.nmobs && !d.mobs_corners))
        return ba_fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    return BaCheck{};
}

// ---------------------------------------------------------------------------------------- the plan --
struct GbaPlan : FrontTree {
    GbaSizes n{};
    int use_markers = 0, leaf = 0, nfree_kf = 0, nv = 0, npairs = 0, n_left_out = 0;
    std::vector<int> kf_free;                 // per keyframe: its free vertex, -1 a fixed one
    std::vector<int> v_kf;                    // per free vertex: its pose (a keyframe, or nkf + marker): free keyframes in order, then the markers
    std::vector<int> v_active;                // the vertex has an edge: one without is not part of the system
    std::vector<int> vtx_eoff, vtx_eitems;    // per free vertex: its monocular edges (observation slots) in point order
    std::vector<int> vtx_moff, vtx_mitems;    // per free vertex: its marker corner edges in edge order (a keyframe's, a marker's own)
    std::vector<int> pair_u, pair_v;          // the covisible pairs u <= v of free vertices, by (u, v): the nonzero blocks of S, diagonal ones included
    std::vector<int> pair_off, pair_items;    // per pair: (edge of u, edge of v) of every point both see, in point order
    std::vector<int> pair_moff, pair_mitems;  // per (keyframe, marker) pair: the corner edges between them, in edge order
    std::vector<int> diag_pair;               // per free vertex: the pair (v, v)
    std::vector<int> mo_marker;               // per marker observation: its marker
    size_t front_doubles = 0;
    long long items() const { return (long long)pair_items.size() / 2 + (long long)pair_mitems.size(); }
};

// bounds from the sizes alone, for the scratch of the device call
inline size_t gba_items_cap(const GbaSizes& n) { return (size_t)n.nobs * (size_t)(std::min(n.nkf, GBA_MAX_OBS) + 1) / 2 + 1; }
inline size_t gba_pairs_cap(const GbaSizes& n)
{
    const size_t V = (size_t)n.nkf + n.nma;
    return std::min(V * (V + 1) / 2, V + gba_items_cap(n) + (size_t)n.nmobs) + 1;
}
inline size_t gba_front_cap(const GbaSizes& n, int leaf_vertices)
{
    const double m = 6.0 * n.nma;
    const double bound = (n.nkf ? front_bound(n.nkf, n.nma, gba_leaf(leaf_vertices), 6) : 0.) + m * m + 2 * m;
    return (size_t)std::min(bound, (double)(GBA_FRONT_BUDGET / 8)) + 1;
}

// The plan of one call.  The graph has passed gba_check_graph.  Returns ORBFE_ERR_CAPACITY when the fronts of this covisibility
// graph do not fit the scratch orbfe_gba_scratch_bytes sets aside for them.
inline BaCheck gba_make_plan(GbaPlan& p, const GbaProblem& pb, int use_markers, int leaf_vertices, const char* name)
{
    p = GbaPlan{};
    const GbaSizes& n = pb.n;
    p.n = n;
    p.use_markers = use_markers != 0;
    p.leaf = gba_leaf(leaf_vertices);
    const int nma = p.use_markers ? n.nma : 0, nmobs = p.use_markers ? n.nmobs : 0;
    // 1. the free-vertex numbering: free keyframes in order, then the markers
    p.kf_free.assign((size_t)n.nkf, -1);
    for (int k = 0; k < n.nkf; k++)
        if (!pb.kf_fixed[k]) {
            p.kf_free[(size_t)k] = (int)p.v_kf.size();
            p.v_kf.push_back(k);
        }
    p.nfree_kf = (int)p.v_kf.size();
    for (int m = 0; m < nma; m++) p.v_kf.push_back(n.nkf + m);
    p.nv = (int)p.v_kf.size();
    const size_t V = (size_t)p.nv;
    p.mo_marker.assign((size_t)n.nmobs, 0);
    for (int m = 0; m < n.nma; m++)
        for (int o = pb.mobs_offset[m]; o < pb.mobs_offset[m + 1]; o++) p.mo_marker[(size_t)o] = m;
    for (int i = 0; i < n.np; i++) p.n_left_out += pb.obs_offset[i + 1] == pb.obs_offset[i];

    // 2. the edges of every vertex: a counting sort keeps slot order, which is point order
    p.vtx_eoff.assign(V + 1, 0);
    p.vtx_moff.assign(V + 1, 0);
    for (int e = 0; e < n.nobs; e++)
        if (p.kf_free[(size_t)pb.obs_kf[e]] >= 0) p.vtx_eoff[(size_t)p.kf_free[(size_t)pb.obs_kf[e]] + 1]++;
    for (int o = 0; o < nmobs; o++) {
        if (p.kf_free[(size_t)pb.mobs_kf[o]] >= 0) p.vtx_moff[(size_t)p.kf_free[(size_t)pb.mobs_kf[o]] + 1] += 4;
        p.vtx_moff[(size_t)(p.nfree_kf + p.mo_marker[(size_t)o]) + 1] += 4;
    }
    for (size_t v = 0; v < V; v++) {
        p.vtx_eoff[v + 1] += p.vtx_eoff[v];
        p.vtx_moff[v + 1] += p.vtx_moff[v];
    }
    p.vtx_eitems.assign((size_t)p.vtx_eoff[V], 0);
    p.vtx_mitems.assign((size_t)p.vtx_moff[V], 0);
    {
        std::vector<int> at(p.vtx_eoff.begin(), p.vtx_eoff.end() - 1), am(p.vtx_moff.begin(), p.vtx_moff.end() - 1);
        for (int e = 0; e < n.nobs; e++) {
            const int v = p.kf_free[(size_t)pb.obs_kf[e]];
            if (v >= 0) p.vtx_eitems[(size_t)at[(size_t)v]++] = e;
        }
        for (int j = 0; j < 4 * nmobs; j++) {
            const int v = p.kf_free[(size_t)pb.mobs_kf[j >> 2]], w = p.nfree_kf + p.mo_marker[(size_t)(j >> 2)];
            if (v >= 0) p.vtx_mitems[(size_t)am[(size_t)v]++] = j;
            p.vtx_mitems[(size_t)am[(size_t)w]++] = j;
        }
    }
    p.v_active.assign(V, 0);
    for (size_t v = 0; v < V; v++) p.v_active[v] = p.vtx_eoff[v + 1] > p.vtx_eoff[v] || p.vtx_moff[v + 1] > p.vtx_moff[v];

    // 3. the covisible pairs and their items
    struct Item {
        int u, v, a, b;
    };
    std::vector<Item> pit, mit;
    for (int i = 0; i < n.np; i++)
        for (int e = pb.obs_offset[i]; e < pb.obs_offset[i + 1]; e++) {
            const int ve = p.kf_free[(size_t)pb.obs_kf[e]];
            if (ve < 0) continue;
            for (int f = e; f < pb.obs_offset[i + 1]; f++) {
                const int vf = p.kf_free[(size_t)pb.obs_kf[f]];
                if (vf < 0) continue;
                pit.push_back(ve <= vf ? Item{ve, vf, e, f} : Item{vf, ve, f, e});
            }
        }
    for (int j = 0; j < 4 * nmobs; j++) {
        const int v = p.kf_free[(size_t)pb.mobs_kf[j >> 2]];
        if (v >= 0) mit.push_back(Item{v, p.nfree_kf + p.mo_marker[(size_t)(j >> 2)], j, j});
    }
    auto key = [V](int u, int v) { return (long long)u * (long long)(V + 1) + v; };
    std::vector<long long> keys;
    keys.reserve(V + pit.size() + mit.size());
    for (size_t v = 0; v < V; v++) keys.push_back(key((int)v, (int)v));
    for (const Item& t : pit) keys.push_back(key(t.u, t.v));
    for (const Item& t : mit) keys.push_back(key(t.u, t.v));
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    p.npairs = (int)keys.size();
    const size_t Q = keys.size();
    p.pair_u.resize(Q);
    p.pair_v.resize(Q);
    p.diag_pair.assign(V, -1);
    for (size_t q = 0; q < Q; q++) {
        p.pair_u[q] = (int)(keys[q] / (long long)(V + 1));
        p.pair_v[q] = (int)(keys[q] % (long long)(V + 1));
        if (p.pair_u[q] == p.pair_v[q]) p.diag_pair[(size_t)p.pair_u[q]] = (int)q;
    }
    auto pair_of = [&](int u, int v) { return (size_t)(std::lower_bound(keys.begin(), keys.end(), key(u, v)) - keys.begin()); };
    p.pair_off.assign(Q + 1, 0);
    p.pair_moff.assign(Q + 1, 0);
    std::vector<int> pq(pit.size()), mq(mit.size());
    for (size_t k = 0; k < pit.size(); k++) p.pair_off[(size_t)(pq[k] = (int)pair_of(pit[k].u, pit[k].v)) + 1]++;
    for (size_t k = 0; k < mit.size(); k++) p.pair_moff[(size_t)(mq[k] = (int)pair_of(mit[k].u, mit[k].v)) + 1]++;
    for (size_t q = 0; q < Q; q++) {
        p.pair_off[q + 1] += p.pair_off[q];
        p.pair_moff[q + 1] += p.pair_moff[q];
    }
    p.pair_items.assign(2 * pit.size(), 0);
    p.pair_mitems.assign(mit.size(), 0);
    {
        std::vector<int> at(p.pair_off.begin(), p.pair_off.end() - 1), am(p.pair_moff.begin(), p.pair_moff.end() - 1);
        for (size_t k = 0; k < pit.size(); k++) {
            const size_t s = (size_t)at[(size_t)pq[k]]++;
            p.pair_items[2 * s] = pit[k].a;
            p.pair_items[2 * s + 1] = pit[k].b;
        }
        for (size_t k = 0; k < mit.size(); k++) p.pair_mitems[(size_t)am[(size_t)mq[k]]++] = mit[k].a;
    }

    // 4. the elimination tree over the off-diagonal pairs; the pairs with a marker choose no separator
    std::vector<int> free_list(V), off_u, off_v, off_q;
    for (size_t v = 0; v < V; v++) free_list[v] = (int)v;
    std::vector<std::vector<int>> adj(V), adj_sep(V);
    for (size_t q = 0; q < Q; q++) {
        const int u = p.pair_u[q], v = p.pair_v[q];
        if (u == v) continue;
        off_u.push_back(u); off_v.push_back(v); off_q.push_back((int)q);
        adj[(size_t)u].push_back(v);
        adj[(size_t)v].push_back(u);
        if (v < p.nfree_kf) {
            adj_sep[(size_t)u].push_back(v);
            adj_sep[(size_t)v].push_back(u);
        }
    }
    const double total = front_build_tree(p, p.nv, free_list, adj_sep, adj, p.nfree_kf, p.leaf, 6);
    if (total + 1 > (double)gba_front_cap(n, leaf_vertices))
        return ba_fail(ORBFE_ERR_CAPACITY, "%s: the fronts of this covisibility graph take %.0f MB of scratch, the budget GBA_FRONT_BUDGET is %zu MB", name,
                       total * 8 / 1048576., GBA_FRONT_BUDGET >> 20);
    p.front_doubles = (size_t)total;
    if (front_place_blocks(p, p.nv, off_u, off_v) < 0) return ba_fail(ORBFE_ERR_INVALID, "%s: the elimination plan lost a block", name);
    // a block's id becomes its slot of S: the pair itself, or the diagonal pair of the vertex
    for (FrontSrc& s : p.src) s.id = (s.flags & 1) ? off_q[(size_t)s.id] : p.diag_pair[(size_t)s.id];
    return BaCheck{};
}

// ---------------------------------------------------------------------------------------- the tables and the scratch --
struct GbaCounts {
    size_t nkf, np, nobs, nma, nmobs, nv, nnodes, nvtx, nsrc, ncmap, npairs, nitems, nmitems, nvm;
};
inline GbaCounts gba_counts(const GbaPlan& p)
{
    return GbaCounts{(size_t)p.n.nkf, (size_t)p.n.np, (size_t)p.n.nobs, (size_t)p.n.nma, (size_t)p.n.nmobs, (size_t)p.nv, p.nodes.size(), p.node_vtx.size(),
                     p.src.size(), p.cmap.size(), (size_t)p.npairs, p.pair_items.size() / 2, p.pair_mitems.size(), p.vtx_mitems.size()};
}
// the most each can be for a problem of these sizes: a node of m vertices takes 36 m^2 doubles of the fronts at least
inline GbaCounts gba_counts_cap(const GbaSizes& n, int leaf_vertices)
{
    const size_t V = (size_t)n.nkf + n.nma, W = gba_front_cap(n, leaf_vertices) / 36 + 2 * V + 2, Q = gba_pairs_cap(n);
    return GbaCounts{(size_t)n.nkf, (size_t)n.np, (size_t)n.nobs, (size_t)n.nma, (size_t)n.nmobs, V, 2 * V + 3, W, Q, W, Q, gba_items_cap(n),
                     4 * (size_t)n.nmobs, 8 * (size_t)n.nmobs};
}

struct GbaTables {
    size_t nodes, node_vtx, src, cmap, level_nodes, kf_free, v_kf, v_active, diag_pair, vtx_eoff, vtx_eitems, vtx_moff, vtx_mitems, pair_u, pair_v, pair_off,
        pair_items, pair_moff, pair_mitems, obs_offset, obs_kf, mobs_offset, mobs_kf, mo_marker;
};
struct GbaTake {
    IoLayout o;
    unsigned char* base = nullptr;
    void operator()(size_t& f, size_t bytes) { f = o.take(bytes); }
    template <class T> void operator()(T*& f, size_t bytes) { f = (T*)(base + o.take(bytes)); }
};
// THE list of the tables; returns the bytes of the block
template <class A> size_t gba_tables(A& a, const GbaCounts& c, void* base = nullptr)
{
    GbaTake take;
    take.base = (unsigned char*)base;
    take(a.nodes, c.nnodes * sizeof(FrontNode)); take(a.node_vtx, c.nvtx * 4); take(a.src, c.nsrc * sizeof(FrontSrc)); take(a.cmap, c.ncmap * 4);
    take(a.level_nodes, c.nnodes * 4); take(a.kf_free, c.nkf * 4); take(a.v_kf, c.nv * 4); take(a.v_active, c.nv * 4); take(a.diag_pair, c.nv * 4);
    take(a.vtx_eoff, (c.nv + 1) * 4); take(a.vtx_eitems, c.nobs * 4); take(a.vtx_moff, (c.nv + 1) * 4); take(a.vtx_mitems, c.nvm * 4);
    take(a.pair_u, c.npairs * 4); take(a.pair_v, c.npairs * 4); take(a.pair_off, (c.npairs + 1) * 4); take(a.pair_items, c.nitems * 8);
    take(a.pair_moff, (c.npairs + 1) * 4); take(a.pair_mitems, c.nmitems * 4);
    take(a.obs_offset, (c.np + 1) * 4); take(a.obs_kf, c.nobs * 4); take(a.mobs_offset, (c.nma + 1) * 4); take(a.mobs_kf, c.nmobs * 4);
    take(a.mo_marker, c.nmobs * 4);
    return take.o.end();
}

// the block as bytes, laid out by gba_tables for the plan's own counts
inline void gba_pack_tables(std::vector<unsigned char>& blob, const GbaPlan& p, const GbaProblem& pb)
{
    GbaTables t;
    const GbaCounts c = gba_counts(p);
    blob.assign(gba_tables(t, c), 0);
    auto put = [&](size_t off, const void* src, size_t bytes) {
        if (bytes && src) memcpy(blob.data() + off, src, bytes);
    };
    auto vec = [&](size_t off, const std::vector<int>& v) { put(off, v.data(), v.size() * 4); };
    put(t.nodes, p.nodes.data(), c.nnodes * sizeof(FrontNode)); vec(t.node_vtx, p.node_vtx); put(t.src, p.src.data(), c.nsrc * sizeof(FrontSrc));
    vec(t.cmap, p.cmap); vec(t.level_nodes, p.level_nodes); vec(t.kf_free, p.kf_free); vec(t.v_kf, p.v_kf); vec(t.v_active, p.v_active);
    vec(t.diag_pair, p.diag_pair); vec(t.vtx_eoff, p.vtx_eoff); vec(t.vtx_eitems, p.vtx_eitems); vec(t.vtx_moff, p.vtx_moff); vec(t.vtx_mitems, p.vtx_mitems);
    vec(t.pair_u, p.pair_u); vec(t.pair_v, p.pair_v); vec(t.pair_off, p.pair_off); vec(t.pair_items, p.pair_items); vec(t.pair_moff, p.pair_moff);
    vec(t.pair_mitems, p.pair_mitems);
    if (c.np) put(t.obs_offset, pb.obs_offset, (c.np + 1) * 4);
    put(t.obs_kf, pb.obs_kf, c.nobs * 4);
    if (c.nma) put(t.mobs_offset, pb.mobs_offset, (c.nma + 1) * 4);
    put(t.mobs_kf, pb.mobs_kf, c.nmobs * 4);
    vec(t.mo_marker, p.mo_marker);
}

inline int gba_point_blocks(int np) { return (np + GBA_PT - 1) / GBA_PT; }              // workgroups of a pass over the points
inline int gba_marker_blocks(int nmobs) { return (4 * nmobs + GBA_PT - 1) / GBA_PT; }    // over the marker corner edges, 4 an observation

// the offsets of the scratch arrays, named as the kernels' argument (GbaP of global_ba.hip) names its pointers
struct GbaLayout {
    size_t ctl, xv, xt, xl, pose[2], pt[2], e_pt, e_ox, e_oy, e_info, e_use, e_blk, m_use, m_blk, Hll, bl, Dinv, Hpp, bp, vmax, S, bs, chi_part, scale_part,
        max_part, tables, fronts;
};
struct GbaExtent {
    size_t zero_end, end;   // [0, zero_end) is zeroed at every call
};
// THE list of the scratch arrays, in their order.  plan: the host call has made its plan before it asks for scratch and takes what
// that plan's tables, blocks and fronts need; the device call's scratch is sized by the caller from the sizes alone (nullptr: the bounds)
template <class A> GbaExtent gba_scratch(A& a, const GbaSizes& n, int leaf_vertices, void* base = nullptr, const GbaPlan* plan = nullptr)
{
    GbaTake take;
    take.base = (unsigned char*)base;
    GbaExtent x;
    const size_t K = (size_t)std::max(n.nkf, 1), P = (size_t)std::max(n.np, 1), E = (size_t)std::max(n.nobs, 1), M = (size_t)std::max(n.nma, 1),
                 ME = 4 * (size_t)std::max(n.nmobs, 1), V = K + M, NB = (size_t)std::max(gba_point_blocks(n.np) + gba_marker_blocks(n.nmobs), 1);
    GbaTables t;
    take(a.ctl, sizeof(GbaCtl));
    take(a.xv, V * 48);                    // the update of the last solved trial, 6 a free vertex
    take(a.xt, V * 48);                    // the trial's solution, written front by front
    take(a.xl, P * 24);
    x.zero_end = take.o.end();
    for (int k = 0; k < 2; k++) take(a.pose[k], (K + M) * GBA_SE3_BYTES);   // nkf keyframes, then nma markers
    for (int k = 0; k < 2; k++) take(a.pt[k], P * 24);
    take(a.e_pt, E * 4); take(a.e_ox, E * 4); take(a.e_oy, E * 4); take(a.e_info, E * 4);
    take(a.e_use, E);
    take(a.e_blk, E * GBA_EBLK * 8);
    take(a.m_use, ME);
    take(a.m_blk, ME * GBA_MBLK * 8);
    take(a.Hll, P * 48); take(a.bl, P * 24); take(a.Dinv, P * 72);
    take(a.Hpp, V * 288); take(a.bp, V * 48); take(a.vmax, V * 8);
    take(a.S, (plan ? (size_t)plan->npairs + 1 : gba_pairs_cap(n)) * 288);   // a 6 x 6 block per covisible pair
    take(a.bs, V * 48);
    take(a.chi_part, NB * 8); take(a.scale_part, NB * 8); take(a.max_part, NB * 8);
    take(a.tables, gba_tables(t, plan ? gba_counts(*plan) : gba_counts_cap(n, leaf_vertices)));
    take(a.fronts, (plan ? plan->front_doubles + 1 : gba_front_cap(n, leaf_vertices)) * 8);
    x.end = take.o.end();
    return x;
}

inline size_t gba_scratch_bytes(const GbaSizes& n, int leaf_vertices, const GbaPlan* plan = nullptr)
{
    GbaLayout l;
    return gba_scratch(l, n, leaf_vertices, nullptr, plan).end;
}

// ---------------------------------------------------------------------------------------- the host call's staging block --
struct GbaHostIo {
    IoLayout io;
    size_t xy, oct, mloc, mcor;   // inputs (the graph travels with the plan's tables)
    size_t T, X, M;               // in-out
    size_t res, ctl;              // outputs; ctl: where the host call reads the control block between iterations
};
inline GbaHostIo gba_host_io(const GbaSizes& n)
{
    const size_t K = (size_t)std::max(n.nkf, 1), P = (size_t)std::max(n.np, 1), E = (size_t)std::max(n.nobs, 1), M = (size_t)std::max(n.nma, 1),
                 MO = (size_t)std::max(n.nmobs, 1);
    GbaHostIo l;
    IoLayout& o = l.io;
    l.xy = o.take(E * 8); l.oct = o.take(E * 4); l.mloc = o.take(M * 48); l.mcor = o.take(MO * 32);
    o.inout();
    l.T = o.take(K * 48); l.X = o.take(P * 12); l.M = o.take(M * 48);
    o.outputs();
    l.res = o.take(sizeof(orbfe_gba_result)); l.ctl = o.take(sizeof(GbaCtl));
    return l;
}

// ---------------------------------------------------------------------------------------- the launch schedule --
// setup (k_gba_setup, k_gba_begin); an iteration: k_gba_linearize, k_gba_pose_blocks, k_gba_ctl_lin and `trials` trials, each
// k_gba_schur_points, k_gba_reduce, k_gba_front once per level upwards, k_gba_back once per level below the top downwards,
// k_gba_update, k_gba_backsub, k_gba_ctl_trial; k_gba_finish after.  The number of launches is a function of the plan; an inspect call
// is setup, one iteration of one trial without k_gba_ctl_trial, and no finish.
struct GbaSchedule {
    int npb, nb;       // workgroups of GBA_PT threads over the points; those and the ones over the marker corner edges (when in use)
    int g_setup;       // k_gba_setup, k_gba_finish: 256 threads over the longest of the caller's arrays
    int g_pass;        // k_gba_linearize, k_gba_backsub: nb
    int g_points;      // k_gba_schur_points: npb
    int g_vertices;    // k_gba_pose_blocks: a workgroup per free vertex
    int g_pairs;       // k_gba_reduce: a wave per covisible pair
    int g_update;      // k_gba_update: 256 threads over the free vertices
    int nlevels, back_levels;
    int lds_rows;      // rows of a front k_gba_front factors in LDS at most
    size_t tri_bytes;
    int iterations, trials;
    int launches_iteration, launches_trial, launches;
};
inline GbaSchedule gba_schedule(const GbaPlan& p, int iterations, bool inspect, size_t lds_limit)
{
    GbaSchedule s;
    const GbaSizes& n = p.n;
    s.npb = gba_point_blocks(n.np);
    s.nb = s.npb + (p.use_markers ? gba_marker_blocks(n.nmobs) : 0);
    s.g_setup = std::max((std::max(std::max(n.nobs, n.np), std::max(n.nkf + n.nma, n.nmobs)) + 255) / 256, 1);
    s.g_pass = std::max(s.nb, 1);
    s.g_points = std::max(s.npb, 1);
    s.g_vertices = std::max(p.nv, 1);
    s.g_pairs = std::max(p.npairs, 1);
    s.g_update = std::max((p.nv + 255) / 256, 1);
    s.nlevels = p.nlevels;
    s.back_levels = std::max(p.nlevels - 1, 0);
    s.lds_rows = p.max_rows;
    while (s.lds_rows > 0 && (size_t)s.lds_rows * (s.lds_rows + 1) / 2 * 8 + GBA_SOLVE_LDS > lds_limit) s.lds_rows -= 6;
    s.lds_rows = std::max(s.lds_rows, 0);
    s.tri_bytes = (size_t)s.lds_rows * (s.lds_rows + 1) / 2 * 8;
    s.iterations = inspect ? 1 : iterations;
    s.trials = inspect ? 1 : GBA_TRIALS;
    s.launches_trial = 2 + s.nlevels + s.back_levels + (inspect ? 2 : 3);
    s.launches_iteration = 3 + s.trials * s.launches_trial;
    s.launches = 2 + s.iterations * s.launches_iteration + (inspect ? 0 : 1);
    return s;
}

} // namespace orbfe
