// front_plan.hpp -- the elimination plan the sparse solvers share (essential_plan.hpp: the pose graph, 7 rows a vertex; gba_plan.hpp:
// the reduced camera system of the map-wide bundle adjustment, 6 rows a vertex): a nested dissection on the caller's order, a tree of
// fronts.  Pure host arithmetic, no HIP.
//
// The free vertices keep the caller's order, which is temporal: edges are short except for loop edges.  A range of them longer than
// `leaf` is split at its middle; its separator is every vertex of the left half not yet in a separator that has an edge to such a
// vertex of the right half; both halves recurse.  A node of the tree owns its separator (a leaf: what is left of its range); leaves
// are eliminated first, then the separators bottom-up (by level, a node's level being one more than its highest child's).  Every edge
// joins two vertices of one node, or a vertex with one of an ancestor: the separator cuts every edge that crosses the middle, whatever
// the graph, and a far loop edge only enlarges a separator.  A node's boundary is the set of ancestor vertices that its own vertices'
// edges or its children's boundaries touch; its front is the dense symmetric matrix over (own, boundary), `rows` rows a vertex, both
// lists in elimination order.  Children are always (left, right).
//
// Vertices eliminated last: the free indices from `nsplit` on are not bisected.  They are the own vertices of one node above the
// tree of the others, and the adjacency that chooses the separators (adj_sep) leaves their edges out, so that a vertex joined to
// many others along the whole order (a marker seen along a trajectory) pulls nobody into a separator; their edges (in adj) still
// place their blocks in the fronts through the boundaries.
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include <algorithm>
#include <vector>

namespace orbfe {

// a node of the elimination tree, as the kernels read it
struct FrontNode {
    long long front;        // offset in doubles: the front (n x n, row-major, lower triangle in use), its right-hand side (n), a work vector (n)
    int parent, level, nown, nb;
    int vtx;                // offset in node_vtx: own vertices, then the boundary; caller's positions
    int src, nsrc;          // its blocks of the linearised system (FrontSrc)
    int child[2], cmap[2];  // left and right child (-1: none) and where each one's scatter map starts: for every boundary vertex of the
                            // child, its index in this node's (own, boundary) list
    int pad;
};
static_assert(sizeof(FrontNode) == 56, "the tables' layout pins this size");

struct FrontSrc {
    int id;                 // a vertex (its diagonal block and right-hand side) or a pair
    int r, c;               // the block's place in the front, r >= c
    int flags;              // 1: a pair; 2: the pair's block goes in transposed
};

struct FrontTree {
    int nlevels = 0, max_rows = 0, max_level_nodes = 0;
    std::vector<int> node_of, order_of;     // per vertex, caller's positions: its node and its place in the elimination order, -1 a fixed one
    std::vector<int> perm;                  // the free vertices in elimination order
    std::vector<FrontNode> nodes;
    std::vector<int> node_vtx, cmap, level_off, level_nodes;
    std::vector<FrontSrc> src;
};

namespace front_detail {

struct Builder {
    FrontTree& p;
    int leaf;
    const std::vector<std::vector<int>>& adj;   // over free indices: the edges that choose separators
    std::vector<char> assigned;
    std::vector<std::vector<int>> own;          // per node, free indices

    int new_node()
    {
        FrontNode nd{};
        nd.parent = -1;
        nd.child[0] = nd.child[1] = -1;
        p.nodes.push_back(nd);
        own.emplace_back();
        return (int)p.nodes.size() - 1;
    }
    // the node of the free indices [lo, hi), -1 when every one of them sits in a separator above
    int build(int lo, int hi)
    {
        bool any = false;
        for (int u = lo; u < hi && !any; u++) any = !assigned[(size_t)u];
        if (!any) return -1;
        if (hi - lo <= leaf) {
            const int id = new_node();
            for (int u = lo; u < hi; u++)
                if (!assigned[(size_t)u]) {
                    assigned[(size_t)u] = 1;
                    own[(size_t)id].push_back(u);
                }
            return id;
        }
        const int mid = lo + (hi - lo) / 2;
        std::vector<int> sep;
        for (int u = lo; u < mid; u++) {
            if (assigned[(size_t)u]) continue;
            for (int w : adj[(size_t)u])
                if (w >= mid && w < hi && !assigned[(size_t)w]) {
                    sep.push_back(u);
                    break;
                }
        }
        for (int u : sep) assigned[(size_t)u] = 1;
        const int l = build(lo, mid), r = build(mid, hi);
        if (sep.empty() && l < 0) return r;   // a node without own vertices joins two children, or is not made
        if (sep.empty() && r < 0) return l;
        const int id = new_node();
        own[(size_t)id] = sep;
        p.nodes[(size_t)id].child[0] = l;
        p.nodes[(size_t)id].child[1] = r;
        if (l >= 0) p.nodes[(size_t)l].parent = id;
        if (r >= 0) p.nodes[(size_t)r].parent = id;
        return id;
    }
    int level_of(int id)
    {
        int lv = 0;
        for (int k = 0; k < 2; k++)
            if (p.nodes[(size_t)id].child[k] >= 0) lv = std::max(lv, 1 + level_of(p.nodes[(size_t)id].child[k]));
        p.nodes[(size_t)id].level = lv;
        return lv;
    }
};

} // namespace front_detail

// The tree, the elimination order, the boundaries and the fronts' places.  K: the caller's positions (node_of, order_of); free_list:
// the position of every free index; adj_sep / adj: adjacency over free indices (see the head of this file; the same list twice when
// no vertex is eliminated last, nsplit = the number of free indices).  Returns the doubles of all fronts.
inline double front_build_tree(FrontTree& p, int K, const std::vector<int>& free_list, const std::vector<std::vector<int>>& adj_sep,
                               const std::vector<std::vector<int>>& adj, int nsplit, int leaf, int rows)
{
    const int nfree = (int)free_list.size();
    p.node_of.assign((size_t)K, -1);
    p.order_of.assign((size_t)K, -1);
    front_detail::Builder B{p, leaf, adj_sep, std::vector<char>((size_t)nfree, 0), {}};
    int root = B.build(0, nsplit);
    if (nsplit < nfree) {
        const int id = B.new_node();
        for (int u = nsplit; u < nfree; u++) B.own[(size_t)id].push_back(u);
        p.nodes[(size_t)id].child[0] = root;
        if (root >= 0) p.nodes[(size_t)root].parent = id;
        root = id;
    }
    const int nnodes = (int)p.nodes.size();
    if (root >= 0) p.nlevels = B.level_of(root) + 1;

    // levels, the elimination order
    p.level_off.assign((size_t)p.nlevels + 1, 0);
    for (const FrontNode& nd : p.nodes) p.level_off[(size_t)nd.level + 1]++;
    for (int l = 0; l < p.nlevels; l++) {
        p.max_level_nodes = std::max(p.max_level_nodes, p.level_off[(size_t)l + 1]);
        p.level_off[(size_t)l + 1] += p.level_off[(size_t)l];
    }
    p.level_nodes.assign((size_t)nnodes, 0);
    {
        std::vector<int> at(p.level_off.begin(), p.level_off.end() - 1);
        for (int id = 0; id < nnodes; id++) p.level_nodes[(size_t)at[(size_t)p.nodes[(size_t)id].level]++] = id;
    }
    for (int id : p.level_nodes)
        for (int u : B.own[(size_t)id]) {
            const int v = free_list[(size_t)u];
            p.node_of[(size_t)v] = id;
            p.order_of[(size_t)v] = (int)p.perm.size();
            p.perm.push_back(v);
        }

    // boundaries, bottom-up; the lists (own, boundary) of every node in elimination order
    std::vector<std::vector<int>> bnd((size_t)nnodes);
    for (int id : p.level_nodes) {
        std::vector<int>& b = bnd[(size_t)id];
        int last = -1;   // the place of this node's last own vertex; below a node without own vertices, of its subtree's last one
        for (int u : B.own[(size_t)id]) last = std::max(last, p.order_of[(size_t)free_list[(size_t)u]]);
        for (int u : B.own[(size_t)id])
            for (int w : adj[(size_t)u]) {
                const int v = free_list[(size_t)w];
                if (p.order_of[(size_t)v] > last) b.push_back(v);
            }
        for (int k = 0; k < 2; k++) {
            const int c = p.nodes[(size_t)id].child[k];
            if (c < 0) continue;
            for (int v : bnd[(size_t)c])
                if (p.node_of[(size_t)v] != id) b.push_back(v);
        }
        std::sort(b.begin(), b.end(), [&](int x, int y) { return p.order_of[(size_t)x] < p.order_of[(size_t)y]; });
        b.erase(std::unique(b.begin(), b.end()), b.end());
    }
    double total = 0;
    for (int id = 0; id < nnodes; id++) {
        FrontNode& nd = p.nodes[(size_t)id];
        nd.nown = (int)B.own[(size_t)id].size();
        nd.nb = (int)bnd[(size_t)id].size();
        nd.vtx = (int)p.node_vtx.size();
        for (int u : B.own[(size_t)id]) p.node_vtx.push_back(free_list[(size_t)u]);
        for (int v : bnd[(size_t)id]) p.node_vtx.push_back(v);
        const double m = (double)rows * (nd.nown + nd.nb);
        nd.front = (long long)total;
        total += m * m + 2 * m;
        p.max_rows = std::max(p.max_rows, (int)m);
    }
    return total;
}

// Every node's blocks: the diagonal blocks of its own vertices; the block of pair q = (pair_u[q], pair_v[q]), two different free
// vertices, in the node of whichever vertex goes first.  Then the children's scatter maps.  Returns 0, or -1 - q when pair q has no
// front that holds both its vertices, or -1 - npairs - c when a boundary vertex of node c is missing from its parent: the plan is
// wrong then.
inline long long front_place_blocks(FrontTree& p, int K, const std::vector<int>& pair_u, const std::vector<int>& pair_v)
{
    const int nnodes = (int)p.nodes.size(), npairs = (int)pair_u.size();
    std::vector<std::vector<FrontSrc>> srcs((size_t)nnodes);
    std::vector<int> pos((size_t)K, -1);
    for (int id = 0; id < nnodes; id++) {
        const FrontNode& nd = p.nodes[(size_t)id];
        for (int k = 0; k < nd.nown; k++) srcs[(size_t)id].push_back(FrontSrc{p.node_vtx[(size_t)nd.vtx + k], k, k, 0});
    }
    for (int q = 0; q < npairs; q++) {
        const int u = pair_u[(size_t)q], v = pair_v[(size_t)q];
        const int id = p.order_of[(size_t)u] < p.order_of[(size_t)v] ? p.node_of[(size_t)u] : p.node_of[(size_t)v];
        const FrontNode& nd = p.nodes[(size_t)id];
        int iu = -1, iv = -1;
        for (int k = 0; k < nd.nown + nd.nb; k++) {
            if (p.node_vtx[(size_t)nd.vtx + k] == u) iu = k;
            if (p.node_vtx[(size_t)nd.vtx + k] == v) iv = k;
        }
        if (iu < 0 || iv < 0) return -1 - (long long)q;
        srcs[(size_t)id].push_back(iu > iv ? FrontSrc{q, iu, iv, 1} : FrontSrc{q, iv, iu, 3});
    }
    for (int id = 0; id < nnodes; id++) {
        FrontNode& nd = p.nodes[(size_t)id];
        nd.src = (int)p.src.size();
        nd.nsrc = (int)srcs[(size_t)id].size();
        p.src.insert(p.src.end(), srcs[(size_t)id].begin(), srcs[(size_t)id].end());
        for (int k = 0; k < nd.nown + nd.nb; k++) pos[(size_t)p.node_vtx[(size_t)nd.vtx + k]] = k;
        for (int k = 0; k < 2; k++) {
            const int c = nd.child[k];
            nd.cmap[k] = (int)p.cmap.size();
            if (c < 0) continue;
            const FrontNode& ch = p.nodes[(size_t)c];
            for (int b = 0; b < ch.nb; b++) {
                const int at = pos[(size_t)p.node_vtx[(size_t)ch.vtx + ch.nown + b]];
                if (at < 0) return -1 - (long long)npairs - c;
                p.cmap.push_back(at);
            }
        }
        for (int k = 0; k < nd.nown + nd.nb; k++) pos[(size_t)p.node_vtx[(size_t)nd.vtx + k]] = -1;
    }
    return 0;
}

// A bound on the doubles of all fronts that holds for every graph of these sizes: a node of a range of r vertices under `anc`
// separator vertices of its ancestors has at most r + anc vertices in its front.
inline double front_bound(int r, int anc, int leaf, int rows)
{
    const double m = (double)rows * (r + anc);
    const double own = m * m + 2 * m;
    if (r <= leaf) return own;
    const int left = r / 2;
    return own + front_bound(left, anc, leaf, rows) + front_bound(r - left, anc + left, leaf, rows);
}

// The rows a front kernel reserves LDS for at each level: the largest front of the level that fits lds_rows (0: none does, the level
// runs in global memory).  A level of small fronts then shares a compute unit among several workgroups.
inline std::vector<int> front_level_lds_rows(const FrontTree& p, int rows, int lds_rows)
{
    std::vector<int> out((size_t)p.nlevels, 0);
    for (const FrontNode& nd : p.nodes) {
        const int m = rows * (nd.nown + nd.nb);
        if (m <= lds_rows) out[(size_t)nd.level] = std::max(out[(size_t)nd.level], m);
    }
    return out;
}

#ifdef __HIPCC__
// the launches of one solve: the front kernel once per level, leaves first, with the LDS of the level's largest front that fits
// (level_rows), then the back kernel once per level downwards from below the root's
template <class P>
void front_enqueue_levels(void (*front)(P, int, int), void (*back)(P, int), const std::vector<int>& level_off, const std::vector<int>& level_rows, int threads,
                          const P& p, hipStream_t s)
{
    const int nlevels = (int)level_off.size() - 1;
    auto grid = [&](int l) { return dim3(level_off[(size_t)l + 1] - level_off[(size_t)l]); };
    for (int l = 0; l < nlevels; l++) {
        const int rows = level_rows[(size_t)l];
        hipLaunchKernelGGL(front, grid(l), dim3(threads), (size_t)rows * (rows + 1) / 2 * 8, s, p, level_off[(size_t)l], rows);
    }
    for (int l = nlevels - 2; l >= 0; l--) hipLaunchKernelGGL(back, grid(l), dim3(threads), 0, s, p, level_off[(size_t)l]);
}
#endif

} // namespace orbfe
