// C entry points over csrc/gba_plan.hpp for tests/test_gba_plan_cpu.py (built with g++ by tests/gba_plan_build.py: the header has no
// HIP in it), and with -DGBA_PLAN_MAIN a program of its own that walks the same rules on buffers of exactly their lengths, for a run
// under -fsanitize=address,undefined.  Test infrastructure only.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../orb_slam2_aruco_amd/csrc/gba_plan.hpp"

using namespace orbfe;

namespace {

int give(const BaCheck& c, char* msg, int msg_len)
{
    if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", c.msg);
    return c.err;
}

GbaProblem graph_of(const int* n, const uint8_t* fixed, const int32_t* off, const int32_t* okf, const int32_t* moff, const int32_t* mkf)
{
    return GbaProblem{{n[0], n[1], n[2], n[3], n[4]}, nullptr, fixed, nullptr, off, okf, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, moff, mkf, nullptr};
}

constexpr int N_SCRATCH = 29;
void scratch_offsets(const GbaLayout& l, size_t* v)
{
    const size_t o[N_SCRATCH] = {l.ctl, l.xv, l.xt, l.xl, l.pose[0], l.pose[1], l.pt[0], l.pt[1], l.e_pt, l.e_ox, l.e_oy, l.e_info, l.e_use, l.e_blk, l.m_use,
                                 l.m_blk, l.Hll, l.bl, l.Dinv, l.Hpp, l.bp, l.vmax, l.S, l.bs, l.chi_part, l.scale_part, l.max_part, l.tables, l.fronts};
    memcpy(v, o, sizeof o);
}

} // namespace

extern "C" {

// out: GBA_MAXV, GBA_MAX_OBS, GBA_LEAF_DEFAULT, the front budget, GBA_SE3_BYTES, sizeof GbaCtl, sizeof FrontNode, sizeof FrontSrc, sizeof the
// record, GBA_MAX_ITERATIONS, GBA_TRIALS
void gplan_constants(long long* out)
{
    const long long v[11] = {GBA_MAXV, GBA_MAX_OBS, GBA_LEAF_DEFAULT, (long long)GBA_FRONT_BUDGET, (long long)GBA_SE3_BYTES, (long long)sizeof(GbaCtl),
                             (long long)sizeof(FrontNode), (long long)sizeof(FrontSrc), (long long)sizeof(orbfe_gba_result), GBA_MAX_ITERATIONS, GBA_TRIALS};
    memcpy(out, v, sizeof v);
}

int gplan_check_sizes(const int* n, int iterations, int leaf, char* msg, int msg_len)
{
    return give(gba_check_sizes(GbaSizes{n[0], n[1], n[2], n[3], n[4]}, iterations, leaf, "call"), msg, msg_len);
}

int gplan_check_graph(const int* n, const uint8_t* fixed, const int32_t* off, const int32_t* okf, const int32_t* moff, const int32_t* mkf, char* msg, int msg_len)
{
    return give(gba_check_graph(graph_of(n, fixed, off, okf, moff, mkf), "call"), msg, msg_len);
}

// The plan of a graph.  counts: nv, free keyframes, pairs, point items, marker items, nodes, levels, entries of node_vtx, of src, of cmap,
// the largest front's rows, doubles of all fronts, points left out.  Per vertex (at most nkf + nma): v_kf, v_active, node_of, order_of,
// diag_pair, vtx_eoff (+ 1), vtx_moff (+ 1).  nodes: 8 a node (parent, level, own, boundary, offset in node_vtx, first child, second
// child, blocks).  Lists with their capacities in cap: vtx_eitems, vtx_mitems, pairs (u, v, off, moff: 4 a pair, and one more row of
// offsets), pair_items (2 an item), pair_mitems, node_vtx, src (4 a block), cmap.  Returns the error code, -100 when a list does not fit.
int gplan_make(const int* n, const uint8_t* fixed, const int32_t* off, const int32_t* okf, const int32_t* moff, const int32_t* mkf, int use_markers,
               int leaf, long long* counts, int32_t* vtx, int32_t* nodes, const long long* cap, int32_t* vtx_eitems, int32_t* vtx_mitems, int32_t* pairs,
               int32_t* pair_items, int32_t* pair_mitems, int32_t* node_vtx, int32_t* src, int32_t* cmap, int32_t* level_nodes, char* msg, int msg_len)
{
    GbaPlan p;
    const GbaProblem pb = graph_of(n, fixed, off, okf, moff, mkf);
    const BaCheck c = gba_make_plan(p, pb, use_markers, leaf, "call");
    if (c.err) return give(c, msg, msg_len);
    const long long v[13] = {p.nv, p.nfree_kf, p.npairs, (long long)p.pair_items.size() / 2, (long long)p.pair_mitems.size(), (long long)p.nodes.size(),
                             p.nlevels, (long long)p.node_vtx.size(), (long long)p.src.size(), (long long)p.cmap.size(), p.max_rows,
                             (long long)p.front_doubles, p.n_left_out};
    memcpy(counts, v, sizeof v);
    if ((long long)p.vtx_eitems.size() > cap[0] || (long long)p.vtx_mitems.size() > cap[1] || p.npairs > cap[2] || (long long)p.pair_items.size() > 2 * cap[3] ||
        (long long)p.pair_mitems.size() > cap[4] || (long long)p.node_vtx.size() > cap[5] || (long long)p.src.size() > cap[6] || (long long)p.cmap.size() > cap[7])
        return -100;
    const int V = n[0] + n[3];
    for (int k = 0; k < p.nv; k++) {
        vtx[k] = p.v_kf[(size_t)k]; vtx[V + k] = p.v_active[(size_t)k]; vtx[2 * V + k] = p.node_of[(size_t)k]; vtx[3 * V + k] = p.order_of[(size_t)k];
        vtx[4 * V + k] = p.diag_pair[(size_t)k];
    }
    for (int k = 0; k <= p.nv; k++) {
        vtx[5 * V + k] = p.vtx_eoff[(size_t)k];
        vtx[6 * V + 1 + k] = p.vtx_moff[(size_t)k];
    }
    for (size_t k = 0; k < p.nodes.size(); k++) {
        const FrontNode& nd = p.nodes[k];
        const int32_t r[8] = {nd.parent, nd.level, nd.nown, nd.nb, nd.vtx, nd.child[0], nd.child[1], nd.nsrc};
        memcpy(nodes + 8 * k, r, sizeof r);
        level_nodes[k] = p.level_nodes[k];
    }
    auto copy = [](int32_t* dst, const std::vector<int>& s) { if (!s.empty()) memcpy(dst, s.data(), s.size() * 4); };
    copy(vtx_eitems, p.vtx_eitems); copy(vtx_mitems, p.vtx_mitems); copy(pair_items, p.pair_items); copy(pair_mitems, p.pair_mitems);
    copy(node_vtx, p.node_vtx); copy(cmap, p.cmap);
    for (int q = 0; q <= p.npairs; q++) {
        if (q < p.npairs) { pairs[4 * q] = p.pair_u[(size_t)q]; pairs[4 * q + 1] = p.pair_v[(size_t)q]; }
        else pairs[4 * q] = pairs[4 * q + 1] = -1;
        pairs[4 * q + 2] = p.pair_off[(size_t)q]; pairs[4 * q + 3] = p.pair_moff[(size_t)q];
    }
    for (size_t k = 0; k < p.src.size(); k++) {
        const int32_t r[4] = {p.src[k].id, p.src[k].r, p.src[k].c, p.src[k].flags};
        memcpy(src + 4 * k, r, sizeof r);
    }
    // the tables as they travel: the block the plan packs must fit what the scratch sets aside for it from the sizes alone
    std::vector<unsigned char> blob;
    gba_pack_tables(blob, p, pb);
    GbaTables t;
    if (blob.size() > gba_tables(t, gba_counts_cap(pb.n, leaf))) return -101;
    if ((size_t)p.npairs + 1 > gba_pairs_cap(pb.n) || p.front_doubles + 1 > gba_front_cap(pb.n, leaf)) return -102;
    return 0;
}

// offsets of the scratch arrays in the order of GbaLayout, then zero_end, end; what orbfe_gba_scratch_bytes returns; the bytes set aside
// for the blocks of S, the tables and the fronts
void gplan_scratch(const int* n, int leaf, unsigned long long* off, unsigned long long* ext, unsigned long long* sizes)
{
    const GbaSizes s{n[0], n[1], n[2], n[3], n[4]};
    GbaLayout l;
    const GbaExtent x = gba_scratch(l, s, leaf);
    size_t v[N_SCRATCH];
    scratch_offsets(l, v);
    for (int k = 0; k < N_SCRATCH; k++) off[k] = v[k];
    ext[0] = x.zero_end; ext[1] = x.end;
    GbaTables t;
    sizes[0] = gba_scratch_bytes(s, leaf);
    sizes[1] = gba_pairs_cap(s) * 288;
    sizes[2] = gba_tables(t, gba_counts_cap(s, leaf));
    sizes[3] = gba_front_cap(s, leaf) * 8;
}

// launches of a call, for a plan of this graph: npb, nb, g_setup, g_pairs, nlevels, back_levels, lds_rows, tri_bytes, iterations, trials,
// launches_trial, launches_iteration, launches; then the bytes of scratch the host call takes for this plan
int gplan_schedule(const int* n, const uint8_t* fixed, const int32_t* off, const int32_t* okf, const int32_t* moff, const int32_t* mkf, int use_markers,
                   int leaf, int iterations, int inspect, long long lds_limit, long long* out)
{
    GbaPlan p;
    const BaCheck c = gba_make_plan(p, graph_of(n, fixed, off, okf, moff, mkf), use_markers, leaf, "call");
    if (c.err) return c.err;
    const GbaSchedule s = gba_schedule(p, iterations, inspect != 0, (size_t)lds_limit);
    const long long v[14] = {s.npb, s.nb, s.g_setup, s.g_pairs, s.nlevels, s.back_levels, s.lds_rows, (long long)s.tri_bytes, s.iterations, s.trials,
                             s.launches_trial, s.launches_iteration, s.launches, (long long)gba_scratch_bytes(p.n, leaf, &p)};
    memcpy(out, v, sizeof v);
    return 0;
}

} // extern "C"

#ifdef GBA_PLAN_MAIN
namespace {

long checked = 0;

// a chain: nkf keyframes (the first fixed), npts points each seen from `span` consecutive keyframes, nma markers each seen from three
// keyframes spread over the chain; every array allocated at exactly its length
struct Graph {
    std::vector<uint8_t> fixed;
    std::vector<int32_t> off, okf, moff, mkf;
    int n[5];
};
Graph chain(int nkf, int npts, int span, int nma)
{
    Graph g;
    g.fixed.assign((size_t)nkf, 0);
    if (nkf) g.fixed[0] = 1;
    g.off.push_back(0);
    for (int i = 0; i < npts; i++) {
        const int s = nkf > span ? (i * 7) % (nkf - span + 1) : 0;
        for (int k = 0; k < span && k < nkf; k++) g.okf.push_back(s + std::min(span, nkf) - 1 - k);   // not in keyframe order
        g.off.push_back((int32_t)g.okf.size());
    }
    g.moff.push_back(0);
    for (int m = 0; m < nma; m++) {
        for (int k = 0; k < 3 && nkf; k++) g.mkf.push_back((m + k * (nkf / 3)) % nkf);
        g.moff.push_back((int32_t)g.mkf.size());
    }
    const int n[5] = {nkf, npts, (int)g.okf.size(), nma, (int)g.mkf.size()};
    memcpy(g.n, n, sizeof n);
    return g;
}

template <class T> const T* ptr(const std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

bool walk(const Graph& g, int use_markers, int leaf)
{
    const GbaProblem pb = graph_of(g.n, ptr(g.fixed), ptr(g.off), ptr(g.okf), ptr(g.moff), ptr(g.mkf));
    BaCheck c = gba_check_graph(pb, "call");
    if (c.err) { printf("graph refused: %s\n", c.msg); return false; }
    GbaPlan p;
    c = gba_make_plan(p, pb, use_markers, leaf, "call");
    if (c.err) { printf("plan refused: %s\n", c.msg); return false; }
    checked++;
    // every off-diagonal pair's block sits in exactly one front, every diagonal one too
    std::vector<int> placed((size_t)p.npairs, 0);
    for (const FrontSrc& s : p.src) {
        if (s.id < 0 || s.id >= p.npairs || s.r < s.c) { printf("a block out of place\n"); return false; }
        placed[(size_t)s.id]++;
    }
    for (int q = 0; q < p.npairs; q++, checked++)
        if (placed[(size_t)q] != 1) { printf("pair %d placed %d times\n", q, placed[(size_t)q]); return false; }
    // the tables in a block of exactly their bytes, the scratch of the plan in a buffer of exactly its bytes
    std::vector<unsigned char> blob;
    gba_pack_tables(blob, p, pb);
    GbaTables t;
    if (blob.size() != gba_tables(t, gba_counts(p)) || blob.size() > gba_tables(t, gba_counts_cap(pb.n, leaf))) { printf("tables do not fit\n"); return false; }
    for (const GbaPlan* plan : {(const GbaPlan*)nullptr, (const GbaPlan*)&p}) {
        GbaLayout l;
        const GbaExtent x = gba_scratch(l, pb.n, leaf, nullptr, plan);
        size_t off[N_SCRATCH];
        scratch_offsets(l, off);
        std::vector<unsigned char> buf(x.end);
        for (int i = 0; i < N_SCRATCH; i++, checked++) {
            if (off[i] % 256 != 0 || (i && off[i] <= off[i - 1]) || off[i] >= x.end) { printf("scratch array %d misplaced\n", i); return false; }
            buf[off[i]] = (unsigned char)(i + 1);
        }
        if (l.fronts + (p.front_doubles + 1) * 8 > x.end || l.S + ((size_t)p.npairs + 1) * 288 > l.bs || l.tables + blob.size() > l.fronts) {
            printf("the plan does not fit its scratch\n");
            return false;
        }
        memcpy(buf.data() + l.tables, blob.data(), blob.size());
    }
    const GbaSchedule s = gba_schedule(p, 10, false, 160 * 1024);
    if (s.launches != 2 + 10 * (3 + 10 * (5 + s.nlevels + s.back_levels)) + 1) { printf("launch count\n"); return false; }
    checked++;
    return true;
}

} // namespace

int main()
{
    bool ok = true;
    ok = ok && walk(chain(0, 0, 3, 0), 1, 0);
    ok = ok && walk(chain(1, 0, 3, 0), 1, 0);
    ok = ok && walk(chain(2, 40, 2, 1), 1, 0);
    ok = ok && walk(chain(12, 400, 4, 0), 0, 2);
    ok = ok && walk(chain(12, 400, 4, 0), 0, 0);
    ok = ok && walk(chain(24, 300, 5, 3), 1, 2);
    ok = ok && walk(chain(24, 300, 5, 3), 0, 2);
    ok = ok && walk(chain(70, 300, 3, 2), 1, 4);
    ok = ok && walk(chain(40, 10, 40, 0), 1, 4096);
    // refused graphs
    {
        Graph g = chain(4, 5, 3, 0);
        g.okf[1] = g.okf[0];
        const BaCheck c = gba_check_graph(graph_of(g.n, ptr(g.fixed), ptr(g.off), ptr(g.okf), ptr(g.moff), ptr(g.mkf)), "call");
        ok = ok && c.err == ORBFE_ERR_INVALID && strstr(c.msg, "twice");
        checked++;
    }
    {
        Graph g = chain(4, 5, 3, 0);
        g.okf[2] = 4;
        const BaCheck c = gba_check_graph(graph_of(g.n, ptr(g.fixed), ptr(g.off), ptr(g.okf), ptr(g.moff), ptr(g.mkf)), "call");
        ok = ok && c.err == ORBFE_ERR_INVALID && strstr(c.msg, "names keyframe");
        checked++;
    }
    if (ok) printf("gba_plan: %ld checks ok\n", checked);
    return ok ? 0 : 1;
}
#endif
