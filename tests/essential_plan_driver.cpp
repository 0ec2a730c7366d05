// C entry points over csrc/essential_plan.hpp for tests/test_essential_plan_cpu.py (built with g++ by tests/essential_plan_build.py:
// the header has no HIP in it).  Test infrastructure only.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../orb_slam2_aruco_amd/csrc/essential_plan.hpp"

using namespace orbfe;

namespace {

int give(const BaCheck& c, char* msg, int msg_len)
{
    if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", c.msg);
    return c.err;
}

constexpr int N_SCRATCH = 18;

} // namespace

extern "C" {

// out: EG_MAXKF, EG_MAXE, EG_LEAF_DEFAULT, the front budget, EG_SIM3_BYTES, sizeof EgCtl, sizeof EgNode, sizeof EgSrc, sizeof the record
void eplan_constants(long long* out)
{
    const long long v[9] = {EG_MAXKF, EG_MAXE, EG_LEAF_DEFAULT, (long long)EG_FRONT_BUDGET, (long long)EG_SIM3_BYTES, (long long)sizeof(EgCtl),
                            (long long)sizeof(EgNode), (long long)sizeof(EgSrc), (long long)sizeof(orbfe_eg_result)};
    memcpy(out, v, sizeof v);
}

int eplan_check_sizes(const int* n, int fixed, int iterations, int leaf, char* msg, int msg_len)
{
    return give(eg_check_sizes(EgSizes{n[0], n[1], n[2], n[3], n[4]}, fixed, iterations, leaf, "call"), msg, msg_len);
}

int eplan_check_edges(const int* n, const int32_t* ei, const int32_t* ej, const int32_t* ek, const int32_t* kf_id, char* msg, int msg_len)
{
    return give(eg_check_edges(EgSizes{n[0], n[1], n[2], n[3], n[4]}, ei, ej, ek, kf_id, "call"), msg, msg_len);
}

int eplan_check_values(const int* n, const float* Tcw, const int32_t* cpos, const double* csim, const int32_t* npos, const double* nsim, const float* X,
                       const int32_t* pref, char* msg, int msg_len)
{
    return give(eg_check_values(EgSizes{n[0], n[1], n[2], n[3], n[4]}, Tcw, cpos, csim, npos, nsim, X, pref, "call"), msg, msg_len);
}

// The plan of a graph.  counts: nodes, levels, pairs, entries of node_vtx, of src, of cmap, the largest front's rows, doubles of all
// fronts.  node_of / order_of: nkf.  nodes: 8 a node (parent, level, own, boundary, offset in node_vtx, first child, second child,
// blocks), at most 2 nkf + 2.  node_vtx: at most vtx_cap.  front: a node's offset in doubles.  levels: level of every node in launch
// order (level_nodes), then the offsets.  Returns the error code.
int eplan_make(int nkf, int ne, int fixed, const int32_t* ei, const int32_t* ej, int leaf, long long* counts, int32_t* node_of, int32_t* order_of,
               int32_t* nodes, int32_t* node_vtx, int vtx_cap, long long* front, int32_t* level_nodes, int32_t* src, int32_t* cmap, char* msg, int msg_len)
{
    EgPlan p;
    const BaCheck c = eg_make_plan(p, EgSizes{nkf, ne, 0, 0, 0}, fixed, ei, ej, leaf, "call");
    if (c.err) return give(c, msg, msg_len);
    const long long v[8] = {(long long)p.nodes.size(), p.nlevels, p.npairs, (long long)p.node_vtx.size(), (long long)p.src.size(), (long long)p.cmap.size(),
                            p.max_rows, (long long)p.front_doubles};
    memcpy(counts, v, sizeof v);
    if ((int)p.node_vtx.size() > vtx_cap || (int)p.cmap.size() > vtx_cap) return -100;
    for (int k = 0; k < nkf; k++) {
        node_of[k] = p.node_of[(size_t)k];
        order_of[k] = p.order_of[(size_t)k];
    }
    for (size_t k = 0; k < p.nodes.size(); k++) {
        const EgNode& nd = p.nodes[k];
        const int32_t r[8] = {nd.parent, nd.level, nd.nown, nd.nb, nd.vtx, nd.child[0], nd.child[1], nd.nsrc};
        memcpy(nodes + 8 * k, r, sizeof r);
        front[k] = nd.front;
        level_nodes[k] = p.level_nodes[k];
    }
    for (size_t k = 0; k < p.node_vtx.size(); k++) node_vtx[k] = p.node_vtx[k];
    for (size_t k = 0; k < p.src.size(); k++) {
        const int32_t r[4] = {p.src[k].id, p.src[k].r, p.src[k].c, p.src[k].flags};
        memcpy(src + 4 * k, r, sizeof r);
    }
    for (size_t k = 0; k < p.cmap.size(); k++) cmap[k] = p.cmap[k];
    // the tables as they travel: the block the plan packs must fit what the scratch sets aside for it
    std::vector<unsigned char> blob;
    std::vector<int32_t> kind((size_t)std::max(ne, 1), 1);
    eg_pack_tables(blob, p, ei, ej, kind.data());
    EgTables t;
    if (blob.size() > eg_tables(t, eg_counts_cap(EgSizes{nkf, ne, 0, 0, 0}, leaf))) return -101;
    return 0;
}

// offsets of the scratch arrays in the order of EgLayout, then zero_end, ff_begin, ff_end, end; what orbfe_essential_graph_scratch_bytes
// returns; the bytes set aside for the tables and for the fronts
void eplan_scratch(const int* n, int leaf, unsigned long long* off, unsigned long long* ext, unsigned long long* sizes)
{
    const EgSizes s{n[0], n[1], n[2], n[3], n[4]};
    EgLayout l;
    const EgExtent x = eg_scratch(l, s, leaf);
    const size_t v[N_SCRATCH] = {l.ctl, l.xv, l.xt, l.kf_nc, l.kf_c, l.S0, l.est[0], l.est[1], l.meas, l.e_err, l.e_chi, l.Ji, l.Jj, l.Hd, l.bv, l.Hp, l.tables,
                                 l.fronts};
    for (int k = 0; k < N_SCRATCH; k++) off[k] = v[k];
    ext[0] = x.zero_end; ext[1] = x.ff_begin; ext[2] = x.ff_end; ext[3] = x.end;
    EgTables t;
    sizes[0] = eg_scratch_bytes(s, leaf);
    sizes[1] = eg_tables(t, eg_counts_cap(s, leaf));
    sizes[2] = eg_front_cap(s.nkf, leaf) * 8;
}

// launches of a call: the schedule's count and the levels, for a plan of this graph
int eplan_schedule(int nkf, int ne, int fixed, const int32_t* ei, const int32_t* ej, int leaf, int iterations, int inspect, long long lds_limit,
                   long long* out)
{
    EgPlan p;
    const BaCheck c = eg_make_plan(p, EgSizes{nkf, ne, 0, 0, 0}, fixed, ei, ej, leaf, "call");
    if (c.err) return c.err;
    const EgSchedule s = eg_schedule(p, iterations, inspect != 0, (size_t)lds_limit);
    const long long v[8] = {s.nlevels, s.back_levels, s.lds_rows, (long long)s.tri_bytes, s.iterations, s.trials, s.launches_trial, s.launches};
    memcpy(out, v, sizeof v);
    return 0;
}

} // extern "C"
