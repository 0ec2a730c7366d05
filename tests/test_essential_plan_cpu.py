"""CPU tests of csrc/essential_plan.hpp (the host plan of OptimizeEssentialGraph) through tests/essential_plan_driver.cpp: the
elimination plan against a brute-force symbolic elimination, the scratch layout, the schedule and the validation codes."""
import numpy as np
import pytest

import essential_cases as S
import essential_plan_build as B

INV, CAP = -1, -4
LEAVES = (1, 2, 4, 0)


def _graphs():
    rng = np.random.default_rng(5)
    out = {}
    for name in ("two", "chain3", "ring24_leaf2", "double_edge", "leaf_to_fixed", "fixed_middle", "far_edge", "isolated", "ring48"):
        pb = S.case(name)
        out[name] = (len(pb["Tcw"]), int(pb["fixed"]), pb["edge_i"], pb["edge_j"])
    n = 40                                              # a graph that is not temporal at all
    ei = rng.integers(0, n, 120); ej = (ei + 1 + rng.integers(0, n - 1, 120)) % n
    out["random40"] = (n, 17, ei.astype(np.int32), ej.astype(np.int32))
    out["complete9"] = (9, 0, np.array([i for i in range(9) for j in range(i)], np.int32), np.array([j for i in range(9) for j in range(i)], np.int32))
    out["no_free_edges"] = (5, 2, np.array([0, 1, 3, 4], np.int32), np.array([2, 2, 2, 2], np.int32))
    return out


GRAPHS = _graphs()


def _brute_boundaries(nkf, fixed, ei, ej, plan):
    """symbolic elimination in the plan's order, vertex by vertex with the fill it makes: a node's boundary is what the vertices of its
    subtree were joined to, beyond the subtree, when their turns came"""
    adj = {v: set() for v in range(nkf) if v != fixed}
    for i, j in zip(ei.tolist(), ej.tolist()):
        if i != fixed and j != fixed:
            adj[i].add(j); adj[j].add(i)
    order = sorted(adj, key=lambda v: plan["order_of"][v])
    touched = {k: set() for k in range(plan["nnodes"])}
    for v in order:
        nb = adj.pop(v)
        touched[int(plan["node_of"][v])] |= nb
        for a in nb:
            adj[a].discard(v)
            adj[a] |= nb - {a}
    out = {}

    def subtree(k):
        verts, seen = set(plan["own"][k]), set(touched[k])
        for c in plan["children"][k]:
            if c >= 0:
                v2, s2 = subtree(int(c))
                verts |= v2; seen |= s2
        out[k] = seen - verts
        return verts, seen

    for k in range(plan["nnodes"]):
        if plan["parent"][k] < 0:
            subtree(k)
    return out


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_plan_is_a_valid_elimination(name, leaf):
    nkf, fixed, ei, ej = GRAPHS[name]
    p = B.make(nkf, fixed, ei, ej, leaf)
    assert p["rc"] == 0
    free = [v for v in range(nkf) if v != fixed]
    # the permutation is a permutation; the fixed vertex is in no node
    assert sorted(p["order_of"][free].tolist()) == list(range(nkf - 1)) and p["order_of"][fixed] == -1 and p["node_of"][fixed] == -1
    assert sorted(v for o in p["own"] for v in o) == free
    lim = leaf or B.constants()["EG_LEAF_DEFAULT"]
    anc = []
    for k in range(p["nnodes"]):
        a, q = set(), int(p["parent"][k])
        while q >= 0:
            a.add(q); q = int(p["parent"][q])
        anc.append(a)
        kids = [int(c) for c in p["children"][k] if c >= 0]
        assert all(p["parent"][c] == k for c in kids)
        assert p["level"][k] == (1 + max(p["level"][c] for c in kids) if kids else 0)
        if not kids:
            assert 1 <= len(p["own"][k]) <= lim
        assert p["own"][k] == sorted(p["own"][k]) and all(p["node_of"][v] == k for v in p["own"][k])
        # own and boundary in elimination order, the boundary made of ancestors' vertices
        both = p["own"][k] + p["boundary"][k]
        assert [p["order_of"][v] for v in both] == sorted(p["order_of"][v] for v in both)
        assert all(int(p["node_of"][v]) in a for v in p["boundary"][k])
    assert sum(p["parent"] < 0) == (1 if free else 0)
    # no edge joins two subtrees except through an ancestor
    for i, j in zip(ei.tolist(), ej.tolist()):
        if i != fixed and j != fixed:
            a, b = int(p["node_of"][i]), int(p["node_of"][j])
            assert a == b or a in anc[b] or b in anc[a], (i, j)
    # each boundary is the brute-force one
    brute = _brute_boundaries(nkf, fixed, ei, ej, p)
    for k in range(p["nnodes"]):
        assert set(p["boundary"][k]) == brute[k], (k, p["boundary"][k], brute[k])
    # levels in launch order; fronts side by side; every block placed once in the lower triangle
    assert [p["level"][k] for k in p["level_nodes"]] == sorted(p["level"].tolist())
    end = 0
    for k in range(p["nnodes"]):
        m = 7 * (len(p["own"][k]) + len(p["boundary"][k]))
        assert p["front"][k] == end
        end += m * m + 2 * m
    assert end == p["front_doubles"] and p["max_rows"] == max(7 * (len(o) + len(b)) for o, b in zip(p["own"], p["boundary"]))
    pairs = {(min(i, j), max(i, j)) for i, j in zip(ei.tolist(), ej.tolist()) if i != fixed and j != fixed}
    assert p["npairs"] == len(pairs) and p["nsrc"] == len(free) + len(pairs) and int(p["node_nsrc"].sum()) == p["nsrc"]
    assert all(r >= c for _, r, c, _ in p["src"].tolist())
    # the scratch function covers the layout: the fronts and the tables of this plan fit what it sets aside
    _, ext, sizes = B.scratch((nkf, len(ei), 0, 0, 0), leaf)
    assert p["front_doubles"] * 8 <= sizes["fronts"] and ext["end"] == sizes["bytes"]


def test_default_leaf_and_single_front():
    nkf, fixed, ei, ej = GRAPHS["ring24_leaf2"]
    assert B.make(nkf, fixed, ei, ej, 0)["own"] == B.make(nkf, fixed, ei, ej, B.constants()["EG_LEAF_DEFAULT"])["own"]
    one = B.make(nkf, fixed, ei, ej, 23)
    assert one["nnodes"] == 1 and one["nlevels"] == 1 and one["boundary"] == [[]] and one["max_rows"] == 7 * 23
    deep = B.make(nkf, fixed, ei, ej, 2)
    assert deep["nlevels"] >= 3
    far = B.make(*GRAPHS["far_edge"], 2)
    assert far["front_doubles"] >= deep["front_doubles"]     # a far loop edge only enlarges separators


def test_scratch_layout_and_caps():
    c = B.constants()
    assert (c["EG_MAXKF"], c["EG_MAXE"], c["EG_LEAF_DEFAULT"], c["EG_SIM3_BYTES"], c["sizeof_ctl"], c["sizeof_node"], c["sizeof_src"], c["sizeof_result"]) == \
        (4096, 65536, 8, 64, 112, 56, 16, 40)
    for n in ((1, 0, 0, 0, 0), (2, 1, 0, 1, 1), (24, 72, 200, 4, 4), (48, 300, 200, 48, 48), (1000, 10000, 20000, 30, 30)):
        for leaf in LEAVES:
            off, ext, sizes = B.scratch(n, leaf)
            K, E = max(n[0], 1), max(n[1], 1)
            # what the kernels of essential_graph.hip index in each array, in bytes: the test's own statement
            need = dict(ctl=112, xv=K * 56, xt=K * 56, kf_nc=K * 4, kf_c=K * 4, S0=K * 64, est0=K * 64, est1=K * 64, meas=E * 64, e_err=E * 56, e_chi=E * 8,
                        Ji=E * 392, Jj=E * 392, Hd=K * 392, bv=K * 56, Hp=E * 392, tables=sizes["tables"], fronts=sizes["fronts"])
            names = list(B.SCRATCH)
            for a, b in zip(names, names[1:] + [None]):
                nxt = off[b] if b else ext["end"]
                assert off[a] % 256 == 0 and off[a] + need[a] <= nxt, (n, leaf, a)
            assert ext["zero_end"] == off["kf_nc"] == ext["ff_begin"] and ext["ff_end"] == off["S0"] and ext["end"] == sizes["bytes"]
    _, _, big = B.scratch((c["EG_MAXKF"], c["EG_MAXE"], 100000, c["EG_MAXKF"], c["EG_MAXKF"]), 0)
    assert big["bytes"] < 1e9 and big["fronts"] <= c["EG_FRONT_BUDGET"] + 8


def test_schedule_counts_launches_from_the_plan():
    nkf, fixed, ei, ej = GRAPHS["ring24_leaf2"]
    p = B.make(nkf, fixed, ei, ej, 2)
    s = B.schedule(nkf, fixed, ei, ej, 2)
    assert s["nlevels"] == p["nlevels"] and s["back_levels"] == p["nlevels"] - 1 and s["trials"] == 10 and s["iterations"] == 20
    assert s["launches_trial"] == 2 * p["nlevels"] - 1 + 3 and s["launches"] == 3 + 20 * (3 + 10 * s["launches_trial"]) + 1
    assert s["lds_rows"] == p["max_rows"] and s["tri_bytes"] == p["max_rows"] * (p["max_rows"] + 1) // 2 * 8
    small = B.schedule(nkf, fixed, ei, ej, 64, lds_limit=65536)
    assert small["lds_rows"] < 7 * 23 and small["lds_rows"] % 7 == 0 and small["tri_bytes"] + 1024 <= 65536
    i = B.schedule(nkf, fixed, ei, ej, 2, inspect=True)
    assert i["iterations"] == 1 and i["trials"] == 1 and i["launches"] == 3 + 3 + 2 * p["nlevels"] - 1 + 1
    assert B.schedule(3, 0, [], [], 0)["iterations"] == 0


def test_validation_codes():
    ok = (24, 72, 10, 4, 4)
    assert B.check_sizes(ok, 0)[0] == 0
    assert B.check_sizes((0, 0, 0, 0, 0), 0)[0] == INV and B.check_sizes((24, -1, 0, 0, 0), 0)[0] == INV
    rc, msg = B.check_sizes((4097, 0, 0, 0, 0), 0)
    assert rc == CAP and "ORBFE_EG_MAX_KEYFRAMES = 4096" in msg
    rc, msg = B.check_sizes((24, 65537, 0, 0, 0), 0)
    assert rc == CAP and "ORBFE_EG_MAX_EDGES = 65536" in msg
    assert B.check_sizes(ok, 24)[0] == INV and B.check_sizes(ok, -1)[0] == INV and "fixed" in B.check_sizes(ok, 24)[1]
    assert B.check_sizes(ok, 0, iterations=21)[0] == INV and B.check_sizes(ok, 0, leaf=-1)[0] == INV and B.check_sizes((24, 1, 0, 25, 0), 0)[0] == INV
    n = (4, 2, 0, 0, 0)
    assert B.check_edges(n, [1, 2], [0, 1], [1, 0])[0] == 0
    assert B.check_edges(n, None, [0, 1], [1, 0])[0] == INV
    assert B.check_edges(n, [1, 4], [0, 1], [1, 0])[0] == INV and B.check_edges(n, [1, 2], [0, -1], [1, 0])[0] == INV
    rc, msg = B.check_edges(n, [1, 2], [0, 2], [1, 0], kf_id=[10, 11, 12, 13])
    assert rc == INV and "keyframe 12 (position 2) with itself" in msg
    assert B.check_edges(n, [1, 2], [0, 1], [1, 2])[0] == INV
    T = np.tile(np.eye(3, 4, dtype=np.float32), (4, 1, 1)); sim = np.array([[0, 0, 0, 1, 0, 0, 0, 1.0]]); X = np.zeros((2, 3), np.float32)
    v = (4, 0, 2, 1, 1)
    assert B.check_values(v, T, [3], sim, [3], sim, X, [0, -1])[0] == 0
    assert B.check_values(v, None, [3], sim, [3], sim, X, [0, -1])[0] == INV and B.check_values(v, T, [3], sim, [3], sim, None, [0, -1])[0] == INV
    assert B.check_values(v, T, [4], sim, [3], sim, X, [0, -1])[0] == INV and B.check_values(v, T, [3], sim, [-1], sim, X, [0, -1])[0] == INV
    assert B.check_values(v, T, [3], sim, [3], sim, X, [0, 4])[0] == INV and B.check_values(v, T, [3], sim, [3], sim, X, [0, -2])[0] == INV
    bad = T.copy(); bad[2, 1, 3] = np.inf
    assert B.check_values(v, bad, [3], sim, [3], sim, X, [0, -1])[0] == INV
    for k, val in ((7, 0.0), (7, -2.0), (7, np.nan), (1, np.inf)):
        s = sim.copy(); s[0, k] = val
        assert B.check_values(v, T, [3], s, [3], sim, X, [0, -1])[0] == INV and B.check_values(v, T, [3], sim, [3], s, X, [0, -1])[0] == INV
    Xb = X.copy(); Xb[1, 2] = np.nan
    assert B.check_values(v, T, [3], sim, [3], sim, Xb, [0, -1])[0] == INV
    two = np.vstack([sim, sim])
    assert B.check_values((4, 0, 2, 2, 1), T, [3, 3], two, [3], sim, X, [0, -1])[0] == INV


def test_a_graph_too_dense_for_the_front_budget_is_a_capacity_error():
    """the complete graph on 1 200 vertices: one separator after another, 0.6 GB for the root's front alone"""
    n = 1200
    i, j = np.triu_indices(n, 1)
    keep = np.random.default_rng(2).permutation(len(i))[:65000]      # within ORBFE_EG_MAX_EDGES, still dense everywhere
    p = B.make(n, 0, i[keep].astype(np.int32), j[keep].astype(np.int32), 0)
    assert p["rc"] == CAP and "budget" in p["msg"]
