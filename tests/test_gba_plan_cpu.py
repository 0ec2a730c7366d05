"""CPU tests of csrc/gba_plan.hpp through tests/gba_plan_driver.cpp: the lists the kernels of the map-wide bundle adjustment walk
(the edges of every vertex, the covisible pairs with their items) against a brute-force count in Python, the elimination tree (every
pair in one front, the markers at the root and in nobody's separator), the bounds, the scratch and the launch counts pinned as
literals, and the one structural performance condition: the plan's item count grows with the observations, not with nkf x np."""
import subprocess

import numpy as np
import pytest

import gba_cases as S
import gba_plan_build as PB

OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -4


def test_constants():
    assert PB.constants() == dict(GBA_MAXV=4096, GBA_MAX_OBS=256, GBA_LEAF_DEFAULT=8, GBA_FRONT_BUDGET=768 << 20, GBA_SE3_BYTES=64, sizeof_ctl=112,
                                  sizeof_node=56, sizeof_src=16, sizeof_result=48, GBA_MAX_ITERATIONS=20, GBA_TRIALS=10)


def _brute(pb):
    """free-vertex numbering, the edges of every vertex and the items of every pair, counted the slow way"""
    um = pb["use_markers"]
    free = [k for k in range(len(pb["kf_fixed"])) if not pb["kf_fixed"][k]]
    nma = len(pb["Twm"]) if um else 0
    v_kf = free + [len(pb["kf_fixed"]) + m for m in range(nma)]
    vof = {k: v for v, k in enumerate(free)}
    edges = [[e for e in range(len(pb["obs_kf"])) if pb["obs_kf"][e] == k] for k in free] + [[] for _ in range(nma)]
    medges = [[] for _ in v_kf]
    items, mitems = {}, {}
    for v in range(len(v_kf)):
        items[(v, v)], mitems[(v, v)] = [], []
    off = pb["obs_offset"]
    for i in range(len(pb["x3Dw"])):
        obs = [(vof[pb["obs_kf"][e]], e) for e in range(off[i], off[i + 1]) if pb["obs_kf"][e] in vof]
        for a, (va, ea) in enumerate(obs):
            for vb, eb in obs[a:]:
                key, it = ((va, vb), [ea, eb]) if va <= vb else ((vb, va), [eb, ea])
                items.setdefault(key, []).append(it)
                mitems.setdefault(key, [])
    moff = pb["mobs_offset"]
    for m in range(nma):
        for o in range(moff[m], moff[m + 1]):
            for j in range(4 * o, 4 * o + 4):
                medges[len(free) + m].append(j)
                if pb["mobs_kf"][o] in vof:
                    v = vof[pb["mobs_kf"][o]]
                    medges[v].append(j)
                    items.setdefault((v, len(free) + m), [])
                    mitems.setdefault((v, len(free) + m), []).append(j)
    for v in range(len(free)):
        medges[v].sort()
    return v_kf, edges, medges, items, mitems


@pytest.mark.parametrize("name", ["chain12_p400", "ring24_p600_m3_out_r1", "orphans", "orphans_markers_unused"])
def test_lists_match_a_brute_force_count(name):
    pb = S.case(name)
    p = PB.make(pb)
    assert p["rc"] == 0
    v_kf, edges, medges, items, mitems = _brute(pb)
    assert p["v_kf"].tolist() == v_kf and p["nv"] == len(v_kf) and p["nfree_kf"] == int((pb["kf_fixed"] == 0).sum())
    assert p["vtx_edges"] == edges and p["vtx_medges"] == medges
    assert p["v_active"].tolist() == [int(bool(e or m)) for e, m in zip(edges, medges)]
    pairs = sorted(items)
    assert list(zip(p["pair_u"].tolist(), p["pair_v"].tolist())) == pairs
    assert p["pair_items"] == [items[q] for q in pairs] and p["pair_mitems"] == [mitems[q] for q in pairs]
    assert p["diag_pair"].tolist() == [pairs.index((v, v)) for v in range(len(v_kf))]
    assert p["n_left_out"] == int((np.diff(pb["obs_offset"]) == 0).sum())
    if name == "orphans":
        assert p["v_active"].tolist() == [1, 1, 0, 1, 1, 1, 1, 0] and p["n_left_out"] == 1


@pytest.mark.parametrize("name", ["chain12_p400_leaf2", "chain12_p400", "ring24_p600_m3_out_r1", "k70_p300", "orphans", "init2_p120_m1_r1", "dense8_p200"])
def test_every_pair_meets_in_one_front_and_every_block_is_placed_once(name):
    pb = S.case(name)
    p = PB.make(pb)
    assert p["rc"] == 0 and sorted(p["order_of"].tolist()) == list(range(p["nv"]))
    front = [set(o) | set(b) for o, b in zip(p["own"], p["boundary"])]
    for u, v in zip(p["pair_u"], p["pair_v"]):
        first = u if p["order_of"][u] < p["order_of"][v] else v
        assert {u, v} <= front[p["node_of"][first]], (u, v)
    # a node's boundary lies in its parent's front; own vertices partition the free vertices
    for k in range(p["nnodes"]):
        if p["parent"][k] >= 0:
            assert set(p["boundary"][k]) <= front[p["parent"][k]]
        else:
            assert p["boundary"][k] == []
    assert sorted(v for o in p["own"] for v in o) == list(range(p["nv"]))
    assert sorted(p["src"][:, 0].tolist()) == list(range(p["npairs"])) and (p["src"][:, 1] >= p["src"][:, 2]).all()
    assert p["front_doubles"] == sum((6 * (len(o) + len(b))) ** 2 + 12 * (len(o) + len(b)) for o, b in zip(p["own"], p["boundary"]))


@pytest.mark.parametrize("name", ["ring24_p600_m3_out_r1", "orphans", "init2_p120_m1_r1"])
def test_markers_sit_at_the_root_and_pull_no_keyframe_into_a_separator(name):
    """the keyframes' tree is the tree of the same graph without markers, node for node; the markers are the own vertices of one more
    node above it"""
    pb = S.case(name)
    p, q = PB.make(pb), PB.make(pb, use_markers=0)
    nf = p["nfree_kf"]
    root = int(np.flatnonzero(p["parent"] == -1)[0])
    assert p["own"][root] == list(range(nf, p["nv"])) and p["nnodes"] == q["nnodes"] + 1
    assert p["own"][:q["nnodes"]] == q["own"] and np.array_equal(p["parent"][:q["nnodes"]][q["parent"] >= 0], q["parent"][q["parent"] >= 0])
    # a marker is in the boundary of a node only where a keyframe below sees it
    seen = {nf + m: {int(k) for k in pb["mobs_kf"][pb["mobs_offset"][m]:pb["mobs_offset"][m + 1]]} for m in range(len(pb["Twm"]))}
    for k in range(q["nnodes"]):
        sub, todo = set(), [k]
        while todo:
            c = todo.pop()
            sub |= set(p["own"][c])
            todo += [int(x) for x in p["children"][c] if x >= 0]
        kfs = {int(p["v_kf"][v]) for v in sub}
        assert {v for v in p["boundary"][k] if v >= nf} == {mv for mv, who in seen.items() if who & kfs}, k


def test_the_plan_grows_with_the_observations_not_with_keyframes_times_points():
    """a chain twice as long with twice the points has about twice the items and pairs, not four times"""
    a, b = PB.make(S.chain(12, 400)), PB.make(S.chain(24, 800))
    print(a["nitems"], b["nitems"], a["npairs"], b["npairs"])
    assert 1.7 <= b["nitems"] / a["nitems"] <= 2.4 and b["npairs"] / a["npairs"] <= 2.6
    assert a["nitems"] <= 400 * 15 and b["nitems"] <= 800 * 15          # at most 5 observations a point: 5 x 6 / 2 items


def test_bounds():
    assert PB.check_sizes([4000, 0, 0, 96, 0]) == (OK, "")
    rc, msg = PB.check_sizes([4000, 0, 0, 97, 0])
    assert rc == ERR_CAPACITY and "ORBFE_GBA_MAX_POSES = 4096" in msg
    assert PB.check_sizes([1, 0, 0, 0, 0], 0)[0] == ERR_INVALID and PB.check_sizes([1, 0, 0, 0, 0], 21)[0] == ERR_INVALID
    assert PB.check_sizes([1, 0, 0, 0, 0], 20)[0] == OK and PB.check_sizes([1, 0, 0, 0, 0], 10, -1)[0] == ERR_INVALID
    rc, msg = PB.check_graph(S.obs257())
    assert rc == ERR_CAPACITY and "ORBFE_GBA_MAX_OBSERVATIONS = 256" in msg
    pb = S.case("init2_p120_r20")
    assert PB.check_graph(pb) == (OK, "")
    twice = dict(pb, obs_kf=pb["obs_kf"].copy())
    twice["obs_kf"][1] = twice["obs_kf"][0]
    assert PB.check_graph(twice)[0] == ERR_INVALID and "twice" in PB.check_graph(twice)[1]
    far = dict(pb, obs_kf=pb["obs_kf"].copy())
    far["obs_kf"][5] = 2
    assert PB.check_graph(far)[0] == ERR_INVALID


def test_a_complete_covisibility_graph_past_the_front_budget_is_refused_by_the_plan_alone():
    one = PB.make(S.complete_graph(200))
    assert one["rc"] == 0 and one["npairs"] == 199 * 200 // 2
    r = PB.make(S.complete_graph(1700))
    assert r["rc"] == ERR_CAPACITY and "GBA_FRONT_BUDGET" in r["msg"] and "768 MB" in r["msg"]


def test_scratch_and_launch_counts():
    off, ext, sizes = PB.scratch([24, 600, 2425, 3, 10], 2)
    assert all(o % 256 == 0 for o in off.values()) and list(off) == list(PB.SCRATCH) and sorted(off.values()) == list(off.values())
    assert ext == dict(zero_end=17920, end=4599808) and sizes == dict(bytes=4599808, S=109152, tables=368640, fronts=3028232)
    assert PB.scratch([12, 400, 1591, 0, 0], 2)[1] == dict(zero_end=11520, end=1144832)
    assert PB.scratch([7, 150, 476, 2, 3], 2)[2] == dict(bytes=380928, S=13248, tables=29952, fronts=106952)
    # the loop of tools/essential_timing.py is a legal size; its fronts are bounded by the budget
    big = PB.scratch([1000, 20000, 100000, 0, 0], 0)[2]
    assert big["fronts"] == (768 << 20) + 8 and big["bytes"] == 1134329088
    s = PB.schedule(S.case("chain12_p400_leaf2"))
    assert s == dict(npb=7, nb=7, g_setup=7, g_pairs=45, nlevels=4, back_levels=3, lds_rows=42, tri_bytes=7224, iterations=10, trials=10, launches_trial=12,
                     launches_iteration=123, launches=1233, host_scratch_bytes=811520)
    r = PB.schedule(S.case("ring24_p600_m3_out_r1"))
    assert (r["nlevels"], r["launches_trial"], r["launches"], r["host_scratch_bytes"]) == (6, 16, 1633, 1502208)
    assert PB.schedule(S.case("ring24_p600_m3_out_r1"), inspect=True)["launches"] == 20
    assert PB.schedule(S.case("chain12_p400_leaf2"), iterations=20)["launches"] == 2463
    # the most rows, 6 a vertex, whose packed triangle fits beside the kernel's own 1 KB: 12 x 13 / 2 x 8 = 624 B fit 2 KB, 18 rows (1368 B) do not
    assert PB.schedule(S.case("chain12_p400_leaf2"), lds_limit=2048)["lds_rows"] == 12


def test_plan_under_sanitizers():
    exe = PB.sanitizer_program()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "gba_plan: 1832 checks ok" in r.stdout, r.stdout
