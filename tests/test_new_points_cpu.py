"""CPU tests of CreateNewMapPoints: the ABI list, the host-only plan header (csrc/new_points_plan.hpp through
tests/new_points_plan_driver.cpp), and the CPU restatement (tests/new_points_ref.cpp) on its own terms -- a float64 second opinion on
every point it creates, every status code, the neighbour order, and the share of matches the parity contract excludes, for every case
the GPU tests use."""
import ctypes as C
import os

import numpy as np
import pytest

import new_points_cases as nc
import ref_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["orbfe_new_points_prepare_batch_device", "orbfe_triangulate_matches_batch_device", "orbfe_create_new_map_points_device",
       "orbfe_create_new_map_points", "orbfe_new_points_inspect"]
ERR_INVALID, ERR_CAPACITY = -1, -4


def test_new_symbols_are_declared_bound_and_built():
    from orb_slam2_aruco_amd import binding, header
    for s in NEW:
        assert s in header.functions, s
        assert s in binding.SYMBOLS, s
    assert "new_map_points.hip" in __import__("__graft_entry__").HIP_SOURCES
    if os.path.exists(binding.LIB_PATH):
        L = C.CDLL(binding.LIB_PATH)
        assert all(hasattr(L, s) for s in NEW)


def test_svd_lives_in_one_header():
    csrc = os.path.join(ROOT, "orb_slam2_aruco_amd", "csrc")
    assert "void svd_jacobi(" in open(os.path.join(csrc, "svd_jacobi.hpp")).read()
    for f in ("initializer.hip", "new_map_points.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert '#include "svd_jacobi.hpp"' in txt and "void svd_jacobi(" not in txt, f


# ---------------------------------------------------------------------------------------------------- the plan header
def plan():
    L = ref_build.build_shared("new_points_plan_driver.cpp", std="c++17", prefix="new_points_plan_")
    vp, i32 = C.c_void_p, C.c_int
    L.nplan_constants.argtypes = [vp]
    L.nplan_check_common.argtypes = [i32, i32, i32, i32, vp, vp, i32]
    L.nplan_check_levels.argtypes = [vp, vp, i32, C.c_float, vp, i32]
    L.nplan_geometry.argtypes = [i32, i32, vp]
    L.nplan_chain_step.argtypes = [i32, i32, i32, vp]
    L.nplan_host_layout.argtypes = [i32, i32, i32, vp]
    return L


def _out(fn, n, *args):
    o = np.zeros(n, np.int64)
    fn(*args, o.ctypes.data_as(C.c_void_p))
    return o.tolist()


def test_plan_constants_and_geometry():
    L = plan()
    assert _out(L.nplan_constants, 7) == [256, 4096, 16, 1, 6, 16, 12]
    # prepare: a workgroup per pair; triangulate: 256 features a workgroup, pairs along y; launches 1 + npairs * (1 + 1)
    assert _out(L.nplan_geometry, 7, 512, 6) == [6, 1, 256, 2, 6, 256, 13]
    assert _out(L.nplan_geometry, 7, 513, 1) == [1, 1, 256, 3, 1, 256, 3]
    assert _out(L.nplan_geometry, 7, 1, 20) == [20, 1, 256, 1, 20, 256, 41]
    assert _out(L.nplan_geometry, 7, 4096, 300)[3:6] == [16, 300, 256]


def test_plan_validation():
    L = plan()
    K = np.array([500, 500, 320, 240], np.float32)
    msg = C.create_string_buffer(160)
    chk = lambda cap, npairs, p1, p2, k=K: L.nplan_check_common(cap, npairs, p1, p2, None if k is None else k.ctypes.data_as(C.c_void_p), msg, 160)
    assert chk(512, 6, 1, 1) == 0 and chk(512, 6, 0, 0) == 0 and chk(4096, 0, 0, 0) == 0
    assert chk(0, 1, 0, 0) == ERR_INVALID and chk(512, -1, 0, 0) == ERR_INVALID
    assert chk(512, 1, 1, 0) == ERR_INVALID and b"both" in msg.value
    assert chk(512, 1, 0, 0, None) == ERR_INVALID
    assert chk(512, 1, 0, 0, np.array([np.nan, 500, 320, 240], np.float32)) == ERR_INVALID
    assert chk(512, 1, 0, 0, np.array([500, 0, 320, 240], np.float32)) == ERR_INVALID
    assert chk(4097, 1, 0, 0) == ERR_CAPACITY and b"4096" in msg.value
    sf, sg = nc.SCALE.copy(), nc.SIGMA2.copy()
    lev = lambda a, b, n, r: L.nplan_check_levels(None if a is None else a.ctypes.data_as(C.c_void_p), None if b is None else b.ctypes.data_as(C.c_void_p),
                                                  n, r, msg, 160)
    assert lev(sf, sg, 8, 1.8) == 0 and lev(sf, sg, 1, 1.8) == 0
    assert lev(sf, sg, 0, 1.8) == ERR_INVALID and lev(np.ones(17, np.float32), np.ones(17, np.float32), 17, 1.8) == ERR_INVALID
    assert lev(None, sg, 8, 1.8) == ERR_INVALID and lev(sf, sg, 8, 0.0) == ERR_INVALID and lev(sf, sg, 8, float("nan")) == ERR_INVALID
    bad = sg.copy(); bad[3] = 0
    assert lev(sf, bad, 8, 1.8) == ERR_INVALID and lev(sf, bad, 3, 1.8) == 0


def test_plan_chain_steps():
    L = plan()
    # with index arrays the blocks stay and the arrays advance; without them pair p is frames (p, p + 1): the blocks advance by p frames
    assert _out(L.nplan_chain_step, 7, 0, 1, 512) == [0, 0, 0, 0, 0, 0, 0]
    assert _out(L.nplan_chain_step, 7, 3, 1, 512) == [3, 0, 3, 0, 0, 0, 0]
    assert _out(L.nplan_chain_step, 7, 3, 0, 512) == [3, 3, 0, 3 * 512, 3 * 513, 3, 36]
    assert _out(L.nplan_chain_step, 7, 19, 0, 1000) == [19, 19, 0, 19000, 19 * 1001, 19, 228]


def test_plan_host_layout():
    L = plan()
    names = ("kps desc n fn fo ff nf tcw x3Dw valid free F12 epipole prep m12 m21 nm status x3D normal dist res inspect split down end").split()
    l = dict(zip(names, _out(L.nplan_host_layout, 26, 512, 1, 0)))
    up = lambda b: (b + 255) // 256 * 256
    assert l["kps"] == 0 and l["desc"] == up(2 * 512 * 28) and l["n"] == l["desc"] + 2 * 512 * 32 and l["fn"] == l["n"] + 256
    assert l["fo"] == l["fn"] + 4096 and l["ff"] == l["fo"] + up(2 * 513 * 4)
    assert l["down"] == l["x3Dw"] and l["split"] == l["F12"] and l["valid"] == l["x3Dw"] + 2 * 512 * 12
    assert l["inspect"] == l["end"]                      # no room asked for
    assert all(l[k] % 256 == 0 for k in names)
    i = dict(zip(names, _out(L.nplan_host_layout, 26, 100, 0, 1)))
    assert i["desc"] == i["n"] and i["fn"] == i["fo"] == i["ff"] and i["m21"] == i["nm"]      # the search's arrays take no room
    assert i["end"] == i["inspect"] + up(100 * 6 * 4)


# ---------------------------------------------------------------------------------------------------- the restatement
ALL_CASES = [("parity", n) for n in nc.PARITY_CASES] + [("edge", c) for c in nc.EDGE_COUNTS]


def _case(kind, key):
    return nc.parity_case(key) if kind == "parity" else nc.edge_case(key)


@pytest.mark.parametrize("kind,key", ALL_CASES)
def test_float64_second_opinion(kind, key):
    """every point the restatement creates against the null vector of np.linalg.svd: relative deviation <= 64 eps s1 / s3, the
    first-order perturbation bound of a null vector under an eps * s1 perturbation times 64 for the ~ten float roundings on the way
    in; on a noise-free scene the same bound against the true points"""
    sc, m12, r = _case(kind, key)
    f0, f1 = sc["frames"]
    T1, T2 = f0["Tcw"].astype(np.float64), f1["Tcw"].astype(np.float64)
    noise_free = kind == "parity" and nc.PARITY_CASES[key][1] == 0.0
    worst = worst_true = 0.0
    for i in np.flatnonzero(r["status"] == 1):
        x, s1, s3 = nc.dlt64(f0["kps"], T1, f1["kps"], T2, i, m12[i])
        bound = 64 * nc.FLT_EPS * s1 / s3
        worst = max(worst, np.linalg.norm(r["x3D"][i] - x) / np.linalg.norm(x) / bound)
        if noise_free:
            Xt = sc["X"][sc["landmark"][0][i]]
            worst_true = max(worst_true, np.linalg.norm(r["x3D"][i] - Xt) / np.linalg.norm(Xt) / bound)
    print("%s %s: worst deviation / bound %.4f (float64 DLT), %.4f (true points)" % (kind, key, worst, worst_true))
    assert worst <= 1.0 and worst_true <= 1.0
    if noise_free:
        assert (r["status"] == 1).sum() > 50


def test_every_status_code_on_the_restatement():
    c = nc.every_code_case()
    seen = set()
    for (a, b), m in zip(c["pairs"], c["match12"]):
        r = nc.ref_triangulate(c["kps"][a], c["Tcw"][a], c["kps"][b], c["Tcw"][b], m)
        assert r["rc"] == 0
        seen |= set(r["status"].tolist())
    assert seen == set(range(11)), sorted(seen)
    r = nc.ref_triangulate(c["kps"][0], c["Tcw"][0], c["kps"][1], c["Tcw"][1], c["match12"][0])
    assert r["status"].tolist() == [1, 2, 5, 6, 7, 8, 10, 0, 0, 0]


def test_invalid_octave_on_the_restatement():
    sc, m12, _ = nc.edge_case(65)
    f0, f1 = sc["frames"]
    k = f1["kps"].copy()
    k["octave"][m12[np.flatnonzero(m12 >= 0)[7]]] = nc.NLEVELS
    r = nc.ref_triangulate(f0["kps"], f0["Tcw"], k, f1["Tcw"], m12)
    assert r["rc"] == -1 and tuple(r["result"]) == (0, 0, -1) and not r["status"].any()


@pytest.mark.parametrize("m", [1, 2, 5, 6])
def test_median_depth_index(m):
    """ComputeSceneMedianDepth(2) takes the (m - 1) / 2-th smallest: the lower median for an even count"""
    rng = np.random.default_rng(m)
    x = np.zeros((12, 3), np.float32); x[:, 2] = rng.uniform(-3, 9, 12)
    valid = np.zeros(12, np.uint8); valid[rng.permutation(12)[:m]] = 1
    T = nc.tcw(np.eye(3), [0, 0, 0]); T2 = nc.tcw(np.eye(3), [-0.5, 0, 0])
    _, _, rec = nc.ref_prepare(dict(Tcw=T), dict(Tcw=T2, x3Dw=x, valid=valid))
    assert rec["n_depths"] == m and rec["median_depth"] == np.sort(x[valid != 0, 2])[(m - 1) // 2]


def test_neighbour_order_on_the_restatement():
    """two neighbours that match the same features of the current keyframe: the second creates no point on a feature the first took,
    and the unordered (single-launch) result differs -- the property the GPU chain test relies on"""
    sc = nc.chain_scene()
    out, st = nc.ref_sequence(sc["frames"])
    taken = np.zeros(nc.CAPACITY, bool)
    total = 0
    for o in out:
        created = o["status"] == 1
        assert not np.any(created & taken)
        assert not np.any((o["match12"] >= 0) & taken)         # the search skipped them already
        taken |= created
        total += int(created.sum())
    assert sum(int((o["status"] == 1).sum()) > 20 for o in out) >= 2
    assert np.array_equal(st[0][1] != 0, taken | (sc["frames"][0]["valid"] != 0))
    un, _ = nc.ref_sequence(sc["frames"], ordered=False)
    again = sum(int(((u["status"] == 1) & (out[0]["status"] == 1)).sum()) for u in un[1:])
    assert again > 20 and any(not np.array_equal(u["status"], o["status"]) for u, o in zip(un, out))


@pytest.mark.parametrize("kind,key", ALL_CASES)
def test_excluded_share_is_capped(kind, key):
    """the matches whose gate quantity lies inside a band of the parity contract: at most 5 % of a case's matches"""
    sc, m12, r = _case(kind, key)
    band = nc.banded(r, sc["frames"][0]["kps"], sc["frames"][1]["kps"], m12)
    nmatch = int((m12 >= 0).sum())
    print("%s %s: %d of %d matches inside a band" % (kind, key, int(band.sum()), nmatch))
    assert band.sum() <= 0.05 * nmatch
    assert not np.any(band & (m12 < 0))


def test_excluded_share_of_the_chain_case():
    sc = nc.chain_scene()
    out, _ = nc.ref_sequence(sc["frames"])
    for p, o in enumerate(out, 1):
        band = nc.banded(o, sc["frames"][0]["kps"], sc["frames"][p]["kps"], o["match12"])
        nmatch = int((o["match12"] >= 0).sum())
        print("chain neighbour %d: %d of %d matches inside a band" % (p, int(band.sum()), nmatch))
        assert band.sum() <= 0.05 * nmatch


# ---------------------------------------------------------------------------------------------------- the shim
def _library():
    from orb_slam2_aruco_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def test_local_mapping_shim_builds_and_refuses_without_a_gpu(tmp_path):
    """include/shims/LocalMapping_orbfe.cc with its driver: g++ -Wall -Werror against the mock tree, linked against liborbfe.so;
    without a GPU the driver stops at the library's loud "no device" answer"""
    import subprocess
    import local_mapping_shim_build as lb
    from orb_slam2_aruco_amd import binding
    _library()
    exe = lb.build(str(tmp_path))
    assert os.path.exists(exe)
    if binding.load().orbfe_device_count() > 0:
        return          # a GPU is present: tests/test_new_points_gpu.py runs the driver
    lb.write_inputs(str(tmp_path / "in"), nc.smoke_scene()["frames"], nc.K4, nc.SCALE, nc.SIGMA2)
    r = subprocess.run([exe, str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 3 and "HIP device" in r.stderr and "no CPU fallback" in r.stderr


def test_eight_shims_link_into_one_program(tmp_path):
    import subprocess
    import shim_build
    _library()
    r = subprocess.run([shim_build.build("all", str(tmp_path))], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: 11 shims"), r.stderr
