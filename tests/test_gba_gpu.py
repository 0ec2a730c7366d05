"""GPU tests of GlobalBundleAdjustment (csrc/global_ba.hip) against the CPU restatement tests/gba_ref.cpp, which solves the reduced
system densely: the stages of one linearisation and trial and the elimination tree (orbfe_gba_inspect), the whole call on every case
of tests/gba_cases.py (tolerance = 10 x the spread between the restatement's two summation orders, tests/gba_parity.py), equal bits
between the host call, the device call and a repeat, the (keyframe, feature) observation form, the leaf sizes, the vertices that are
no part of the system, the stop flag, the bounds, and the chain behind orbfe_optimize_essential_graph_device."""
import numpy as np
import pytest

import gba_build as B
import gba_cases as S
import gba_parity as P
from pose_opt_device import Dev, Out

pytestmark = pytest.mark.gpu

_gpu = {}


def gpu_result(orbfe, name):
    if name not in _gpu:
        _gpu[name] = orbfe.global_bundle_adjustment(P.problem(name)[0])
    return _gpu[name]


@pytest.mark.parametrize("name", ["chain12_p400_leaf2", "ring24_p600_m3_out_r1"])
def test_one_linearisation_and_trial_match_the_restatement(orbfe, name):
    """b, the diagonal blocks, chi2 and lambda0 against the restatement in device order: 1e-9 of each array's largest entry, the level
    the 2e-9 divisor of the numeric Jacobians leaves.  The first update to 1e-6, the figure of the local bundle
    adjustment for the same solve; the restatement's dense factorisation and the library's sparse fronts eliminate in different
    orders.  The tree is the plan's: every vertex in one node, a parent above every node but the root, own vertices summing to nv."""
    pb = P.problem(name)[0]
    g, r = orbfe.gba_inspect(pb), B.inspect(pb, B.DEVICE)
    nv = int((pb["kf_fixed"] == 0).sum()) + (len(pb["Twm"]) if pb["use_markers"] else 0)
    assert g["nv"] == r["nv"] == nv and g["solved"] and r["solved"]
    for key, rel in (("b_pose", 1e-9), ("b_point", 1e-9), ("Hpp", 1e-9), ("Hll", 1e-9), ("x_pose", 1e-6), ("x_point", 1e-6)):
        scale = np.abs(r[key]).max()
        err = np.abs(g[key] - r[key]).max() / scale
        print("%s %-8s max |d| / max |ref| = %.2e" % (name, key, err))
        assert err <= rel, key
    assert abs(g["chi2"] - r["chi2"]) <= 1e-9 * r["chi2"] and abs(g["lambda0"] - r["lambda0"]) <= 1e-9 * r["lambda0"]
    import gba_plan_build as PB
    plan = PB.make(pb)
    assert g["nlevels"] == plan["nlevels"] >= 3 and np.array_equal(g["node_of"], plan["node_of"]) and np.array_equal(g["order_of"], plan["order_of"])
    for key in ("parent", "level", "nown", "nb"):
        assert np.array_equal(g[key], plan[key]), key
    assert g["nown"].sum() == nv and sorted(g["order_of"]) == list(range(nv)) and (g["parent"] == -1).sum() == 1


def test_whole_call_matches_the_restatement_on_every_case(orbfe):
    """Poses, points and marker poses within 10 x the order spread, against the restatement in either order; iterations and trials
    are reported, not asserted (they turn on rounding).  No number is taken from the GPU result."""
    tol = P.tolerance()
    print("tolerance:", {k: "%.2e" % v for k, v in tol.items()})
    left_out = P.spread()["left_out"]
    assert len(left_out) <= P.MAX_NOT_COMPARED * len(P.NAMES), left_out
    worst = {o: dict.fromkeys(P.QUANTITIES, 0.0) for o in (0, 1)}
    failures = []
    for name in P.NAMES:
        pb, r0, r1 = P.problem(name)
        g = gpu_result(orbfe, name)
        res = g["result"]
        assert res["status"] == 0 and res["n_edges_mono"] == len(pb["obs_kf"]) and res["n_points_left_out"] == r0["result"]["n_points_left_out"]
        assert res["n_edges_marker"] == (4 * len(pb["mobs_kf"]) if pb["use_markers"] else 0)
        print("%-26s gpu it %d tr %d chi2 %.6g -> %.6g   ref it %d tr %d chi2 %.6g -> %.6g" % (
            name, res["iterations"], res["trials"], res["chi2_first"], res["chi2_last"], r0["result"]["iterations"], r0["result"]["trials"],
            r0["result"]["chi2_first"], r0["result"]["chi2_last"]))
        if name in left_out:
            continue
        for order, r in ((0, r0), (1, r1)):
            d = P.distance(r, g, pb)
            print("    order %d  " % order + "  ".join("%s %.2e" % (k, d[k]) for k in P.QUANTITIES))
            for k in P.QUANTITIES:
                worst[order][k] = max(worst[order][k], d[k])
            if not P.within(d, tol):
                failures.append((name, order, d))
    for order in (0, 1):
        print("GPU vs restatement order %d, maxima: %s" % (order, {k: "%.2e" % v for k, v in worst[order].items()}))
    assert not failures, failures


def _device_run(orbfe, pb, form_kps=False, stop=None, d_Tcw=None, d_x3Dw=None):
    """the device call on copies of pb's arrays (or in place on the given device blocks); returns (dict like the host call's, arrays)"""
    a = orbfe.gba_arrays(pb)
    nkf, n, nobs, nma, nmobs = len(a["Tcw"]), len(a["x3Dw"]), len(a["obs_kf"]), len(a["Twm"]), len(a["mobs_kf"])
    d = dict(Tcw=d_Tcw or Out(a["Tcw"]), x3Dw=d_x3Dw or Out(a["x3Dw"]), Twm=Out(a["Twm"]), res=Out(np.zeros(1, orbfe.GBA_RESULT_DTYPE)))
    for k in ("marker_local", "mobs_corners"):
        d[k] = Dev(a[k])
    cap = 0
    if form_kps:
        # the observations as features of resident keypoint blocks: keyframe k's block holds its observations from the back
        cap = int(np.bincount(a["obs_kf"], minlength=nkf).max()) + 3
        kps = np.zeros((nkf, cap), orbfe.KP_DTYPE)
        kps["octave"] = -1
        feat = np.zeros(nobs, np.int32)
        fill = np.zeros(nkf, np.int64)
        for e in range(nobs):
            k = a["obs_kf"][e]
            f = cap - 1 - fill[k]
            fill[k] += 1
            kps[k, f]["x"], kps[k, f]["y"], kps[k, f]["octave"] = a["obs_xy"][e, 0], a["obs_xy"][e, 1], a["obs_octave"][e]
            feat[e] = f
        d["kps"], d["obs_feature"] = Dev(kps), Dev(feat)
    else:
        d["obs_xy"], d["obs_octave"] = Dev(a["obs_xy"]), Dev(a["obs_octave"])
    if stop is not None:
        d["stop"] = Dev(np.array([stop], np.uint8))
    nbytes = orbfe.gba_scratch_bytes(nkf, n, nobs, nma, nmobs, a["leaf_vertices"])
    assert nbytes > 0
    d["scratch"] = Out(np.zeros(nbytes, np.uint8))
    ptr = {k: v.ptr for k, v in d.items()}
    ptr["scratch_bytes"] = nbytes
    orbfe.global_bundle_adjustment_device(pb, ptr, capacity=cap)
    d["scratch"].get()
    out = dict(Tcw=d["Tcw"].get().reshape(-1, 3, 4), x3Dw=d["x3Dw"].get().reshape(-1, 3), Twm=d["Twm"].get().reshape(-1, 3, 4), result=d["res"].get()[0])
    return out, a


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("Tcw", "x3Dw", "Twm")) and a["result"].tobytes() == b["result"].tobytes()


@pytest.mark.parametrize("name", ["ring24_p600_m3_out_r1", "orphans", "p257", "k70_p300"])
def test_device_call_host_call_and_a_repeat_give_equal_bits(orbfe, name):
    """in place on the caller's arrays, guard bytes around every in-place array and the scratch untouched"""
    pb = P.problem(name)[0]
    host = gpu_result(orbfe, name)
    dev, _ = _device_run(orbfe, pb)
    assert _same_bits(host, dev), (host["result"], dev["result"])
    assert _same_bits(host, orbfe.global_bundle_adjustment(pb))
    assert _same_bits(dev, _device_run(orbfe, pb)[0])


def test_keyframe_feature_observation_form_equals_the_host_call(orbfe):
    pb = P.problem("chain12_p400")[0]
    assert _same_bits(gpu_result(orbfe, "chain12_p400"), _device_run(orbfe, pb, form_kps=True)[0])


@pytest.mark.parametrize("name", ["chain12_p400", "ring24_p600_m3_out_r1"])
def test_leaf_sizes_agree_and_each_repeats_its_bits(orbfe, name):
    """leaf_vertices = 2, the default and 4096 (one front: the dense solve) eliminate in different orders: each within the tolerance
    of the others, each with equal bits on a repeat"""
    pb = P.problem(name)[0]
    runs = {leaf: orbfe.global_bundle_adjustment(dict(pb, leaf_vertices=leaf)) for leaf in (2, 0, 4096)}
    assert orbfe.gba_inspect(dict(pb, leaf_vertices=4096))["nlevels"] <= (2 if pb["use_markers"] else 1)
    assert orbfe.gba_inspect(dict(pb, leaf_vertices=2))["nlevels"] >= 3
    tol = P.tolerance()
    for leaf, r in runs.items():
        assert _same_bits(r, orbfe.global_bundle_adjustment(dict(pb, leaf_vertices=leaf))), leaf
        d = P.distance(runs[2], r, pb)
        print(name, "leaf", leaf, "it", r["result"]["iterations"], {k: "%.2e" % v for k, v in d.items()})
        assert P.within(d, tol), (leaf, d)


def test_vertices_without_an_edge_keep_their_bits(orbfe):
    """the point without observations, the free keyframe without an edge and the marker without observations come back to the bit,
    n_points_left_out counts the point; with use_markers = 0 no marker is written and no marker edge exists"""
    pb = P.problem("orphans")[0]
    a = orbfe.gba_arrays(pb)
    for g in (gpu_result(orbfe, "orphans"), _device_run(orbfe, pb)[0]):
        assert g["result"]["n_points_left_out"] == 1 and g["result"]["n_edges_marker"] == 12
        i, k, m = pb["lonely_point"], pb["lonely_keyframe"], pb["lonely_marker"]
        assert np.array_equal(g["x3Dw"][i].view(np.uint32), a["x3Dw"][i].view(np.uint32))
        assert np.array_equal(g["Tcw"][k].reshape(-1).view(np.uint32), a["Tcw"][k].view(np.uint32))
        assert np.array_equal(g["Twm"][m].reshape(-1).view(np.uint32), a["Twm"][m].view(np.uint32))
        assert np.array_equal(g["Tcw"][0].reshape(-1).view(np.uint32), a["Tcw"][0].view(np.uint32))      # the fixed keyframe
        assert not np.array_equal(g["Twm"][0].reshape(-1), a["Twm"][0]) and not np.array_equal(g["Tcw"][1].reshape(-1), a["Tcw"][1])
    unused = gpu_result(orbfe, "orphans_markers_unused")
    assert np.array_equal(unused["Twm"].reshape(-1, 12).view(np.uint32), a["Twm"].view(np.uint32)) and unused["result"]["n_edges_marker"] == 0


def test_stop_flag(orbfe):
    pb = P.problem("chain12_p400")[0]
    a = orbfe.gba_arrays(pb)
    r = orbfe.global_bundle_adjustment(pb, stop=True)
    assert r["result"]["status"] == orbfe.GBA_STOPPED and r["result"]["n_edges_mono"] == 0 and r["result"]["iterations"] == 0
    assert np.array_equal(r["Tcw"].reshape(-1, 12).view(np.uint32), a["Tcw"].view(np.uint32)) and np.array_equal(r["x3Dw"].view(np.uint32), a["x3Dw"].view(np.uint32))
    d, _ = _device_run(orbfe, pb, stop=1)
    assert d["result"]["status"] == orbfe.GBA_STOPPED and d["result"]["n_edges_mono"] == 0
    assert np.array_equal(d["Tcw"].reshape(-1, 12).view(np.uint32), a["Tcw"].view(np.uint32)) and np.array_equal(d["x3Dw"].view(np.uint32), a["x3Dw"].view(np.uint32))
    # a flag that stays 0 changes nothing
    assert _same_bits(_device_run(orbfe, pb, stop=0)[0], gpu_result(orbfe, "chain12_p400"))


def test_bounds_and_invalid_input(orbfe):
    """4096 poses are a legal size and 4097 are refused, by the sizes alone; a short or misaligned scratch is refused before any
    launch; a bad octave and a NaN come back as return codes of the host call and in the record of the device call, with nothing else
    written.  (The front budget is the plan's to refuse: tests/test_gba_plan_cpu.py.)"""
    assert orbfe.gba_scratch_bytes(4090, 0, 0, 6, 0) > 0 and orbfe.gba_scratch_bytes(4090, 0, 0, 7, 0) == 0
    empty = dict(Tcw=np.zeros((4097, 12), np.float32), kf_fixed=np.zeros(4097, np.uint8), K=S.K4, inv_level_sigma2=S.INV_SIGMA2)
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.global_bundle_adjustment(empty)
    assert "(-4)" in str(e.value) and "ORBFE_GBA_MAX_POSES" in str(e.value)
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.global_bundle_adjustment_device(empty, dict(Tcw=256, res=256, scratch=256, scratch_bytes=1 << 40))
    assert "(-4)" in str(e.value) and "ORBFE_GBA_MAX_POSES" in str(e.value)
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.global_bundle_adjustment(S.obs257())
    assert "(-4)" in str(e.value) and "ORBFE_GBA_MAX_OBSERVATIONS" in str(e.value)
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.global_bundle_adjustment(S.bad_octave())
    assert "(-1)" in str(e.value) and "octave" in str(e.value)
    bad = S.case("init2_p120_r20")
    bad["x3Dw"] = bad["x3Dw"].copy()
    bad["x3Dw"][3, 1] = np.nan
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.global_bundle_adjustment(bad)
    assert "(-1)" in str(e.value)
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.global_bundle_adjustment(dict(S.case("init2_p120_r20"), iterations=21))
    assert "(-1)" in str(e.value) and "iterations" in str(e.value)
    for pb in (S.bad_octave(), bad):
        d, a = _device_run(orbfe, pb)
        assert d["result"]["status"] == -1 and d["result"]["n_edges_mono"] == 0
        assert np.array_equal(d["Tcw"].reshape(-1, 12).view(np.uint32), a["Tcw"].view(np.uint32))
        assert np.array_equal(d["x3Dw"].view(np.uint32), a["x3Dw"].view(np.uint32))
    # the scratch: one byte short is ORBFE_ERR_CAPACITY, not 256-byte aligned is ORBFE_ERR_INVALID, both before any launch
    pb = S.case("init2_p120_r20")
    a = orbfe.gba_arrays(pb)
    nkf, n, nobs = len(a["Tcw"]), len(a["x3Dw"]), len(a["obs_kf"])
    nbytes = orbfe.gba_scratch_bytes(nkf, n, nobs, 0, 0)
    out = dict(Tcw=Out(a["Tcw"]), x3Dw=Out(a["x3Dw"]), res=Out(np.full(12, -1, np.int32)), scratch=Out(np.full(nbytes + 256, 0xA5, np.uint8)))
    d = dict(out, obs_xy=Dev(a["obs_xy"]), obs_octave=Dev(a["obs_octave"]))
    for shift, short, code in ((0, 1, "(-4)"), (128, 0, "(-1)")):
        ptr = {k: v.ptr for k, v in d.items()}
        ptr["scratch"] += shift
        ptr["scratch_bytes"] = nbytes - short
        with pytest.raises(orbfe.OrbfeError) as e:
            orbfe.global_bundle_adjustment_device(pb, ptr)
        assert code in str(e.value)
        for k, v in out.items():
            assert np.array_equal(v.get().view(np.uint8), v.a.view(np.uint8)), k


def test_chain_behind_the_essential_graph_on_one_stream(orbfe):
    """orbfe_optimize_essential_graph_device and orbfe_global_bundle_adjustment_device back to back on one stream: the bundle adjustment
    works in place on the essential graph's d_Tcw_out / d_x3Dw_out and nothing is fetched in between.  The result equals the two host
    calls in sequence bit for bit.  A ring of 24 keyframes; every point is observed from the three keyframes around its reference
    one, at the pixels the input map projects it to."""
    import essential_cases as E
    ep = E.case("ring24_leaf2")
    ea = orbfe.eg_arrays(ep)
    nkf, n = len(ea["Tcw"]), len(ea["x3Dw"])
    assert nkf == 24 and n >= 100
    T = ea["Tcw"].reshape(-1, 3, 4).astype(np.float64)
    off, okf, oxy = [0], [], []
    for i in range(n):
        ref = int(ea["point_ref"][i])
        for k in ([(ref + s) % nkf for s in (-1, 0, 1)] if ref >= 0 else []):
            uv, z = S.project(T[k], ea["x3Dw"][i:i + 1].astype(np.float64))
            if z[0] > 0.1 and np.isfinite(uv).all():
                okf.append(k); oxy.append(uv[0])
        off.append(len(okf))
    assert len(okf) > 2 * nkf
    fixed = np.zeros(nkf, np.uint8)
    fixed[ea["fixed"]] = 1
    host_eg = orbfe.optimize_essential_graph(ep)
    gp = dict(Tcw=host_eg["Tcw"], kf_fixed=fixed, x3Dw=host_eg["x3Dw"], obs_offset=np.array(off, np.int32), obs_kf=np.array(okf, np.int32),
              obs_xy=np.array(oxy, np.float32).reshape(-1, 2), obs_octave=np.zeros(len(okf), np.int32), K=S.K4, inv_level_sigma2=S.INV_SIGMA2,
              iterations=10, robust=0, leaf_vertices=2)
    host = orbfe.global_bundle_adjustment(gp)
    assert host["result"]["status"] == 0 and host["result"]["iterations"] >= 1
    assert not np.array_equal(host["Tcw"], host_eg["Tcw"])
    # the same on the device, one stream (the null stream), nothing fetched in between
    eb = orbfe.essential_graph_scratch_bytes(nkf, len(ea["edge_i"]), n, ea["leaf_vertices"])
    Tout, Xout = Out(np.zeros((nkf, 12), np.float32)), Out(np.zeros((n, 3), np.float32))
    ed = dict(Tcw=Dev(ea["Tcw"]), corrected_pos=Dev(ea["corrected_pos"]), corrected=Dev(ea["corrected"]), noncorrected_pos=Dev(ea["noncorrected_pos"]),
              noncorrected=Dev(ea["noncorrected"]), x3Dw=Dev(ea["x3Dw"]), point_ref=Dev(ea["point_ref"]), Tcw_out=Tout, x3Dw_out=Xout,
              res=Out(np.zeros(1, orbfe.EG_RESULT_DTYPE)), scratch=Out(np.zeros(eb, np.uint8)))
    eptr = {k: v.ptr for k, v in ed.items()}
    eptr["scratch_bytes"] = eb
    orbfe.optimize_essential_graph_device(ep, eptr)
    dev, _ = _device_run(orbfe, gp, d_Tcw=Tout, d_x3Dw=Xout)
    ed["scratch"].get()
    assert np.array_equal(dev["Tcw"].view(np.uint32), host["Tcw"].view(np.uint32))
    assert np.array_equal(dev["x3Dw"].view(np.uint32), host["x3Dw"].view(np.uint32))
    assert dev["result"].tobytes() == host["result"].tobytes()
