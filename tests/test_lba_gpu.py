"""GPU tests of LocalBundleAdjustment (csrc/local_ba.hip) against the CPU restatement tests/lba_ref.cpp: the stages of one
linearisation and trial (orbfe_lba_inspect), the decisions and results of the whole call on every case of tests/lba_cases.py
(tolerance = 10 x the spread between the restatement's two summation orders, tests/lba_parity.py), equal bits between the host call,
the device call and a repeat, the (keyframe, feature) observation form, and the edge conditions of include/orbfe.h."""
import numpy as np
import pytest

import lba_build as B
import lba_cases as S
import lba_parity as P
from pose_opt_device import Dev, Out

pytestmark = pytest.mark.gpu

_gpu = {}


def gpu_result(orbfe, name):
    if name not in _gpu:
        _gpu[name] = orbfe.local_bundle_adjustment(P.problem(name)[0])
    return _gpu[name]


@pytest.mark.parametrize("name", ["k4f2_p300_out10", "k6f3_p1000_out20_m2"])
def test_one_linearisation_and_trial_match_the_restatement(orbfe, name):
    """b, the diagonal blocks, chi2, lambda0 and the first trial's update against the restatement in device order.  The two sum the
    same terms in the same order, so what is left is the device's libm in the numeric Jacobians (none without markers) and the
    contraction-free arithmetic of two compilers: 1e-9 of each array's largest entry, the level the 2e-9 divisor of the numeric
    Jacobians leaves, holds for the sums; the update solves a system whose condition amplifies that, 1e-6."""
    pb = P.problem(name)[0]
    g, r = orbfe.lba_inspect(pb), B.inspect(pb, B.DEVICE)
    assert g["nv"] == r["nv"] == int((pb["kf_fixed"] == 0).sum()) + (len(pb["Twm"]) if pb["use_markers"] else 0)
    for key, rel in (("b_pose", 1e-9), ("b_point", 1e-9), ("Hpp", 1e-9), ("Hll", 1e-9), ("x_pose", 1e-6), ("x_point", 1e-6)):
        scale = np.abs(r[key]).max()
        err = np.abs(g[key] - r[key]).max() / scale
        print("%s %-8s max |d| / max |ref| = %.2e" % (name, key, err))
        assert err <= rel, key
    assert abs(g["chi2"] - r["chi2"]) <= 1e-9 * r["chi2"] and abs(g["lambda0"] - r["lambda0"]) <= 1e-9 * r["lambda0"]


def test_whole_call_matches_the_restatement_on_every_case(orbfe):
    """Decisions equal (n_level1, n_erase, every erase byte) unless the gate rule sets the case aside, at most 10 % of the cases;
    poses, points and marker poses within 10 x the order spread, against the restatement in either order."""
    tol = P.tolerance()
    print("tolerance:", {k: "%.2e" % v for k, v in tol.items()})
    worst = {o: dict.fromkeys(P.QUANTITIES, 0.0) for o in (0, 1)}
    not_compared, failures = [], []
    for name in P.NAMES:
        pb, r0, r1 = P.problem(name)
        g = gpu_result(orbfe, name)
        res = g["result"]
        assert res["status"] == 0 and res["n_edges_mono"] == len(pb["obs_kf"])
        assert res["n_edges_marker"] == (4 * len(pb["mobs_kf"]) if pb["use_markers"] else 0)
        print("%-22s gpu %s ref %s" % (name, res, r0["result"]))
        for order, r in ((0, r0), (1, r1)):
            if not P.decisions_equal(r, g):
                if P.gated(r, g):
                    not_compared.append((name, order))
                else:
                    failures.append((name, order, "decisions", res, r["result"]))
                continue
            d = P.distance(r, g, pb)
            print("    order %d  " % order + "  ".join("%s %.2e" % (k, d[k]) for k in P.QUANTITIES))
            for k in P.QUANTITIES:
                worst[order][k] = max(worst[order][k], d[k])
            if not P.within(d, P.tolerance(name)):
                failures.append((name, order, d))
    for order in (0, 1):
        print("GPU vs restatement order %d, maxima: %s" % (order, {k: "%.2e" % v for k, v in worst[order].items()}))
    print("not compared:", not_compared)
    assert not failures, failures
    assert len(set(n for n, _ in not_compared)) <= P.MAX_NOT_COMPARED * len(P.NAMES), not_compared


def _device_run(orbfe, pb, form_kps=False, stop=None, sentinel=True):
    """the device call on copies of pb's arrays; returns (dict like the host call's, the buffers)"""
    a = orbfe.lba_arrays(pb)
    nkf, n, nobs, nma, nmobs = len(a["Tcw"]), len(a["x3Dw"]), len(a["obs_kf"]), len(a["Twm"]), len(a["mobs_kf"])
    mk = Out if sentinel else Dev
    d = dict(Tcw=mk(a["Tcw"]), x3Dw=mk(a["x3Dw"]), Twm=mk(a["Twm"]), erase=mk(np.full(max(nobs, 1), 7, np.uint8)),
             res=mk(np.zeros(1, orbfe.LBA_RESULT_DTYPE)))
    for k in ("kf_fixed", "obs_offset", "obs_kf", "marker_local", "mobs_offset", "mobs_kf", "mobs_corners"):
        d[k] = Dev(a[k])
    cap = 0
    if form_kps:
        # the observations as features of resident keypoint blocks: keyframe k's block holds its observations in slot order
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
    nbytes = orbfe.lba_scratch_bytes(nkf, n, nobs, nma, nmobs)
    assert nbytes > 0
    d["scratch"] = Out(np.zeros(nbytes, np.uint8))
    ptr = {k: v.ptr for k, v in d.items()}
    ptr["scratch_bytes"] = nbytes
    orbfe.local_bundle_adjustment_device(ptr, nkf, n, nobs, nma, nmobs, a["K4"], a["inv_level_sigma2"], a["marker_info"], a["use_markers"],
                                         capacity=cap)
    d["scratch"].get()
    out = dict(Tcw=d["Tcw"].get().reshape(-1, 3, 4), x3Dw=d["x3Dw"].get(), Twm=d["Twm"].get().reshape(-1, 3, 4), erase=d["erase"].get()[:nobs],
               result=d["res"].get()[0])
    return out, a


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("Tcw", "x3Dw", "Twm", "erase")) and \
        a["result"].tobytes() == b["result"].tobytes()


@pytest.mark.parametrize("name", ["k6f3_p1000_out20_m2", "special", "k3_p257"])
def test_device_call_host_call_and_a_repeat_give_equal_bits(orbfe, name):
    """in place on the caller's arrays, guard bytes around every output and the scratch untouched"""
    pb = P.problem(name)[0]
    host = gpu_result(orbfe, name)
    dev, _ = _device_run(orbfe, pb)
    assert _same_bits(host, dev), (host["result"], dev["result"])
    assert _same_bits(host, orbfe.local_bundle_adjustment(pb))
    assert _same_bits(dev, _device_run(orbfe, pb)[0])


def test_keyframe_feature_observation_form_equals_the_host_call(orbfe):
    """the form that reads resident keypoint blocks, as behind orbfe_create_new_map_points_device"""
    pb = P.problem("k4f2_p300_out10")[0]
    assert _same_bits(gpu_result(orbfe, "k4f2_p300_out10"), _device_run(orbfe, pb, form_kps=True)[0])


def test_stop_set_before_the_call_leaves_everything_untouched(orbfe):
    pb = P.problem("no_markers")[0]
    r = orbfe.local_bundle_adjustment(pb, stop=True)
    a = orbfe.lba_arrays(pb)
    assert r["result"]["status"] == orbfe.LBA_STOPPED and r["result"]["n_edges_mono"] == 0 and r["result"]["iterations"].sum() == 0
    assert np.array_equal(r["Tcw"].reshape(-1, 12), a["Tcw"]) and np.array_equal(r["x3Dw"], a["x3Dw"]) and not r["erase"].any()
    d, _ = _device_run(orbfe, pb, stop=1)
    assert d["result"]["status"] == orbfe.LBA_STOPPED and np.array_equal(d["Tcw"].reshape(-1, 12), a["Tcw"]) and np.array_equal(d["x3Dw"], a["x3Dw"])
    assert (d["erase"] == 7).all()
    # a flag that stays 0 changes nothing
    assert _same_bits(_device_run(orbfe, pb, stop=0)[0], gpu_result(orbfe, "no_markers"))


def test_bounds_and_invalid_input(orbfe):
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.local_bundle_adjustment(S.over_bound())
    assert "(-4)" in str(e.value) and "ORBFE_LBA_MAX_FREE_POSES" in str(e.value)
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.local_bundle_adjustment(S.obs257())
    assert "(-4)" in str(e.value) and "ORBFE_LBA_MAX_OBSERVATIONS" in str(e.value)
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.local_bundle_adjustment(S.bad_octave())
    assert "(-1)" in str(e.value) and "octave" in str(e.value)
    bad = S.case("k3_p40_clean")
    bad["x3Dw"] = bad["x3Dw"].copy()
    bad["x3Dw"][3, 1] = np.nan
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.local_bundle_adjustment(bad)
    assert "(-1)" in str(e.value)
    # the device call sees the same problems on the device only: it reports them in the record and writes nothing else
    for pb, status in ((S.over_bound(), -4), (S.obs257(), -4), (S.bad_octave(), -1), (bad, -1)):
        d, a = _device_run(orbfe, pb)
        assert d["result"]["status"] == status and d["result"]["n_edges_mono"] == 0
        assert np.array_equal(d["Tcw"].reshape(-1, 12).view(np.uint32), a["Tcw"].view(np.uint32)) and (d["erase"] == 7).all()
        assert np.array_equal(d["x3Dw"].view(np.uint32), a["x3Dw"].view(np.uint32))


def test_device_call_refuses_a_short_or_misaligned_scratch_before_any_launch(orbfe):
    """one byte less than orbfe_lba_scratch_bytes asks for is ORBFE_ERR_CAPACITY, a scratch that is not 256-byte aligned is
    ORBFE_ERR_INVALID; both are decided on the host: the record, the estimates, the erase bytes and the scratch keep their pattern"""
    a = orbfe.lba_arrays(S.case("k3_p40_clean"))
    nkf, n, nobs = len(a["Tcw"]), len(a["x3Dw"]), len(a["obs_kf"])
    assert (nkf, n, len(a["Twm"])) == (3, 40, 0)
    nbytes = orbfe.lba_scratch_bytes(nkf, n, nobs, 0, 0)
    # the scratch has 256 bytes to spare, so that the shifted pointer with the full size still names memory of the buffer
    out = dict(Tcw=Out(a["Tcw"]), x3Dw=Out(a["x3Dw"]), erase=Out(np.full(nobs, 7, np.uint8)), res=Out(np.full(1, -1, np.int32).repeat(9)),
               scratch=Out(np.full(nbytes + 256, 0xA5, np.uint8)))
    d = dict(out, **{k: Dev(a[k]) for k in ("kf_fixed", "obs_offset", "obs_kf", "obs_xy", "obs_octave")})
    for shift, short, code in ((0, 1, "(-4)"), (128, 0, "(-1)")):
        ptr = {k: v.ptr for k, v in d.items()}
        ptr["scratch"] += shift
        ptr["scratch_bytes"] = nbytes - short
        with pytest.raises(orbfe.OrbfeError) as e:
            orbfe.local_bundle_adjustment_device(ptr, nkf, n, nobs, 0, 0, a["K4"], a["inv_level_sigma2"], a["marker_info"], 0)
        assert code in str(e.value)
        for k, v in out.items():
            assert np.array_equal(v.get().view(np.uint8), v.a.view(np.uint8)), k


def test_special_vertices_do_not_move(orbfe):
    """the free keyframe without observations keeps its pose to the bit; the marker whose edges all went to level 1 keeps in round 2
    what round 1 left (the restatement's value, within the tolerance, is what the parity test checks); a projection through z = 0 is
    a bad edge at the first check and is erased"""
    pb = P.problem("special")[0]
    g = gpu_result(orbfe, "special")
    k = pb["lonely_keyframe"]
    alone = dict(Tcw=pb["Tcw"][k:k + 1], kf_fixed=np.zeros(1, np.uint8), K=S.K4, inv_level_sigma2=S.INV_SIGMA2)
    assert np.array_equal(g["Tcw"][k], orbfe.local_bundle_adjustment(alone)["Tcw"][0])
    assert np.array_equal(g["Tcw"][pb["kf_fixed"] != 0], orbfe.lba_arrays(pb)["Tcw"].reshape(-1, 3, 4)[pb["kf_fixed"] != 0])
    assert g["result"]["n_level1"][1] == P.problem("special")[1]["result"]["n_level1"][1] >= 8
    unused = gpu_result(orbfe, "markers_given_unused")
    assert np.array_equal(unused["Twm"].reshape(-1, 12), orbfe.lba_arrays(P.problem("markers_given_unused")[0])["Twm"]) and unused["result"]["n_edges_marker"] == 0
    pz = P.problem("z0")[0]
    gz = gpu_result(orbfe, "z0")
    assert gz["erase"][pz["z0_slot"]] == 1 and gz["result"]["n_level1"][0] >= 1


def test_chain_behind_create_new_map_points_device(orbfe):
    """CreateNewMapPoints and LocalBundleAdjustment of resident keyframes, back to back on one stream with nothing fetched in between:
    orbfe_create_new_map_points_device of one keyframe against three neighbours, then orbfe_local_bundle_adjustment_device on the SAME
    blocks -- the keypoints d_kps (capacity 512, the (keyframe, feature) observation form), the poses d_Tcw in place, and as its
    points the current keyframe's block of the map state d_x3Dw, where the chain has just written the points it created.  Which
    features get a point is data the chain decides, so the observation lists are those of the sequential restatement of the chain
    (that the device made exactly those points is asserted at the end).  The result equals the host call on the same data: the
    state a run of the chain alone leaves."""
    import new_points_cases as nc
    import test_new_points_gpu as NP
    frames = nc.chain_scene()["frames"]
    pairs = [(0, 1), (0, 2), (0, 3)]
    want, _ = nc.ref_sequence(frames, pairs)
    CAP = NP.CAP
    assert len(frames[0]["kps"]) == CAP
    # the points are the current keyframe's feature slots; the created ones are seen from it and from the neighbour that made them
    seen = [[(0, i)] if frames[0]["valid"][i] else [] for i in range(CAP)]
    for p, (a, c) in enumerate(pairs):
        for i1 in np.flatnonzero(want[p]["status"] == 1):
            assert not seen[i1]
            seen[i1] = [(a, int(i1)), (c, int(want[p]["match12"][i1]))]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.int32)
    okf = np.array([k for s in seen for k, _ in s], np.int32)
    feat = np.array([f for s in seen for _, f in s], np.int32)
    created = sum(len(s) == 2 for s in seen)
    assert created > 60 and len(set(okf)) == 4
    fixed = np.array([1, 0, 0, 0], np.uint8)
    sig = (1.0 / nc.SIGMA2).astype(np.float32)

    def chain(b):
        NP.ok(NP.lib().orbfe_create_new_map_points_device(
            b.kps.ptr, b.desc.ptr, b.n.ptr, b.fn.ptr, b.fo.ptr, b.ff.ptr, b.nfv.ptr, CAP, b.x.ptr, b.valid.ptr, b.free.ptr, b.T.ptr, b.p1.ptr,
            b.p2.ptr, b.npairs, NP.cp(nc.K4), NP.cp(nc.SCALE), NP.cp(nc.SIGMA2), nc.NLEVELS, nc.RATIO, 0, b.F12.ptr, b.epi.ptr, b.prep.ptr,
            b.m12.ptr, b.s21.ptr, b.nm.ptr, b.status.ptr, b.x3D.ptr, b.normal.ptr, b.dist.ptr, b.res.ptr, None))

    # the chain alone: the state it leaves is the host call's input
    alone = NP.Batch(frames, pairs, search=True)
    chain(alone)
    state = alone.x.get()[0].copy()
    made = np.stack([o["status"] == 1 for o in alone.outputs()])
    assert all(np.array_equal(made[p], want[p]["status"] == 1) for p in range(3)), "the device chain made other points than its restatement"
    assert np.isfinite(state).all()
    kps = alone.P["kps"]
    host = orbfe.local_bundle_adjustment(dict(Tcw=alone.P["Tcw"], kf_fixed=fixed, x3Dw=state, obs_offset=off, obs_kf=okf,
                                              obs_xy=np.stack([kps["x"][okf, feat], kps["y"][okf, feat]], 1), obs_octave=kps["octave"][okf, feat],
                                              K=nc.K4, inv_level_sigma2=sig))
    assert host["result"]["status"] == 0 and host["result"]["n_edges_mono"] == len(okf) and host["result"]["iterations"].sum() >= 2
    assert not np.array_equal(host["Tcw"][1:], alone.P["Tcw"].reshape(-1, 3, 4)[1:]) and np.array_equal(host["Tcw"][0], alone.P["Tcw"].reshape(-1, 3, 4)[0])

    # chain and bundle adjustment back to back on the null stream, on the same blocks
    b = NP.Batch(frames, pairs, search=True)
    nbytes = orbfe.lba_scratch_bytes(4, CAP, len(okf), 0, 0)
    d = dict(kf_fixed=Dev(fixed), obs_offset=Dev(off), obs_kf=Dev(okf), obs_feature=Dev(feat), erase=Out(np.full(len(okf), 7, np.uint8)),
             res=Out(np.zeros(1, orbfe.LBA_RESULT_DTYPE)), scratch=Out(np.zeros(nbytes, np.uint8)))
    ptr = {k: v.ptr for k, v in d.items()}
    ptr.update(Tcw=b.T.ptr, x3Dw=b.x.ptr, kps=b.kps.ptr, scratch_bytes=nbytes)
    chain(b)
    orbfe.local_bundle_adjustment_device(ptr, 4, CAP, len(okf), 0, 0, nc.K4, sig, 25.0, 0, capacity=CAP)
    d["scratch"].get()
    x_after = b.x.get()
    assert np.array_equal(x_after[0].view(np.uint32), host["x3Dw"].view(np.uint32))
    assert np.array_equal(b.T.get().reshape(-1, 3, 4).view(np.uint32), host["Tcw"].view(np.uint32))
    assert np.array_equal(d["erase"].get(), host["erase"]) and d["res"].get()[0].tobytes() == host["result"].tobytes()
    # the neighbours' blocks of the map state are the chain's, untouched by the bundle adjustment
    assert NP.same_bytes(x_after[1:], alone.x.get()[1:])
