"""GPU parity of orbfe_sim3_* (csrc/sim3_solver.hip) against the CPU restatement of ORB_SLAM2::Sim3Solver (tests/sim3_ref.cpp).
The contract, with the tolerances of the initializer's (tests/test_initializer_gpu.py; float arithmetic, independent eigen code on
the two sides):
  1. N, indices1 and the sets are equal; X3Dc*, P*im*, maxError* are bit-exact.
  2. Per hypothesis R12 to 1e-4 absolute, s12 to 1e-4 relative, t12 to 1e-4 of the cloud's extent, for every hypothesis whose N
     matrix has well separated leading eigenvalues on the restatement's side, (l1 - l2) > 0.03 |l1|; the excluded share is printed
     and capped at 15 %.
  3. Inlier counts of the compared hypotheses are equal except through correspondences whose err1 or err2 (float64, from the
     restatement's model) lies within 1e-4 relative of its maxError; the winner's differing flags are checked one by one.
  4. found, n_inliers, no_more, best are equal wherever the scan's decisions are clear on the restatement's side
     (sim3_parity.decision_reason); each case prints whether it was compared, and the outlier-free and 30 % cases at N >= 100 must be.
  5. Sixty iterate(5)-shaped calls with the carried best equal one whole run bit for bit.
  6. The batch call over 16 pairs, chained after orbfe_search_by_bow_batch_device, equals 16 host-pointer calls bit for bit.
  7. Argument errors and the defined corner cases."""

import numpy as np
import pytest

import sim3_build as B
import sim3_cases as S
import sim3_parity as P
import voc_cases
from orb_slam2_aruco_amd import synth

pytestmark = pytest.mark.gpu


def _solver(orbfe, sc):
    return orbfe.Sim3Solver((sc["kps1"], sc["x3Dw1"], sc["valid1"], sc["Tcw1"], sc["K4_1"]),
                            (sc["kps2"], sc["x3Dw2"], sc["valid2"], sc["Tcw2"], sc["K4_2"]), sc["m12"], sc["level_sigma2"], sc["fix_scale"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_parity_with_the_restatement(orbfe, c):
    name = S.case_id(c)
    sc = S.case_scene(c)
    prob, min_inl, max_it = S.ransac_of(c)
    w = S.case_words(c)
    sol = _solver(orbfe, sc)
    sol.set_ransac_parameters(prob, min_inl, max_it)
    got = sol.inspect(0, max_it, 0, w)
    want = B.solve(sc, prob, min_inl, max_it, words=w)
    gr, wr = got["result"], want["result"]
    # 1. the constructor and the sets
    assert got["N"] == want["N"] == c[0] == gr["n"]
    assert gr["max_iterations"] == wr["max_iterations"]
    assert np.array_equal(got["indices1"], want["indices1"])
    assert np.array_equal(got["sets"], want["sets"])
    for f in ("X3Dc1", "X3Dc2", "P1im1", "P2im2", "maxError1", "maxError2"):
        assert np.array_equal(_bits(got[f]), _bits(want[f])), f
    k = P.ran(want, min_inl, max_it)
    if k == 0:
        assert gr["no_more"] == wr["no_more"] == 1 and gr["found"] == -1 and gr["best"] == -1 and not got["inliers12"].any()
        assert not got["counts"].any()
        print("%s: nothing to run (N = %d, min_inliers = %d)" % (name, c[0], min_inl))
        return
    # 2. the models of the compared hypotheses
    ok = P.compared(want, k)
    share = 1.0 - ok.mean()
    print("%s: %d hypotheses, excluded share %.3f" % (name, k, share))
    assert share <= P.CAP
    dR = np.abs(got["R12"][:k].astype(np.float64) - want["R12"][:k]).reshape(k, -1).max(axis=1)
    ds = np.abs(got["s12"][:k].astype(np.float64) - want["s12"][:k]) / np.abs(want["s12"][:k].astype(np.float64))
    dt = np.abs(got["t12"][:k].astype(np.float64) - want["t12"][:k]).max(axis=1) / sc["extent"]
    print("%s: compared hypotheses: max |dR| %.2e, max ds/s %.2e, max |dt|/extent %.2e" % (name, dR[ok].max(), ds[ok].max(), dt[ok].max()))
    assert (dR[ok] <= 1e-4).all(), (np.flatnonzero(ok & (dR > 1e-4)), dR[ok].max())
    assert (ds[ok] <= 1e-4).all(), (np.flatnonzero(ok & (ds > 1e-4)), ds[ok].max())
    assert (dt[ok] <= 1e-4).all(), (np.flatnonzero(ok & (dt > 1e-4)), dt[ok].max())
    # 3. the inlier counts
    near = P.near_gate(want, sc, k)
    dc = np.abs(got["counts"][:k].astype(np.int64) - want["counts"][:k])
    assert (dc[ok] <= near.sum(axis=1)[ok]).all(), np.flatnonzero(ok & (dc > near.sum(axis=1)))
    print("%s: %d compared hypotheses differ in their count, all through correspondences near a gate" % (name, int((dc[ok] > 0).sum())))
    # 4. the decision
    why = P.decision_reason(want, sc, min_inl, max_it)
    print("%s: decision %s" % (name, "compared" if why is None else "not compared (%s)" % why))
    if c[0] >= 100 and c[2] <= 0.3:
        assert why is None, why
    if why is None:
        for f in ("found", "n_inliers", "no_more", "best", "best_inliers"):
            assert gr[f] == wr[f], (f, gr[f], wr[f])
        if wr["best"] >= 0:
            b = int(wr["best"])
            assert np.array_equal(_bits(gr["R12"]), _bits(got["R12"][b]).ravel()) and np.array_equal(_bits(gr["t12"]), _bits(got["t12"][b]))
            assert _bits(gr["s12"]) == _bits(got["s12"][b])
            T = gr["T12"].reshape(4, 4)
            assert np.array_equal(T[:3, 3], gr["t12"]) and np.array_equal(T[3], [0, 0, 0, 1])
            assert np.array_equal(_bits(T[:3, :3]), _bits(np.float32(gr["s12"]) * gr["R12"].reshape(3, 3)))
        diff = np.flatnonzero(got["inliers12"] != want["inliers12"])
        if wr["found"] >= 0:
            pos = {int(i1): j for j, i1 in enumerate(want["indices1"])}
            for i1 in diff:
                assert near[int(wr["found"]), pos[int(i1)]], i1
        else:
            assert len(diff) == 0 and not got["inliers12"].any()
    # the plain call returns what the inspecting one returns
    r2, inl2 = sol.solve(0, max_it, 0, w)
    assert r2.tobytes() == gr.tobytes() and np.array_equal(inl2, got["inliers12"])


@pytest.mark.parametrize("c", [(100, 1.3, 0.6, False), (100, 1.0, 0.3, True), (40, 1.3, 0.3, False), (1000, 0.7, 0.6, False)], ids=S.case_id)
def test_window_calls_equal_one_whole_run(orbfe, c):
    """5. iterate(5) sixty times through the class (which carries mnIterations and mnBestInliers) against one find()-shaped call."""
    sc = S.case_scene(c, seed=4)
    w = S.words(300, 7)
    sol = _solver(orbfe, sc)
    sol.set_ransac_parameters(*S.RANSAC)
    whole, whole_inl = sol.solve(0, 300, 0, w)
    hit = None
    for call in range(60):
        it = sol.iterations
        T, no_more, inl, n = sol.iterate(5, w[3 * it:3 * it + 15])
        if T is not None:
            hit = (sol.last, inl)
            break
        if no_more:
            break
    if whole["found"] >= 0:
        assert hit is not None
        for f in ("found", "n_inliers", "best", "best_inliers", "s12", "R12", "t12", "T12", "no_more", "n", "max_iterations"):
            assert np.array_equal(np.asarray(hit[0][f]).view(np.uint32), np.asarray(whole[f]).view(np.uint32)), f
        assert np.array_equal(hit[1], whole_inl)
        assert sol.iterations == whole["found"] + 1
    else:
        assert hit is None and no_more and whole["no_more"] == 1
        assert sol.best_inliers == whole["best_inliers"]
        assert np.array_equal(_bits(sol.T12), _bits(whole["T12"].reshape(4, 4))) and sol.iterations == whole["max_iterations"]
    print("%s: found %d after %d calls" % (S.case_id(c), whole["found"], call + 1))


def test_batch_device_equals_per_pair_calls(orbfe):
    """6. orbfe_sim3_solve_batch_device over 16 pairs, chained after orbfe_search_by_bow_batch_device on the same stream (frames of
    the synthetic stream, a small synthetic vocabulary, made-up world points: every keypoint back-projected to a plane in front of its
    camera), equals one orbfe_sim3_solve per pair bit for bit, padding untouched.  Device memory from the library's own allocator."""
    L = orbfe.load()
    held = []

    def dev(arr):
        arr = np.ascontiguousarray(arr)
        d = L.orbfe_device_alloc(0, arr.nbytes)
        assert d, L.orbfe_last_error()
        held.append(d)
        assert L.orbfe_device_upload_rows(d, arr.nbytes, arr.ctypes.data, arr.nbytes, arr.nbytes, 1) == 0, L.orbfe_last_error()
        return d

    def host(d, like):
        out = np.empty_like(like)
        assert L.orbfe_device_download(out.ctypes.data, d, out.nbytes) == 0, L.orbfe_last_error()
        return out

    nf, npairs, iters = 9, 16, 300
    ex = orbfe.ORBextractor(1000, 1.2, 8, 20, 7)
    frames = [ex(f) for f in synth.stream(480, 640, nf, 2024)]
    voc = voc_cases.make(10, 4, 41, irregular=False)
    gvoc = orbfe.ORBVocabulary.from_arrays(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    cap = max(len(k) for k, _ in frames) + 3
    rng = np.random.default_rng(6)
    kps = np.zeros((nf, cap), orbfe.KP_DTYPE); desc = np.zeros((nf, cap, 32), np.uint8); nk = np.zeros(nf, np.int32)
    fn = np.zeros((nf, cap), np.uint32); fo = np.zeros((nf, cap + 1), np.int32); ff = np.zeros((nf, cap), np.uint32); nfv = np.zeros(nf, np.int32)
    x3Dw = np.zeros((nf, cap, 3), np.float32); valid = np.zeros((nf, cap), np.uint8); Tcw = np.zeros((nf, 3, 4), np.float32)
    for f, (k, d) in enumerate(frames):
        n = len(k)
        kps[f, :n] = k; desc[f, :n] = d; nk[f] = n
        fv = gvoc.transform(d, 4)["fv"]
        nfv[f] = len(fv[0]); fn[f, :nfv[f]] = fv[0]; fo[f, :nfv[f] + 1] = fv[1]; ff[f, :len(fv[2])] = fv[2]
        R, t = S._pose(rng, rng.uniform(0, 180), 3.0)
        Tcw[f] = np.c_[R, t]
        Xc = np.c_[(np.stack([k["x"], k["y"]], 1) - S.K4[2:]) / S.K4[:2], np.ones(n)] * 5.0
        x3Dw[f, :n] = (Xc - t) @ R
        valid[f, :n] = rng.random(n) > 0.1
    pairs = [(p % nf, (p + 1 + p // nf) % nf) for p in range(npairs)]
    p1 = np.array([a for a, _ in pairs], np.int32); p2 = np.array([b for _, b in pairs], np.int32)
    words = np.stack([S.words(iters, 900 + p) for p in range(npairs)])
    m12_0 = np.full((npairs, cap), -1, np.int32)
    res_0 = np.zeros(npairs, orbfe.SIM3_RESULT_DTYPE)
    inl_0 = np.full((npairs, cap), 9, np.uint8)
    try:
        d_kps, d_desc, d_valid, d_n = dev(kps), dev(desc), dev(valid), dev(nk)
        d_fn, d_fo, d_ff, d_nfv = dev(fn), dev(fo), dev(ff), dev(nfv)
        d_p1, d_p2, d_m12, d_m21, d_nm = dev(p1), dev(p2), dev(m12_0), dev(m12_0), dev(np.zeros(npairs, np.int32))
        d_x, d_T, d_w, d_res, d_inl = dev(x3Dw), dev(Tcw), dev(words), dev(res_0), dev(inl_0)
        rc = L.orbfe_search_by_bow_batch_device(d_kps, d_desc, d_valid, d_n, d_fn, d_fo, d_ff, d_nfv, cap, d_p1, d_p2, npairs, 1, 0.75, 1, 49,
                                                np.float32(1.0 / 30), d_m12, d_m21, d_nm, None)
        assert rc == 0, L.orbfe_last_error()
        orbfe.sim3_solve_batch_device(d_kps, d_n, cap, d_x, d_valid, d_T, d_p1, d_p2, npairs, d_m12, S.K4, S.LEVEL_SIGMA2, False, 0.99, 20,
                                      iters, d_w, d_res, d_inl, None)
        res = host(d_res, res_0); m12 = host(d_m12, m12_0); inl = host(d_inl, inl_0)
    finally:
        for d in held:
            L.orbfe_device_free(d)
    assert (res["n"] >= 20).sum() >= npairs // 2, res["n"]
    for p, (a, b) in enumerate(pairs):
        na, nb = nk[a], nk[b]
        sol = orbfe.Sim3Solver((kps[a, :na], x3Dw[a, :na], valid[a, :na], Tcw[a], S.K4), (kps[b, :nb], x3Dw[b, :nb], valid[b, :nb], Tcw[b], S.K4),
                               m12[p, :na], S.LEVEL_SIGMA2, False)
        sol.set_ransac_parameters(0.99, 20, iters)
        r, flags = sol.solve(0, iters, 0, words[p])
        assert res[p].tobytes() == r.tobytes(), (p, res[p], r)
        assert np.array_equal(inl[p, :na], flags.astype(np.uint8)), p
        assert (inl[p, na:] == 9).all(), p
    print("batch: N %s, found %s" % (res["n"].tolist(), res["found"].tolist()))
    assert (res["found"] >= 0).any()


def test_argument_errors_and_corner_cases(orbfe):
    """7."""
    sc = S.scene(100, 1.3, 0.0, False, seed=5)
    w = S.words(300, 5)
    sol = _solver(orbfe, sc)
    sol.set_ransac_parameters(*S.RANSAC)
    ok, _ = sol.solve(0, 300, 0, w)
    assert ok["status"] == 0 and ok["n"] == 100
    kept = np.flatnonzero((sc["m12"] >= 0) & (sc["valid1"] != 0))
    kept = kept[sc["valid2"][sc["m12"][kept]] != 0]
    # a match past keyframe 2
    bad = dict(sc); bad["m12"] = sc["m12"].copy(); bad["m12"][kept[0]] = len(sc["kps2"])
    with pytest.raises(orbfe.OrbfeError):
        _solver(orbfe, bad).solve(0, 300, 0, w)
    bad["m12"][kept[0]] = -2
    with pytest.raises(orbfe.OrbfeError):
        _solver(orbfe, bad).solve(0, 300, 0, w)
    # an octave outside the level table on a kept correspondence; the same octave on a dropped one is not looked at
    bad = dict(sc); bad["kps1"] = sc["kps1"].copy(); bad["kps1"]["octave"][kept[3]] = 8
    with pytest.raises(orbfe.OrbfeError):
        _solver(orbfe, bad).solve(0, 300, 0, w)
    with pytest.raises(ValueError):
        B.solve(bad, *S.RANSAC, words=w)
    free = np.flatnonzero(sc["m12"] < 0)
    fine = dict(sc); fine["kps1"] = sc["kps1"].copy(); fine["kps1"]["octave"][free[0]] = 99
    s2 = _solver(orbfe, fine); s2.set_ransac_parameters(*S.RANSAC)
    assert s2.solve(0, 300, 0, w)[0].tobytes() == ok.tobytes()
    # a negative word; words past the window are not read
    wn = w.copy(); wn[10] = -1
    with pytest.raises(orbfe.OrbfeError):
        sol.solve(0, 300, 0, wn)
    with pytest.raises(orbfe.OrbfeError):
        sol.solve(0, 0, 0, w[:0])
    with pytest.raises(orbfe.OrbfeError):
        sol.solve(0, 5, -1, w[:15])
    L = orbfe.load()
    res = np.zeros(1, orbfe.SIM3_RESULT_DTYPE)
    assert L.orbfe_sim3_solve(None, 5, None, None, None, None, None, 5, None, None, None, None, None, None, 8, 0, 0.99, 20, 300, 0, 300, 0,
                              None, res.ctypes.data, None, 0) == -1
    assert L.orbfe_sim3_solve_batch_device(None, None, 0, None, None, None, None, None, 1, None, None, None, 8, 0, 0.99, 20, 300, None, None,
                                           None, None) == -1
    # N < min_inliers: bNoMore at once, no word read (a negative word past the check would be an error; the device reads none)
    for N, min_inl in ((19, 20), (2, 2), (0, 0)):
        scn = S.scene(N, 1.3, 0.0, False, seed=6)
        s3 = _solver(orbfe, scn); s3.set_ransac_parameters(0.99, min_inl, 300)
        r, inl = s3.solve(0, 300, 0, w)
        assert r["n"] == N and r["no_more"] == 1 and r["found"] == -1 and r["best"] == -1 and r["n_inliers"] == 0 and not inl.any()
        want = B.solve(scn, 0.99, min_inl, 300, words=w)["result"]
        assert r.tobytes() == want.tobytes()
    # a window at and past the end of the run: nothing runs, no more
    r, inl = sol.solve(int(ok["max_iterations"]), 5, 7, w[:15])
    assert r["no_more"] == 1 and r["found"] == -1 and r["best"] == -1 and r["best_inliers"] == 7 and not inl.any()
    # a hypothesis without rotation (the two clouds equal: the quaternion has no imaginary part): zero inliers, never the best
    same = dict(sc); same["x3Dw2"] = sc["x3Dw1"].copy(); same["Tcw2"] = sc["Tcw1"]; same["kps2"] = sc["kps1"]
    same["valid2"] = sc["valid1"]; same["m12"] = np.where(sc["m12"] >= 0, np.arange(len(sc["m12"])), -1).astype(np.int32)
    same["fix_scale"] = True
    s4 = _solver(orbfe, same); s4.set_ransac_parameters(*S.RANSAC)
    g = s4.inspect(0, 300, 0, w)
    wv = B.solve(same, *S.RANSAC, words=w)
    dead = ~wv["R12"].reshape(300, -1).any(axis=1)
    print("identical clouds: %d of 300 hypotheses have no rotation axis on the restatement's side" % dead.sum())
    gd = ~g["R12"].reshape(300, -1).any(axis=1)
    assert not g["counts"][gd].any() and (g["result"]["best"] < 0 or not gd[g["result"]["best"]])
