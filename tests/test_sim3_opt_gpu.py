"""GPU: orbfe_optimize_sim3 / orbfe_optimize_sim3_batch_device against the CPU restatement (tests/sim3_opt_ref.cpp) on every case of
tests/sim3_opt_cases.py, the batch call against per-problem host calls (bit for bit, in place too), and the device chain
orbfe_search_by_bow_batch_device -> orbfe_sim3_solve_batch_device -> orbfe_optimize_sim3_batch_device with no host copy in between.

Parity contract: the GPU sums the edges in a fixed parallel order, the restatement in the reference's insertion order, so the
decisions agree exactly -- except where every pair whose flag differs has a restatement chi2 within 1e-6 relative of th2 at some
check (such a case is reported as not compared; at most 10 % of the cases) -- and the similarity agrees within 10 times the spread
that summation order alone causes between the restatement's two orders, measured on the CPU (tests/sim3_opt_parity.py; the margin
is for the device's libm).  The agreement with the restatement in the device's own order is measured too and must lie inside it."""
import ctypes as C

import numpy as np
import pytest

import sim3_cases
import sim3_opt_build as B
import sim3_opt_cases as S
import sim3_opt_parity as P
import voc_cases
from orb_slam2_aruco_amd import synth
from pose_opt_device import Dev

pytestmark = pytest.mark.gpu


def _gpu(orbfe, pb, out=None, fix_scale=None, match12=None):
    return orbfe.optimize_sim3((pb["kps1"], pb["x3Dw1"], pb["valid1"], pb["Tcw1"], pb["K4_1"]),
                               (pb["kps2"], pb["x3Dw2"], pb["valid2"], pb["Tcw2"], pb["K4_2"]), pb["m12"] if match12 is None else match12,
                               pb["inv_sigma2"], pb["s12_0"], pb["R12_0"], pb["t12_0"], pb["th2"],
                               pb["fix_scale"] if fix_scale is None else fix_scale, match12_out=out)


def test_optimize_sim3_matches_the_restatement(orbfe):
    spread = P.order_spread()
    tol = tuple(10 * v for v in spread["max"])
    excluded, compared, worst_ins, worst_dev = [], 0, [0.0] * 3, [0.0] * 3
    for name in S.CASES:
        pb = S.case(name)
        ref, dev = P.reference(name, B.INSERTION), P.reference(name, B.DEVICE)
        m12, res = _gpu(orbfe, pb)
        assert res["status"] == 0 and ref["rc"] == 0
        verdict, diff = P.decisions(res, m12, ref)
        print("%-26s N %4d bad %4d more %2d in %4d it %s stale %d: %s" % (name, res["n_correspondences"], res["n_bad"], res["more_iterations"],
                                                                       res["n_inliers"], res["iterations"], res["stale_mask"], verdict))
        if verdict == "near gate":
            excluded.append(name)
            continue
        assert verdict == "same", (name, diff[:10], res, ref["result"])
        compared += 1
        d_ins = S.similarity_difference(res, ref["result"], pb["extent"])
        worst_ins = [max(a, b) for a, b in zip(worst_ins, d_ins)]
        assert all(d <= t for d, t in zip(d_ins, tol)), (name, d_ins, tol)
        if P.decisions(dev["result"], dev["match12"], ref)[0] == "same":
            d_dev = S.similarity_difference(res, dev["result"], pb["extent"])
            worst_dev = [max(a, b) for a, b in zip(worst_dev, d_dev)]
    print("OptimizeSim3 parity (max|dR|, ds/s, |dt|/extent): CPU order spread %.2e %.2e %.2e; tolerance = 10 x that; "
          "GPU vs insertion order %.2e %.2e %.2e; GPU vs device order %.2e %.2e %.2e; %d compared, not compared: %s"
          % (spread["max"] + tuple(worst_ins) + tuple(worst_dev) + (compared, excluded)))
    assert len(excluded) <= 0.1 * len(S.CASES), excluded
    assert all(d <= t for d, t in zip(worst_dev, tol)), (worst_dev, tol)     # the tolerance is not below the measured agreement


def test_noise_free_scene_keeps_every_correspondence(orbfe):
    pb = S.case("n100_clean_s07")
    m12, res = _gpu(orbfe, pb)
    assert res["n_inliers"] == res["n_correspondences"] == 100 and res["n_bad"] == 0 and res["more_iterations"] == 5
    assert np.array_equal(m12, pb["m12"]) and abs(res["s12"] - 0.7) < 1e-6


def test_early_return_leaves_the_similarity(orbfe):
    for name in ("n0", "n9_clean", "n10_one_outlier"):
        pb = S.case(name)
        ref = P.reference(name)
        m12, res = _gpu(orbfe, pb)
        assert res["n_inliers"] == 0 and res["more_iterations"] == 0
        # the given similarity, bit for bit what the restatement hands back
        assert res["s12"] == float(pb["s12_0"]) and res["q12"].tobytes() == ref["result"]["q12"].tobytes()
        assert res["t12"].tobytes() == pb["t12_0"].astype(np.float64).tobytes()
        assert np.array_equal(m12, ref["match12"])


def test_host_call_in_place_and_argument_errors(orbfe):
    pb = S.case("n64_fix_novalid")
    want, wres = _gpu(orbfe, pb)
    m = pb["m12"].copy()
    got, gres = _gpu(orbfe, pb, out=m, match12=m)
    assert got is m and np.array_equal(m, want) and gres.tobytes() == wres.tobytes()
    for key, val in (("th2", 0.0), ("th2", -1.0), ("th2", np.nan), ("s12_0", np.inf)):
        bad = dict(pb); bad[key] = val
        with pytest.raises(orbfe.OrbfeError):
            _gpu(orbfe, bad)
    bad = dict(pb); bad["R12_0"] = pb["R12_0"].copy(); bad["R12_0"][1, 1] = np.nan
    with pytest.raises(orbfe.OrbfeError):
        _gpu(orbfe, bad)
    bad = dict(pb); bad["m12"] = pb["m12"].copy(); bad["m12"][0] = len(pb["kps2"])
    with pytest.raises(orbfe.OrbfeError):
        _gpu(orbfe, bad)


def test_projection_through_z_zero(orbfe):
    """finite inputs whose mapped points land at z = 0 at the initial similarity: the decisions of the restatement, which follows
    the rule of the header (skipped in that pass; never an inlier)"""
    tol = tuple(10 * v for v in P.order_spread()["max"])
    pb = S.degenerate_problem(40, 1)
    ref = B.optimize_sim3(pb)
    m12, res = _gpu(orbfe, pb)
    assert m12[0] == -1 and np.array_equal(m12, ref["match12"]) and all(res[f] == ref["result"][f] for f in P.DECISIONS)
    assert all(d <= t for d, t in zip(S.similarity_difference(res, ref["result"], pb["extent"]), tol))
    pb = S.degenerate_problem(0, 3)
    ref = B.optimize_sim3(pb)
    m12, res = _gpu(orbfe, pb)
    assert res["n_bad"] == 3 and res["n_inliers"] == 0 and res["iterations"][0] == 1 and (m12 == -1).all()
    assert res.tobytes() == ref["result"].tobytes()


def test_bad_octave_is_invalid(orbfe):
    pb = S.case("n64_free")
    i = int(np.flatnonzero(pb["good"])[0])
    pb["kps1"] = pb["kps1"].copy(); pb["kps1"]["octave"][i] = -1
    with pytest.raises(orbfe.OrbfeError):
        _gpu(orbfe, pb)


def _batch_inputs(problems, cap):
    """frames 2 p and 2 p + 1 hold problem p's keyframes"""
    F = 2 * len(problems)
    kps = np.zeros((F, cap), B.KP_DTYPE); X = np.zeros((F, cap, 3), np.float32); valid = np.zeros((F, cap), np.uint8)
    n = np.zeros(F, np.int32); T = np.zeros((F, 12), np.float32)
    m12 = np.full((len(problems), cap), -9, np.int32); sim = np.zeros((len(problems), 13), np.float32)
    for p, pb in enumerate(problems):
        for side, f in (("1", 2 * p), ("2", 2 * p + 1)):
            k = len(pb["kps" + side])
            kps[f, :k] = pb["kps" + side]; X[f, :k] = pb["x3Dw" + side]
            valid[f, :k] = 1 if pb["valid" + side] is None else pb["valid" + side]
            n[f] = k; T[f] = pb["Tcw" + side].reshape(12)
        m12[p, :len(pb["m12"])] = pb["m12"]
        sim[p] = np.r_[pb["s12_0"], pb["R12_0"].ravel(), pb["t12_0"]]
    p1 = np.arange(0, F, 2, dtype=np.int32)
    return kps, X, valid, n, T, m12, sim, p1, p1 + 1


def _empty(pb):
    e = dict(pb)
    for side in "12":
        e.update({"kps" + side: pb["kps" + side][:0], "x3Dw" + side: pb["x3Dw" + side][:0],
                  "valid" + side: None if pb["valid" + side] is None else pb["valid" + side][:0]})
    e["m12"] = pb["m12"][:0]
    return e


def test_batch_equals_host_calls_bit_for_bit(orbfe):
    """a ragged batch with an empty problem and one that returns early, out of place and in place; the sentinels past d_n stay"""
    names = ["n257_out30", "n10_one_outlier", "n64_free", "n1000_out30", "n9_clean", "n300_out60"]
    problems = [S.case(nm) for nm in names]
    problems.insert(2, _empty(S.case("n64_free")))
    cap = max(max(len(p["kps1"]), len(p["kps2"])) for p in problems) + 3
    kps, X, valid, n, T, m12, sim, p1, p2 = _batch_inputs(problems, cap)
    NP = len(problems)
    d_kps, d_X, d_valid, d_n, d_T, d_sim, d_p1, d_p2 = Dev(kps), Dev(X), Dev(valid), Dev(n), Dev(T), Dev(sim), Dev(p1), Dev(p2)
    want = [_gpu(orbfe, pb, fix_scale=False) for pb in problems]
    assert sum(w[1]["more_iterations"] == 0 for w in want) >= 3 and sum(w[1]["n_inliers"] > 0 for w in want) >= 3
    for inplace in (False, True):
        d_in = Dev(m12)
        d_out = d_in if inplace else Dev(np.full_like(m12, -9))
        d_res = Dev(np.zeros(NP, orbfe.SIM3_OPT_RESULT_DTYPE))
        orbfe.optimize_sim3_batch_device(d_kps.ptr, d_n.ptr, cap, d_X.ptr, d_valid.ptr, d_T.ptr, d_p1.ptr, d_p2.ptr, NP, d_in.ptr,
                                         sim3_cases.K4, S.INV_SIGMA2, d_sim.ptr, 52, S.TH2, False, d_out.ptr, d_res.ptr, None)
        gres = d_res.get(); gout = d_out.get()
        for p, (pb, (wm, wres)) in enumerate(zip(problems, want)):
            k = len(pb["kps1"])
            assert gres[p].tobytes() == wres.tobytes(), (inplace, p, gres[p], wres)
            assert np.array_equal(gout[p, :k], wm), (inplace, p)
            assert (gout[p, k:] == -9).all(), (inplace, p)          # sentinel kept
        if not inplace:
            assert np.array_equal(d_in.get(), m12)                  # the input is only read


def test_batch_without_valid_flags_equals_host_calls(orbfe):
    """d_valid = NULL (every feature has a good map point) against host calls with valid = None"""
    problems = [S.case(nm) for nm in ("n64_fix_novalid", "n300_free_out30_novalid", "n100_clean_s1")]
    assert all(p["valid1"] is None and p["valid2"] is None for p in problems)
    cap = max(max(len(p["kps1"]), len(p["kps2"])) for p in problems) + 1
    kps, X, _, n, T, m12, sim, p1, p2 = _batch_inputs(problems, cap)
    d_kps, d_X, d_n, d_T, d_sim, d_p1, d_p2 = Dev(kps), Dev(X), Dev(n), Dev(T), Dev(sim), Dev(p1), Dev(p2)
    d_in, d_out, d_res = Dev(m12), Dev(np.full_like(m12, -9)), Dev(np.zeros(3, orbfe.SIM3_OPT_RESULT_DTYPE))
    orbfe.optimize_sim3_batch_device(d_kps.ptr, d_n.ptr, cap, d_X.ptr, None, d_T.ptr, d_p1.ptr, d_p2.ptr, 3, d_in.ptr,
                                     sim3_cases.K4, S.INV_SIGMA2, d_sim.ptr, 52, S.TH2, False, d_out.ptr, d_res.ptr, None)
    res, out = d_res.get(), d_out.get()
    for p, pb in enumerate(problems):
        wm, wres = _gpu(orbfe, pb, fix_scale=False)
        assert wres["n_inliers"] > 0 and res[p].tobytes() == wres.tobytes(), (p, res[p], wres)
        assert np.array_equal(out[p, :len(wm)], wm) and (out[p, len(wm):] == -9).all(), p


def test_batch_skips_a_problem_with_a_bad_octave(orbfe):
    problems = [S.case("n64_free"), S.case("n40_noisy"), S.case("n11_one_outlier")]
    i = int(np.flatnonzero(problems[1]["good"])[0])
    problems[1]["kps2"] = problems[1]["kps2"].copy(); problems[1]["kps2"]["octave"][problems[1]["m12"][i]] = 99
    cap = max(max(len(p["kps1"]), len(p["kps2"])) for p in problems)
    kps, X, valid, n, T, m12, sim, p1, p2 = _batch_inputs(problems, cap)
    d_kps, d_X, d_valid, d_n, d_T, d_sim, d_p1, d_p2 = Dev(kps), Dev(X), Dev(valid), Dev(n), Dev(T), Dev(sim), Dev(p1), Dev(p2)
    d_in, d_out, d_res = Dev(m12), Dev(np.full_like(m12, -9)), Dev(np.zeros(3, orbfe.SIM3_OPT_RESULT_DTYPE))
    orbfe.optimize_sim3_batch_device(d_kps.ptr, d_n.ptr, cap, d_X.ptr, d_valid.ptr, d_T.ptr, d_p1.ptr, d_p2.ptr, 3, d_in.ptr,
                                     sim3_cases.K4, S.INV_SIGMA2, d_sim.ptr, 52, S.TH2, False, d_out.ptr, d_res.ptr, None)
    res, out = d_res.get(), d_out.get()
    assert res[1]["status"] == -1 and not any(res[1][f].any() for f in res.dtype.names if f != "status")
    assert (out[1] == -9).all()
    for p in (0, 2):
        wm, wres = _gpu(orbfe, problems[p], fix_scale=False)
        assert res[p].tobytes() == wres.tobytes() and np.array_equal(out[p, :len(wm)], wm)
    # a capacity whose staged problem cannot fit a workgroup's LDS is refused before anything is launched
    with pytest.raises(orbfe.OrbfeError):
        orbfe.optimize_sim3_batch_device(d_kps.ptr, d_n.ptr, 20000, d_X.ptr, d_valid.ptr, d_T.ptr, d_p1.ptr, d_p2.ptr, 3, d_in.ptr,
                                         sim3_cases.K4, S.INV_SIGMA2, d_sim.ptr, 52, S.TH2, False, d_out.ptr, d_res.ptr, None)
    assert orbfe.load().orbfe_last_error().find(b"LDS") >= 0


def test_device_chain_bow_sim3_optimize(orbfe):
    """orbfe_search_by_bow_batch_device -> orbfe_sim3_solve_batch_device -> orbfe_optimize_sim3_batch_device on one stream, the
    similarity read straight from the solver's records through the stride: equal bit for bit to the chain through host calls"""
    L = orbfe.load()
    nf, npairs, iters = 5, 6, 300
    ex = orbfe.ORBextractor(1000, 1.2, 8, 20, 7)
    frames = [ex(f) for f in synth.stream(480, 640, nf, 2024)]
    voc = voc_cases.make(10, 4, 41, irregular=False)
    gvoc = orbfe.ORBVocabulary.from_arrays(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    cap = max(len(k) for k, _ in frames) + 3
    rng = np.random.default_rng(6)
    K4 = sim3_cases.K4
    kps = np.zeros((nf, cap), orbfe.KP_DTYPE); desc = np.zeros((nf, cap, 32), np.uint8); nk = np.zeros(nf, np.int32)
    fn = np.zeros((nf, cap), np.uint32); fo = np.zeros((nf, cap + 1), np.int32); ff = np.zeros((nf, cap), np.uint32); nfv = np.zeros(nf, np.int32)
    x3Dw = np.zeros((nf, cap, 3), np.float32); valid = np.zeros((nf, cap), np.uint8); Tcw = np.zeros((nf, 3, 4), np.float32)
    for f, (k, d) in enumerate(frames):
        n = len(k)
        kps[f, :n] = k; desc[f, :n] = d; nk[f] = n
        fv = gvoc.transform(d, 4)["fv"]
        nfv[f] = len(fv[0]); fn[f, :nfv[f]] = fv[0]; fo[f, :nfv[f] + 1] = fv[1]; ff[f, :len(fv[2])] = fv[2]
        R, t = sim3_cases._pose(rng, rng.uniform(0, 180), 3.0)
        Tcw[f] = np.c_[R, t]
        Xc = np.c_[(np.stack([k["x"], k["y"]], 1) - K4[2:]) / K4[:2], np.ones(n)] * 5.0
        x3Dw[f, :n] = (Xc - t) @ R
        valid[f, :n] = rng.random(n) > 0.1
    pairs = [(p % nf, (p + 1 + p // nf) % nf) for p in range(npairs)]
    p1 = np.array([a for a, _ in pairs], np.int32); p2 = np.array([b for _, b in pairs], np.int32)
    words = np.stack([sim3_cases.words(iters, 900 + p) for p in range(npairs)])
    m12_0 = np.full((npairs, cap), -1, np.int32)
    d_kps, d_desc, d_valid, d_n = Dev(kps), Dev(desc), Dev(valid), Dev(nk)
    d_fn, d_fo, d_ff, d_nfv = Dev(fn), Dev(fo), Dev(ff), Dev(nfv)
    d_p1, d_p2, d_m12, d_m21, d_nm = Dev(p1), Dev(p2), Dev(m12_0), Dev(m12_0), Dev(np.zeros(npairs, np.int32))
    d_x, d_T, d_w = Dev(x3Dw), Dev(Tcw), Dev(words)
    d_res, d_inl = Dev(np.zeros(npairs, orbfe.SIM3_RESULT_DTYPE)), Dev(np.zeros((npairs, cap), np.uint8))
    d_out, d_ores = Dev(np.full((npairs, cap), -9, np.int32)), Dev(np.zeros(npairs, orbfe.SIM3_OPT_RESULT_DTYPE))
    rc = L.orbfe_search_by_bow_batch_device(d_kps.ptr, d_desc.ptr, d_valid.ptr, d_n.ptr, d_fn.ptr, d_fo.ptr, d_ff.ptr, d_nfv.ptr, cap,
                                            d_p1.ptr, d_p2.ptr, npairs, 1, 0.75, 1, 49, np.float32(1.0 / 30), d_m12.ptr, d_m21.ptr,
                                            d_nm.ptr, None)
    assert rc == 0, L.orbfe_last_error()
    orbfe.sim3_solve_batch_device(d_kps.ptr, d_n.ptr, cap, d_x.ptr, d_valid.ptr, d_T.ptr, d_p1.ptr, d_p2.ptr, npairs, d_m12.ptr, K4,
                                  sim3_cases.LEVEL_SIGMA2, False, 0.99, 20, iters, d_w.ptr, d_res.ptr, d_inl.ptr, None)
    orbfe.optimize_sim3_batch_device(d_kps.ptr, d_n.ptr, cap, d_x.ptr, d_valid.ptr, d_T.ptr, d_p1.ptr, d_p2.ptr, npairs, d_m12.ptr, K4,
                                     S.INV_SIGMA2, d_res.ptr + orbfe.SIM3_RESULT_S12_OFFSET, orbfe.SIM3_RESULT_DTYPE.itemsize, S.TH2,
                                     False, d_out.ptr, d_ores.ptr, None)
    m12, res, out, ores = d_m12.get(), d_res.get(), d_out.get(), d_ores.get()
    for p, (a, b) in enumerate(pairs):
        na, nb = nk[a], nk[b]
        side1, side2 = (kps[a, :na], x3Dw[a, :na], valid[a, :na], Tcw[a], K4), (kps[b, :nb], x3Dw[b, :nb], valid[b, :nb], Tcw[b], K4)
        sol = orbfe.Sim3Solver(side1, side2, m12[p, :na], sim3_cases.LEVEL_SIGMA2, False)
        sol.set_ransac_parameters(0.99, 20, iters)
        r, _ = sol.solve(0, iters, 0, words[p])
        assert res[p].tobytes() == r.tobytes(), p
        wm, wres = orbfe.optimize_sim3(side1, side2, m12[p, :na], S.INV_SIGMA2, r["s12"], r["R12"], r["t12"], S.TH2, False)
        assert ores[p].tobytes() == wres.tobytes(), (p, ores[p], wres)
        assert np.array_equal(out[p, :na], wm) and (out[p, na:] == -9).all(), p
    print("chain: N %s, found %s, optimizer: correspondences %s, inliers %s" % (res["n"].tolist(), res["found"].tolist(),
                                                                              ores["n_correspondences"].tolist(), ores["n_inliers"].tolist()))
    assert (res["found"] >= 0).any() and (ores["n_correspondences"] > 0).any()
