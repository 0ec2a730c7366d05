"""GPU: orbfe_pose_optimization / orbfe_pose_optimization_batch_device against the CPU restatement (tests/pose_opt_ref.cpp) on every
case of tests/pose_opt_cases.py, the batch call against per-problem host calls (bit for bit, in place too), and the device chain
batch search (mode 2) -> orbfe_pose_gather_device -> batch pose optimization with no host copy in between.

Parity contract: the GPU sums the edges in a fixed parallel order, the restatement in the reference's insertion order, so the
pose agrees within a tolerance and the decisions agree exactly -- except where an edge whose flag differs has a restatement chi2
within 1e-6 relative of the 5.991 gate in some round (such a case is reported as not compared; at most 10 % of the cases)."""
import ctypes as C

import numpy as np
import pytest

import pose_opt_build as B
from pose_opt_device import Dev
import pose_opt_cases as S

pytestmark = pytest.mark.gpu

GATE = 5.991


def _gpu(orbfe, pb, outlier_init=7):
    out = np.full(len(pb["kps"]), outlier_init, np.uint8)
    T, out, chi2, res = orbfe.pose_optimization(pb["kps"], pb["has_mp"], pb["x3Dw"], pb["inv_sigma2"], pb["K4"], pb["Tcw"],
                                                markers=pb["markers"], marker_info=pb["marker_info"], outlier=out)
    return T, out, chi2, res


def _near_gate(ref, idx):
    c = ref["chi2"][:, idx]
    c = c[np.isfinite(c)]
    return bool(np.any(np.abs(c - GATE) <= 1e-6 * GATE))


def test_pose_optimization_matches_the_restatement(orbfe):
    excluded, stale_cases, compared = [], [], 0
    for name in S.CASES:
        pb = S.case(name)
        ref = B.pose_optimization(pb)
        T, out, chi2, res = _gpu(orbfe, pb)
        rr = ref["result"]
        assert res["status"] == 0 and ref["rc"] == 0
        assert res["n_initial"] == rr["n_initial"] and res["rounds"] == rr["rounds"], name
        assert res["n_marker_edges"] == rr["n_marker_edges"], name
        has = pb["has_mp"] == 1
        assert (out[~has] == 7).all(), name                       # entries without a map point are not written
        diff = np.flatnonzero(has & (out != ref["outlier"]))
        same_counts = res["n_good"] == rr["n_good"] and np.array_equal(res["n_bad"], rr["n_bad"])
        if len(diff) or not same_counts:
            if len(diff) and all(_near_gate(ref, i) for i in diff):
                excluded.append(name)
                print("not compared: %s (%d flags differ next to the gate)" % (name, len(diff)))
                continue
            pytest.fail("%s: decisions differ away from the gate: flags %s, n_bad %s vs %s" % (name, diff[:10], res["n_bad"], rr["n_bad"]))
        compared += 1
        if rr["stale_mask"]:
            stale_cases.append(name)
        # the pose: R and t within 1e-5 (t relative to the scene depth)
        assert np.abs(T[:, :3] - ref["Tcw"][:, :3]).max() <= 1e-5, (name, np.abs(T[:, :3] - ref["Tcw"][:, :3]).max())
        assert np.abs(T[:, 3] - ref["Tcw"][:, 3]).max() <= 1e-5 * pb["depth"], (name, np.abs(T[:, 3] - ref["Tcw"][:, 3]).max())
        # the last classification's chi2, where it was computed
        if rr["rounds"]:
            last = ref["chi2"][rr["rounds"] - 1]
            assert np.allclose(chi2[has], last[has], rtol=1e-4, atol=1e-6), name
    print("pose optimization: %d cases compared, %d not compared; %d compared cases end a round on rejected trials (%s)"
          % (compared, len(excluded), len(stale_cases), ", ".join(stale_cases)))
    assert len(excluded) <= 0.1 * len(S.CASES), excluded
    assert stale_cases, "no case exercised the stale-error quirk"


def test_fewer_than_three_observations_leave_the_pose(orbfe):
    pb = S.case("n2_markers")
    T, out, chi2, res = _gpu(orbfe, pb)
    assert res["n_good"] == 0 and res["n_initial"] == 2 and res["rounds"] == 0
    assert np.array_equal(T, pb["Tcw"])
    assert (out[pb["has_mp"] == 1] == 0).all() and (out[pb["has_mp"] == 0] == 7).all()


def test_bad_octave_is_invalid(orbfe):
    pb = S.case("n60")
    pb["kps"]["octave"][int(np.flatnonzero(pb["has_mp"])[0])] = -1
    with pytest.raises(orbfe.OrbfeError):
        _gpu(orbfe, pb)


def _batch_inputs(problems, cap, mcap):
    F = len(problems)
    kps = np.zeros((F, cap), B.KP_DTYPE); has = np.zeros((F, cap), np.uint8); X = np.zeros((F, cap, 3), np.float32)
    mk = np.zeros((F, mcap), B.MARKER_DTYPE); n = np.zeros(F, np.int32); nm = np.zeros(F, np.int32); T = np.zeros((F, 12), np.float32)
    for f, pb in enumerate(problems):
        k = len(pb["kps"]); m = len(pb["markers"])
        kps[f, :k] = pb["kps"]; has[f, :k] = pb["has_mp"]; X[f, :k] = pb["x3Dw"]; mk[f, :m] = pb["markers"]
        n[f] = k; nm[f] = m; T[f] = pb["Tcw"].reshape(12)
    return kps, has, X, mk, n, nm, T


def test_batch_equals_host_calls_bit_for_bit(orbfe):
    names = ["n500_out10_m3", "n2", "n60_out30_m1", "n2000_out30_m3", "marker_dominated", "clean_true_n500_m1", "n9"]
    problems = [S.case(nm_) for nm_ in names]
    empty = S.case("n5"); empty.update(kps=empty["kps"][:0], has_mp=empty["has_mp"][:0], x3Dw=empty["x3Dw"][:0], markers=empty["markers"][:0])
    problems.insert(3, empty)
    cap = max(len(p["kps"]) for p in problems)
    mcap = 3
    kps, has, X, mk, n, nm, T = _batch_inputs(problems, cap, mcap)
    F = len(problems)
    d_kps, d_has, d_X, d_mk = Dev(kps), Dev(has), Dev(X), Dev(mk)
    d_n, d_nm = Dev(n), Dev(nm)
    want = [_gpu(orbfe, pb) for pb in problems]
    for inplace in (False, True):
        d_Tin = Dev(T)
        d_Tout = d_Tin if inplace else Dev(np.zeros_like(T))
        d_out = Dev(np.full((F, cap), 7, np.uint8))
        d_chi = Dev(np.full((F, cap), np.nan, np.float32))
        d_res = Dev(np.zeros(F, orbfe.POSE_RESULT_DTYPE))
        orbfe.pose_optimization_batch_device(d_kps.ptr, d_n.ptr, cap, F, d_has.ptr, d_X.ptr, d_mk.ptr,
                                             d_nm.ptr, mcap, S.INV_SIGMA2, S.K4, 25.0, d_Tin.ptr, d_Tout.ptr,
                                             d_out.ptr, d_chi.ptr, d_res.ptr, None)
        gT = d_Tout.get().reshape(F, 3, 4)
        gout = d_out.get().reshape(F, cap)
        gchi = d_chi.get().reshape(F, cap)
        gres = d_res.get()
        for f, (pb, (wT, wout, wchi, wres)) in enumerate(zip(problems, want)):
            k = len(pb["kps"])
            assert gres[f].tobytes() == wres.tobytes(), (f, gres[f], wres)
            assert gT[f].tobytes() == wT.tobytes(), f
            assert np.array_equal(gout[f, :k], wout), f
            assert (gout[f, k:] == 7).all() and (gout[f, :k][pb["has_mp"] == 0] == 7).all(), f    # sentinel kept
            h = pb["has_mp"] == 1
            if wres["rounds"]:
                assert gchi[f, :k][h].tobytes() == wchi[h].tobytes(), f
            assert np.isnan(gchi[f, :k][~h]).all()


def test_batch_skips_a_frame_with_a_bad_octave(orbfe):
    problems = [S.case("n60"), S.case("n60_out50")]
    problems[1]["kps"]["octave"][int(np.flatnonzero(problems[1]["has_mp"])[0])] = 99
    cap = max(len(p["kps"]) for p in problems)
    kps, has, X, mk, n, nm, T = _batch_inputs(problems, cap, 1)
    d_T = Dev(T); d_out = Dev(np.full((2, cap), 7, np.uint8)); d_res = Dev(np.zeros(2, orbfe.POSE_RESULT_DTYPE))
    d_kps, d_n, d_has, d_X = Dev(kps), Dev(n), Dev(has), Dev(X)   # kept alive until the call's results are read
    orbfe.pose_optimization_batch_device(d_kps.ptr, d_n.ptr, cap, 2, d_has.ptr,
                                         d_X.ptr, None, None, 0, S.INV_SIGMA2, S.K4, 25.0, d_T.ptr, d_T.ptr,
                                         d_out.ptr, None, d_res.ptr, None)
    res = d_res.get()
    assert res[0]["status"] == 0 and res[0]["n_initial"] == problems[0]["has_mp"].sum()
    assert res[1]["status"] == -1 and res[1]["n_initial"] == 0
    gT = d_T.get().reshape(2, 12)
    assert np.array_equal(gT[1], T[1]) and (d_out.get().reshape(2, cap)[1] == 7).all()


def _chain_frames(nframes, rng):
    """Synthetic frames for the search -> gather -> optimize chain: a scene of tests/pose_opt_cases.py per frame, map points with
    random descriptors, the keypoints with a map point carrying its descriptor (a few bits flipped), window queries projected with
    the initial pose."""
    frames = []
    for f in range(nframes):
        pb = S.problem(300 + 150 * f, outliers=0.0, nmarkers=f % 3, seed=100 + f, perturb=(0.5, 0.02))
        k = len(pb["kps"])
        pb["kps"]["x"] = np.clip(pb["kps"]["x"], 1, S.COLS - 2); pb["kps"]["y"] = np.clip(pb["kps"]["y"], 1, S.ROWS - 2)
        pb["kps"]["angle"] = 0
        desc = rng.integers(0, 256, (k, 32), dtype=np.uint8)
        qi = np.flatnonzero(pb["has_mp"])
        qdesc = desc[qi].copy()
        for j in range(len(qi)):       # 0 .. 7 flipped bits
            for b in rng.integers(0, 256, rng.integers(0, 8)):
                qdesc[j, b // 8] ^= np.uint8(1 << (b % 8))
        uv, _ = S.project(pb["Tcw"].astype(np.float64), pb["x3Dw"][qi].astype(np.float64))
        q = np.zeros(len(qi), np.dtype([("x", "<f4"), ("y", "<f4"), ("r", "<f4"), ("min_level", "<i4"), ("max_level", "<i4")]))
        q["x"], q["y"] = uv[:, 0], uv[:, 1]
        oc = pb["kps"]["octave"][qi]
        q["r"] = (15.0 * S.SCALE ** oc).astype(np.float32)
        q["min_level"], q["max_level"] = oc - 1, oc + 1
        frames.append(dict(pb=pb, desc=desc, q=q, qdesc=qdesc, qX=pb["x3Dw"][qi].astype(np.float32)))
    return frames


def test_device_chain_search_gather_optimize(orbfe):
    L = orbfe.load()
    rng = np.random.default_rng(5)
    frames = _chain_frames(4, rng)
    F = len(frames)
    cap = max(len(fr["pb"]["kps"]) for fr in frames)
    QC = max(len(fr["q"]) for fr in frames)
    mcap = 2
    kps, _, _, mk, n, nm, T = _batch_inputs([fr["pb"] for fr in frames], cap, mcap)
    desc = np.zeros((F, cap, 32), np.uint8); qs = np.zeros((F, QC), frames[0]["q"].dtype); qd = np.zeros((F, QC, 32), np.uint8)
    qX = np.zeros((F, QC, 3), np.float32); nq = np.zeros(F, np.int32)
    for f, fr in enumerate(frames):
        k, m = len(fr["pb"]["kps"]), len(fr["q"])
        desc[f, :k] = fr["desc"]; qs[f, :m] = fr["q"]; qd[f, :m] = fr["qdesc"]; qX[f, :m] = fr["qX"]; nq[f] = m
    d_kps, d_desc, d_n, d_qs, d_qd, d_nq, d_qX = Dev(kps), Dev(desc), Dev(n), Dev(qs), Dev(qd), Dev(nq), Dev(qX)
    d_qang = Dev(np.zeros((F, QC), np.float32))
    raw = [Dev(np.zeros(F * QC, np.int32)) for _ in range(6)]
    d_mc, d_nmatch = Dev(np.zeros(F * cap, np.int32)), Dev(np.zeros(F, np.int32))
    d_has, d_X = Dev(np.zeros(F * cap, np.uint8)), Dev(np.zeros(F * cap * 3, np.float32))
    d_T = Dev(T)
    d_out, d_chi = Dev(np.full(F * cap, 7, np.uint8)), Dev(np.zeros(F * cap, np.float32))
    d_res, d_mk, d_nm = Dev(np.zeros(F, orbfe.POSE_RESULT_DTYPE)), Dev(mk), Dev(nm)
    bounds = np.array([0, 0, S.COLS, S.ROWS], np.float32)
    # the chain, all on the device
    rc = L.orbfe_search_by_projection_batch_device(d_kps.ptr, d_desc.ptr, d_n.ptr, cap, F, S.COLS, S.ROWS,
                                                   bounds.ctypes.data_as(C.c_void_p), d_qs.ptr, d_qd.ptr, d_nq.ptr, QC,
                                                   None, None, d_qang.ptr, 2, 100, np.float32(0.9), np.float32(1.0 / 30), 0,
                                                   *[r.ptr for r in raw[:5]], raw[5].ptr, d_mc.ptr,
                                                   d_nmatch.ptr, None)
    assert rc == 0, L.orbfe_last_error()
    orbfe.pose_gather_device(d_mc.ptr, d_n.ptr, cap, F, d_qX.ptr, d_nq.ptr, QC, d_has.ptr, d_X.ptr, None)
    orbfe.pose_optimization_batch_device(d_kps.ptr, d_n.ptr, cap, F, d_has.ptr, d_X.ptr, d_mk.ptr,
                                         d_nm.ptr, mcap, S.INV_SIGMA2, S.K4, 25.0, d_T.ptr, d_T.ptr, d_out.ptr,
                                         d_chi.ptr, d_res.ptr, None)
    ovf = C.c_int32(0)
    assert L.orbfe_search_by_projection_batch_status(None, C.byref(ovf)) == 0 and ovf.value == 0
    mc = d_mc.get().reshape(F, cap)
    gT = d_T.get().reshape(F, 3, 4)
    gout = d_out.get().reshape(F, cap)
    gres = d_res.get()
    ghas = d_has.get().reshape(F, cap)
    for f, fr in enumerate(frames):
        k = len(fr["pb"]["kps"])
        # the same problem assembled on the host from the search's matches
        has = (mc[f, :k] >= 0).astype(np.uint8)
        X = np.where(has[:, None] == 1, qX[f][np.maximum(mc[f, :k], 0)], 0).astype(np.float32)
        assert np.array_equal(ghas[f, :k], has) and not ghas[f, k:].any()
        assert has.sum() > 0.5 * len(fr["q"]), (f, has.sum(), len(fr["q"]))
        wT, wout, _, wres = orbfe.pose_optimization(fr["pb"]["kps"], has, X, S.INV_SIGMA2, S.K4, T[f].reshape(3, 4),
                                                    markers=fr["pb"]["markers"], outlier=np.full(k, 7, np.uint8))
        assert gres[f].tobytes() == wres.tobytes(), (f, gres[f], wres)
        assert gT[f].tobytes() == wT.tobytes() and np.array_equal(gout[f, :k], wout), f
        # and the pose moved towards the truth
        assert np.abs(gT[f] - fr["pb"]["T_true"]).max() < np.abs(T[f].reshape(3, 4) - fr["pb"]["T_true"]).max()
