"""CPU tests of LocalBundleAdjustment: the ABI declares and exports it, and the CPU restatement (tests/lba_ref.cpp) that the GPU
parity tests use has second opinions of its own: it recovers ground truth on clean scenes, flags the injected outliers, its analytic
Jacobians match differences and its numeric ones analytic ones, its Schur solve solves the full system, and its two summation
orders give the same decisions.  The spread between the two orders, printed here, sets the tolerance of the GPU parity tests."""

import numpy as np
import pytest

import lba_build as B
import lba_cases as S
import lba_parity as P
from test_abi_cpu import _exports

NEW = ["orbfe_lba_scratch_bytes", "orbfe_local_bundle_adjustment", "orbfe_local_bundle_adjustment_device", "orbfe_lba_inspect"]


def test_header_binding_and_library_agree_on_local_bundle_adjustment():
    from orb_slam2_aruco_amd import binding, header
    assert set(NEW) <= set(header.functions), sorted(set(NEW) - set(header.functions))
    assert set(NEW) <= set(binding.SYMBOLS)
    assert set(NEW) <= _exports(), sorted(set(NEW) - _exports())
    rec = header.dtype("orbfe_lba_result")
    assert rec == binding.LBA_RESULT_DTYPE == B.RESULT_DTYPE and rec.itemsize == 36
    assert header.defines["LBA_MAX_FREE_POSES"] == binding.LBA_MAX_FREE_POSES >= 64
    assert header.defines["LBA_MAX_OBSERVATIONS"] == binding.LBA_MAX_OBSERVATIONS == 256
    assert header.defines["LBA_STOPPED"] == binding.LBA_STOPPED
    import __graft_entry__
    assert "local_ba.hip" in __graft_entry__.HIP_SOURCES


def _reprojection(pb, r):
    """the largest reprojection error (pixels) of a result over the observations and the marker corners"""
    worst = 0.0
    for i in range(len(pb["x3Dw"])):
        for e in range(pb["obs_offset"][i], pb["obs_offset"][i + 1]):
            uv, _ = S.project(r["Tcw"][pb["obs_kf"][e]].astype(np.float64), r["x3Dw"][i:i + 1].astype(np.float64))
            worst = max(worst, float(np.abs(uv[0] - pb["obs_xy"][e]).max()))
    for m in range(len(pb["Twm"])):
        T = r["Twm"][m].astype(np.float64)
        Pw = pb["marker_local"][m].reshape(4, 3).astype(np.float64) @ T[:, :3].T + T[:, 3]
        for o in range(pb["mobs_offset"][m], pb["mobs_offset"][m + 1]):
            uv, _ = S.project(r["Tcw"][pb["mobs_kf"][o]].astype(np.float64), Pw)
            worst = max(worst, float(np.abs(uv - pb["mobs_corners"][o]).max()))
    return worst


@pytest.mark.parametrize("name", ["k3_p40_clean", "k3_p40_clean_m1"])
def test_restatement_recovers_the_truth_on_clean_scenes(name):
    """Noise-free float observations, perturbed start.  One fixed keyframe leaves the scale of a monocular map free, so the truth is
    recovered as a map that explains every observation: the bound is the rounding of the float poses and points that come back,
    (3 x 2 m x 2^-24 + 4 m x 2^-24) / 4 m x 520 px = 8e-5 px, and of the float observations, 640 x 2^-24 = 4e-5 px; 1e-3 px is ten
    times their sum.  The shape is the true one: distances between points, relative to their spread, to 1e-5."""
    pb = S.case(name)
    for order in (B.INSERTION, B.DEVICE):
        r = B.local_bundle_adjustment(pb, order)
        res = r["result"]
        assert r["rc"] == 0 and res["n_erase"] == 0 and not r["erase"].any() and list(res["n_level1"]) == [0, 0]
        err = _reprojection(pb, r)
        print(name, order, "max reprojection error %.2e px, iterations" % err, res["iterations"])
        assert err < 1e-3
        X, Xt = r["x3Dw"].astype(np.float64), pb["true"]["x3Dw"]
        d = np.linalg.norm(X[:, None] - X[None], axis=2)
        dt = np.linalg.norm(Xt[:, None] - Xt[None], axis=2)
        scale = (d * dt).sum() / (dt * dt).sum()
        assert np.abs(d / scale - dt).max() < 1e-5 * dt.max()


def test_restatement_flags_every_injected_outlier():
    """Every gross outlier (15 - 60 px on both axes, chi2 >= 150) of a scene where each is decidable -- at least five observations a
    point, at most one of them an outlier -- ends in the erase list, in both orders."""
    pb = S.case("k6f3_p250_out8_decidable")
    n = np.diff(pb["obs_offset"])
    nout = np.add.reduceat(pb["outlier"].astype(np.int64), pb["obs_offset"][:-1])
    assert n.min() >= 5 and nout.max() == 1 and pb["outlier"].sum() >= 60
    for order in (B.INSERTION, B.DEVICE):
        r = B.local_bundle_adjustment(pb, order)
        missed = np.flatnonzero(pb["outlier"] & (r["erase"] == 0))
        assert len(missed) == 0, missed
        assert r["result"]["n_erase"] == r["erase"].sum() >= pb["outlier"].sum()


@pytest.mark.parametrize("name", ["k4f2_p300_out10", "k6f3_p1000_out20_m2", "no_markers"])
def test_an_outlier_that_is_not_flagged_sits_on_a_point_that_cannot_hold_it(name):
    """The parity cases inject outliers blindly.  There, every outlier on a point with at least four observations and no second
    outlier is erased, and every one that is NOT erased is named and shown to sit on a point with fewer than four observations or
    with a second outlier (the point itself moves towards the outlier and the residual is shared)."""
    pb = S.case(name)
    r = B.local_bundle_adjustment(pb, B.INSERTION)
    n = np.diff(pb["obs_offset"])
    nout = np.add.reduceat(pb["outlier"].astype(np.int64), pb["obs_offset"][:-1])
    held = np.repeat((n >= 4) & (nout == 1), n) & pb["outlier"]
    assert held.sum() > 0 and r["erase"][held].all(), (int(held.sum()), int(r["erase"][held].sum()))
    point_of = np.repeat(np.arange(len(n)), n)
    for e in np.flatnonzero(pb["outlier"] & (r["erase"] == 0)):
        i = point_of[e]
        assert n[i] < 4 or nout[i] >= 2, (int(e), int(i), int(n[i]), int(nout[i]))
    assert r["result"]["n_erase"] == r["erase"].sum()


def test_analytic_projection_jacobians_match_central_differences():
    rng = np.random.RandomState(3)
    pb = S.case("k3_p40_clean")
    for e in rng.choice(len(pb["obs_kf"]), 12, replace=False):
        i = int(np.searchsorted(pb["obs_offset"], e, side="right") - 1)
        T, X, obs = pb["Tcw"][pb["obs_kf"][e]], pb["x3Dw"][i].astype(np.float64), pb["obs_xy"][e].astype(np.float64)
        _, Jp, Jx = B.mono_edge(T, np.zeros(6), X, obs, S.K4)
        h = 1e-6
        Np, Nx = np.zeros((2, 6)), np.zeros((2, 3))
        for d in range(6):
            u = np.zeros(6); u[d] = h
            Np[:, d] = (B.mono_edge(T, u, X, obs, S.K4)[0] - B.mono_edge(T, -u, X, obs, S.K4)[0]) / (2 * h)
        for d in range(3):
            dx = np.zeros(3); dx[d] = h
            Nx[:, d] = (B.mono_edge(T, np.zeros(6), X + dx, obs, S.K4)[0] - B.mono_edge(T, np.zeros(6), X - dx, obs, S.K4)[0]) / (2 * h)
        assert np.abs(Jp - Np).max() <= 1e-5 * np.abs(Jp).max() and np.abs(Jx - Nx).max() <= 1e-5 * np.abs(Jx).max()


def test_numeric_marker_jacobians_match_analytic_ones():
    """d e / d (camera increment) = -dpi(Xc) [-[Xc]x | I]; d e / d (marker increment) = -dpi(Xc) Rcw [-[Xw]x | I], Xw = Twm p"""
    pb = S.case("k6f3_p1000_out20_m2")
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    fx, fy = float(S.K4[0]), float(S.K4[1])
    for m in range(2):
        for o in range(pb["mobs_offset"][m], pb["mobs_offset"][m + 1]):
            Tc, Tm = pb["Tcw"][pb["mobs_kf"][o]].astype(np.float64), pb["Twm"][m].astype(np.float64)
            for k in range(4):
                p = pb["marker_local"][m].reshape(4, 3)[k].astype(np.float64)
                _, Jc, Jm = B.marker_edge(Tc, Tm, p, pb["mobs_corners"][o][k], S.K4)
                Xw = Tm[:, :3] @ p + Tm[:, 3]
                Xc = Tc[:, :3] @ Xw + Tc[:, 3]
                dpi = np.array([[fx / Xc[2], 0, -fx * Xc[0] / Xc[2] ** 2], [0, fy / Xc[2], -fy * Xc[1] / Xc[2] ** 2]])
                Ac = -dpi @ np.hstack([-skew(Xc), np.eye(3)])
                Am = -dpi @ Tc[:, :3] @ np.hstack([-skew(Xw), np.eye(3)])
                assert np.abs(Jc - Ac).max() <= 1e-5 * np.abs(Ac).max() and np.abs(Jm - Am).max() <= 1e-5 * np.abs(Am).max()


@pytest.mark.parametrize("name", ["k3_p40_clean_m1", "special"])
def test_schur_solve_solves_the_full_system(name):
    """The first trial's update, reduced and back-substituted, against the whole (6 nv + 3 np) system: its residual relative to
    |H| |x| + |b| is rounding (the condition number does not enter a residual), and numpy's own solution has a residual no smaller
    than a hundredth of it."""
    pb = S.case(name)
    for order in (B.INSERTION, B.DEVICE):
        r = B.inspect(pb, order, full=True)
        H, b, x = r["H"], r["b"], r["x"]
        live = np.abs(H).sum(1) > 0           # a vertex without an edge has no row
        H, b, x = H[np.ix_(live, live)], b[live], x[live]
        assert np.allclose(H, H.T, rtol=0, atol=1e-9 * np.abs(H).max())
        scale = np.abs(H) @ np.abs(x) + np.abs(b)
        idle = scale == 0                     # a free keyframe without an edge: lambda on its diagonal, nothing else, x = 0
        assert (x[idle] == 0).all() and idle.sum() == (6 if name == "special" else 0)
        H, b, x, scale = H[np.ix_(~idle, ~idle)], b[~idle], x[~idle], scale[~idle]
        mine = np.abs(H @ x - b) / scale
        theirs = np.abs(H @ np.linalg.solve(H, b) - b) / scale
        print(name, order, "residual %.2e, numpy's %.2e" % (mine.max(), theirs.max()))
        assert mine.max() < 1e-12 and np.abs(x).max() > 0


def test_the_stale_cases_still_end_their_rounds_on_rejected_trials():
    for name, mask in (("stale_r1", 1), ("stale_r2", 2)):
        _, r0, r1 = P.problem(name)
        assert r0["result"]["stale_mask"] & mask and r1["result"]["stale_mask"] & mask, (name, r0["result"], r1["result"])


def test_recorded_stale_case_is_the_restarted_scene():
    """tests/golden/lba_stale_r1.npz is scene(3, 1, 60, 306) restarted once from the restatement's own result; the restatement still
    gives that problem (float for float), so the fixture and the recipe in its name stay together"""
    pb, again = S.case("stale_r1"), S.restarted(S.scene(3, 1, 60, 306), 1)
    for k in ("Tcw", "x3Dw", "obs_offset", "obs_kf", "obs_xy", "obs_octave", "kf_fixed"):
        assert np.array_equal(np.asarray(pb[k]), np.asarray(again[k])), k


def test_special_case_is_what_it_says():
    pb, r0, _ = P.problem("special")
    k = pb["lonely_keyframe"]
    assert not (pb["obs_kf"] == k).any() and not (pb["mobs_kf"] == k).any() and pb["kf_fixed"][k] == 0
    # it does not move, not by a bit: what comes back is the float pose through the quaternion, as from a problem that holds nothing else
    alone = dict(Tcw=pb["Tcw"][k:k + 1], kf_fixed=np.zeros(1, np.uint8), K=S.K4, inv_level_sigma2=S.INV_SIGMA2)
    assert np.array_equal(r0["Tcw"][k], B.local_bundle_adjustment(alone)["Tcw"][0]) and np.abs(r0["Tcw"][k] - pb["Tcw"][k]).max() < 2e-7
    assert np.diff(pb["obs_offset"])[pb["single_point"]] == 1
    m = pb["dead_marker"]
    lo, hi = 4 * pb["mobs_offset"][m], 4 * pb["mobs_offset"][m + 1]
    nobs = len(pb["obs_kf"])
    assert (r0["chi2"][0, nobs + lo:nobs + hi] > P.TH).all() and r0["result"]["n_level1"][1] >= hi - lo
    # at level 1 in round 2: the cached chi2 of its edges is still the first round's
    assert np.array_equal(r0["chi2"][0, nobs + lo:nobs + hi], r0["chi2"][1, nobs + lo:nobs + hi])
    pz, rz, _ = P.problem("z0")
    assert rz["erase"][pz["z0_slot"]] and rz["result"]["n_level1"][0] >= 1
    assert B.local_bundle_adjustment(S.over_bound())["rc"] == -4 and P.problem("free64")[1]["rc"] == 0


def test_two_summation_orders_agree_on_every_decision():
    """Every decision of the restatement in g2o's insertion order and in the device's order; a case may be set aside under the gate
    rule only, at most 10 % of them.  Prints the spread that sets the GPU tests' tolerance."""
    not_compared = []
    for name in P.NAMES:
        _, r0, r1 = P.problem(name)
        assert r0["rc"] == r1["rc"] == 0
        if P.decisions_equal(r0, r1):
            continue
        assert P.gated(r0, r1), (name, r0["result"], r1["result"])
        not_compared.append(name)
    assert len(not_compared) <= P.MAX_NOT_COMPARED * len(P.NAMES), not_compared
    s = P.spread()
    for name, d in s["per_case"].items():
        print("%-24s dR %.2e dt %.2e dX %.2e dRm %.2e dtm %.2e" % (name, d["dR"], d["dt"], d["dX"], d["dRm"], d["dtm"]))
    print("order spread over %d cases (%d not compared): %s" % (len(P.NAMES), len(not_compared), {k: "%.2e" % v for k, v in s.items() if k != "per_case"}))
    print("tolerance of the GPU parity tests (10 x):", {k: "%.2e" % v for k, v in P.tolerance().items()})
    # the project's bound is 1e-5.  The keyframes and the points stay far below it.  The marker poses do not: the case that drives
    # their spread is `special`, whose second marker has nothing but contradictory observations (all its edges go to level 1): its pose
    # after round 1 is whatever Huber leaves of a fit without a minimum worth the name, found through Jacobians that divide rounding
    # by 2e-9.  DESIGN.md 4h reports it; nothing is widened for it: every other case stays below the bound on every quantity.
    tol = P.tolerance()
    assert max(tol["dR"], tol["dt"], tol["dX"]) <= 1e-5
    others = [d for name, d in s["per_case"].items() if name != "special"]
    assert 10 * max(max(d["dRm"], d["dtm"]) for d in others) <= 1e-5


@pytest.mark.parametrize("seed,outliers", [(3, 0.0), (4, 0.12), (5, 0.23), (6, 0.12)])
def test_with_points_held_it_reproduces_the_pose_restatement(seed, outliers):
    """The anchor to accepted code.  With its points held at their positions and one free pose, the problem is the motion-only one
    that tests/pose_opt_ref.cpp restates.  That restatement exposes whole calls; with fewer than 10 edges a call is ONE optimize(10)
    with Huber from the initial pose, so nine edges compare every LM step of it, the first included: the same number of LM
    iterations, and the float pose that comes back.  The two differ in how they write the Jacobian (1 / z products against
    divisions) and in the dense solve (pivoted LDLT against LLT), which is rounding in double: the floats may differ by one
    unit in the last place of the largest entry, no more."""
    import pose_opt_build
    import pose_opt_cases
    pp = pose_opt_cases.problem(9, outliers=outliers, nmarkers=0, seed=seed, unmatched=0.0)
    want = pose_opt_build.pose_optimization(pp)
    assert want["rc"] == 0 and want["result"]["rounds"] == 1 and want["result"]["n_initial"] == 9
    kps = pp["kps"]
    pb = dict(Tcw=np.asarray(pp["Tcw"], np.float32).reshape(1, 3, 4), kf_fixed=np.zeros(1, np.uint8), x3Dw=np.asarray(pp["x3Dw"], np.float32),
              obs_offset=np.arange(10, dtype=np.int32), obs_kf=np.zeros(9, np.int32), obs_xy=np.stack([kps["x"], kps["y"]], 1),
              obs_octave=kps["octave"], K=pp["K4"], inv_level_sigma2=pp["inv_sigma2"])
    for order in (B.INSERTION, B.DEVICE):
        T, it = B.poses_only(pb, 10, order)
        ulp = 2.0 ** -23 * max(1.0, float(np.abs(want["Tcw"]).max()))
        print(seed, order, "iterations", it, want["result"]["iterations"][0], "max |dT| %.2e (one ulp %.2e)" % (np.abs(T[0] - want["Tcw"]).max(), ulp))
        assert it == want["result"]["iterations"][0]
        assert np.abs(T[0].astype(np.float64) - want["Tcw"]).max() <= ulp
        assert np.abs(T[0] - pb["Tcw"][0]).max() > 1e-3      # it moved: the comparison is of an optimization, not of two copies
