"""CPU tests of GlobalBundleAdjustment: the ABI declares and exports it, and the CPU restatement (tests/gba_ref.cpp) that the GPU
parity tests use has second opinions of its own: noise-free scenes come back explaining every observation, its analytic Jacobians
match differences and its numeric ones analytic ones, its reduced solve solves the full system, chi2 never rises, and its two
summation orders run the same path on every case.  The spread between the two orders, printed here, sets the tolerance of the GPU
parity tests (tests/gba_parity.py)."""

import numpy as np
import pytest

import gba_build as B
import gba_cases as S
import gba_parity as P
from test_abi_cpu import _exports

NEW = ["orbfe_gba_scratch_bytes", "orbfe_global_bundle_adjustment", "orbfe_global_bundle_adjustment_device", "orbfe_gba_inspect"]


def test_header_binding_and_library_agree_on_global_bundle_adjustment():
    from orb_slam2_aruco_amd import binding, header
    assert set(NEW) <= set(header.functions), sorted(set(NEW) - set(header.functions))
    assert set(NEW) <= set(binding.SYMBOLS)
    assert set(NEW) <= _exports(), sorted(set(NEW) - _exports())
    rec = header.dtype("orbfe_gba_result")
    assert rec == binding.GBA_RESULT_DTYPE == B.RESULT_DTYPE and rec.itemsize == 48
    defines = header.defines
    assert defines["GBA_MAX_POSES"] == binding.GBA_MAX_POSES == defines["EG_MAX_KEYFRAMES"] == 4096
    assert defines["GBA_MAX_OBSERVATIONS"] == binding.GBA_MAX_OBSERVATIONS == defines["LBA_MAX_OBSERVATIONS"]
    assert defines["GBA_STOPPED"] == binding.GBA_STOPPED
    for f in ("global_bundle_adjustment", "global_bundle_adjustment_device", "gba_inspect", "gba_scratch_bytes"):
        assert callable(getattr(binding, f))
    import __graft_entry__
    assert "global_ba.hip" in __graft_entry__.HIP_SOURCES


def _reprojection(pb, r):
    """the largest reprojection error (pixels) of the float result over the observations and the marker corners in use"""
    worst = 0.0
    for i in range(len(pb["x3Dw"])):
        for e in range(pb["obs_offset"][i], pb["obs_offset"][i + 1]):
            uv, _ = S.project(r["Tcw"][pb["obs_kf"][e]].astype(np.float64), r["x3Dw"][i:i + 1].astype(np.float64))
            worst = max(worst, float(np.abs(uv[0] - pb["obs_xy"][e]).max()))
    for m in range(len(pb["Twm"]) if pb["use_markers"] else 0):
        T = r["Twm"][m].astype(np.float64)
        Pw = pb["marker_local"][m].reshape(4, 3).astype(np.float64) @ T[:, :3].T + T[:, 3]
        for o in range(pb["mobs_offset"][m], pb["mobs_offset"][m + 1]):
            uv, _ = S.project(r["Tcw"][pb["mobs_kf"][o]].astype(np.float64), Pw)
            worst = max(worst, float(np.abs(uv - pb["mobs_corners"][o]).max()))
    return worst


# the scenes of the local bundle adjustment's own test of this kind (a clean scene, the same with a marker: here the initial-map
# shapes) and the two sparse structures the stage tests use
@pytest.mark.parametrize("name", ["init2_p120_r20", "init2_p120_m1_r1", "chain12_p400_leaf2", "ring24_p600_m3_out_r1"])
def test_restatement_explains_every_observation_of_a_noise_free_scene(name):
    """Noise-free float observations, perturbed start, the case's own 10 or 20 iterations.  One fixed keyframe leaves the scale of a
    monocular map free, so the truth is recovered as a map that explains every observation: every edge's error at the estimates the
    optimizer reaches (in double) is below 3e-5 px -- what is left is the rounding of the observations themselves, at most half an
    ulp of a float pixel coordinate: 3.05e-5 px from 512 px on, 1.5e-5 px below.  Measured: 2.1e-5, 1.7e-5, 2.8e-5, 3.0e-5 px on
    these four; over the other shapes 1.9e-5 .. 3.01e-5 px (dense8_p200: 3.01e-5; k70_p300 reaches 2.0e-5 px in 20 iterations and
    stands at 3.0e-4 px after its 10).  The float poses and points that come back add their own rounding, (3 x 2 m x 2^-24 +
    4 m x 2^-24) / 4 m x 520 px = 8e-5 px (tests/test_lba_cpu.py): their reprojection error is printed and held to that sum."""
    pb = S.case(name, noise=0.0)
    for order in (B.INSERTION, B.DEVICE):
        r = B.global_bundle_adjustment(pb, order)
        err, back = float(np.abs(r["err"]).max()), _reprojection(pb, r)
        print(name, order, "max |error| %.2e px in double, %.2e px of the float result, iterations %d" % (err, back, r["result"]["iterations"]))
        assert r["result"]["status"] == 0 and err < 3e-5
        assert back < 3e-5 + 8e-5
        X, Xt = r["x3Dw"].astype(np.float64), pb["true"]["x3Dw"]
        d = np.linalg.norm(X[:, None] - X[None], axis=2)
        dt = np.linalg.norm(Xt[:, None] - Xt[None], axis=2)
        scale = (d * dt).sum() / (dt * dt).sum()
        assert np.abs(d / scale - dt).max() < 1e-5 * dt.max()


def test_analytic_projection_jacobians_match_central_differences():
    rng = np.random.RandomState(3)
    pb = S.case("chain12_p400")
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
    pb = S.case("ring24_p600_m3_out_r1")
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    fx, fy = float(S.K4[0]), float(S.K4[1])
    for m in range(3):
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


@pytest.mark.parametrize("name,idle_rows", [("ring24_p600_m3_out_r1", 0), ("orphans", 6 + 6 + 3), ("init2_p120_m1_r0", 0)])
def test_reduced_solve_solves_the_full_system(name, idle_rows):
    """The first trial's update, reduced and back-substituted, against the whole (6 nv + 3 np) system: its residual relative to
    |H| |x| + |b| is rounding (the condition number does not enter a residual).  A vertex without an edge and a point without
    observations hold lambda alone and do not move."""
    pb = S.case(name)
    for order in (B.INSERTION, B.DEVICE):
        r = B.inspect(pb, order, full=True, reduced=True)
        H, b, x = r["H"], r["b"], r["x"]
        assert r["solved"] and np.allclose(H, H.T, rtol=0, atol=1e-9 * np.abs(H).max())
        scale = np.abs(H - np.diag(np.diag(H))).sum(1) + np.abs(b)
        idle = scale == 0
        assert (x[idle] == 0).all() and idle.sum() == idle_rows
        H, b, x = H[np.ix_(~idle, ~idle)], b[~idle], x[~idle]
        scale = np.abs(H) @ np.abs(x) + np.abs(b)
        mine = np.abs(H @ x - b) / scale
        theirs = np.abs(H @ np.linalg.solve(H, b) - b) / scale
        print(name, order, "residual %.2e, numpy's %.2e" % (mine.max(), theirs.max()))
        assert mine.max() < 1e-12 and np.abs(x).max() > 0
        # the reduced system is the Schur complement of the full one
        n6 = 6 * r["nv"]
        live = ~idle[:n6]
        Hf = r["H"]
        Sc = Hf[:n6, :n6] - Hf[:n6, n6:] @ np.linalg.solve(Hf[n6:, n6:], Hf[n6:, :n6])
        assert np.abs(Sc - r["S"])[np.ix_(live, live)].max() <= 1e-9 * np.abs(Sc).max()


def test_chi2_never_rises_and_the_two_orders_run_the_same_path_on_every_case():
    """chi2_last <= chi2_first; the same iterations and trials in both orders, so no case is left out of the spread"""
    s = P.spread()
    for name in P.NAMES:
        _, r0, r1 = P.problem(name)
        for r in (r0, r1):
            res = r["result"]
            assert res["status"] == 0 and res["iterations"] >= 1 and res["chi2_last"] <= res["chi2_first"], (name, res)
    assert s["left_out"] == []
    print("spread between the orders:", {k: "%.2e" % s[k] for k in P.QUANTITIES})
    for name, d in s["per_case"].items():
        print("%-26s" % name, "  ".join("%s %.2e" % (k, d[k]) for k in P.QUANTITIES))
    # the project's bound on a parity tolerance is 1e-5
    assert max(P.tolerance().values()) <= 1e-5 and min(P.tolerance().values()) > 0


def test_cases_are_what_they_say():
    z = P.problem("z0")
    assert np.isinf(z[1]["result"]["chi2_first"]) and np.isfinite(z[1]["result"]["chi2_last"])
    assert P.problem("orphans")[1]["result"]["n_points_left_out"] == 1
    assert (S.case("nofixed6_p150")["kf_fixed"] == 0).all() and (S.case("k70_p300")["kf_fixed"] == 0).sum() == 70
    assert (np.diff(S.case("obs64_p12")["obs_offset"]) == 64).all() and len(S.case("p257")["x3Dw"]) == 257
    ring = S.case("ring24_p600_m3_out_r1")
    assert ring["outlier"].mean() > 0.05 and {0, 23} <= {int(k) for i in range(600) for k in ring["obs_kf"][ring["obs_offset"][i]:ring["obs_offset"][i + 1]]
                                                       if 0 in ring["obs_kf"][ring["obs_offset"][i]:ring["obs_offset"][i + 1]]}
