"""CPU tests of the motion-only pose optimization: the ABI declares and exports it, the shim compiles and links against the mock
headers, and the CPU restatement (tests/pose_opt_ref.cpp) that the GPU parity tests use recovers ground truth on synthetic scenes
(its own second opinion)."""

import numpy as np
import pytest

import pose_opt_build as B
import pose_opt_cases as S
from test_abi_cpu import _exports

NEW = ["orbfe_pose_optimization", "orbfe_pose_optimization_batch_device", "orbfe_pose_gather_device"]


def test_header_binding_and_library_agree_on_the_pose_optimization():
    from orb_slam2_aruco_amd import binding, header
    assert set(NEW) <= set(header.functions), sorted(set(NEW) - set(header.functions))
    assert set(NEW) <= set(binding.SYMBOLS)
    assert set(NEW) <= _exports(), sorted(set(NEW) - _exports())
    assert "orbfe_pose_result" in header.records and "orbfe_pose_marker" in header.records
    # the record layouts the bindings and the restatement use
    assert binding.POSE_RESULT_DTYPE == B.RESULT_DTYPE and binding.POSE_MARKER_DTYPE == B.MARKER_DTYPE


def _rot_err(Ra, Rb):
    """rotation angle of Ra^T Rb, from the skew part (accurate near 0, unlike the trace)"""
    D = np.asarray(Ra, np.float64)[:3, :3].T @ np.asarray(Rb, np.float64)[:3, :3]
    return np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2


@pytest.mark.parametrize("name", ["clean_n500", "clean_true_n60", "clean_true_n500_m1", "clean_true_n2000_m3", "clean_true_n9"])
def test_restatement_recovers_the_true_pose_on_clean_scenes(name):
    pb = S.case(name)
    r = B.pose_optimization(pb)
    res = r["result"]
    assert r["rc"] == 0 and res["n_initial"] == pb["has_mp"].sum() and res["n_good"] == res["n_initial"]
    assert _rot_err(r["Tcw"], pb["T_true"]) < 1e-4
    assert np.linalg.norm(r["Tcw"][:, 3] - pb["T_true"][:, 3]) < 1e-4 * pb["depth"]
    assert not r["outlier"][pb["has_mp"] == 1].any()


@pytest.mark.parametrize("name", ["n60_out30_m1", "n60_out50", "n500_out10_m3", "n500_out30", "n500_out50_m1", "n2000_out10",
                                  "n2000_out30_m3", "big_perturb"])
def test_restatement_flags_the_injected_outliers(name):
    pb = S.case(name)
    r = B.pose_optimization(pb)
    has = pb["has_mp"] == 1
    flagged = r["outlier"][has].astype(bool)
    bad = pb["bad"][has]
    assert flagged[bad].all(), (~flagged[bad]).sum()
    # 1 px noise at chi2(2 dof) = 5.991: about 5 % of the inliers lie beyond the gate
    assert flagged[~bad].mean() < 0.12, flagged[~bad].mean()
    assert r["result"]["n_good"] == (~flagged).sum()
    assert _rot_err(r["Tcw"], pb["T_true"]) < 5e-3 and np.linalg.norm(r["Tcw"][:, 3] - pb["T_true"][:, 3]) < 0.01 * pb["depth"]


def test_untouched_entries_keep_their_value():
    pb = S.case("n500_out10_m3")
    r = B.pose_optimization(pb, outlier_init=7)
    assert (r["outlier"][pb["has_mp"] == 0] == 7).all() and set(r["outlier"][pb["has_mp"] == 1].tolist()) <= {0, 1}


@pytest.mark.parametrize("name", ["n2", "n2_markers"])
def test_fewer_than_three_observations_return_zero_with_the_pose_untouched(name):
    pb = S.case(name)
    r = B.pose_optimization(pb)
    res = r["result"]
    assert res["n_initial"] == 2 and res["n_good"] == 0 and res["rounds"] == 0 and res["n_marker_edges"] == 0
    assert np.array_equal(r["Tcw"], pb["Tcw"])
    assert (r["outlier"][pb["has_mp"] == 1] == 0).all() and (r["outlier"][pb["has_mp"] == 0] == 7).all()


@pytest.mark.parametrize("n,nm,rounds", [(5, 0, 1), (5, 1, 1), (9, 0, 1), (10, 0, 4), (6, 1, 4), (9, 1, 4)])
def test_fewer_than_ten_edges_run_one_round(n, nm, rounds):
    pb = S.problem(n, nmarkers=nm, seed=40 + n + nm)
    res = B.pose_optimization(pb)["result"]
    assert res["n_initial"] == n and res["n_marker_edges"] == 4 * nm and res["rounds"] == rounds


def test_bad_octave_is_rejected():
    pb = S.case("n60")
    i = int(np.flatnonzero(pb["has_mp"])[3])
    pb["kps"]["octave"][i] = 8
    assert B.pose_optimization(pb)["rc"] == -1


def test_some_cases_end_rounds_on_rejected_trials():
    """the stale-error quirk (a round that ends on rejected trials classifies its inliers with the rejected trial's errors) is
    exercised by the case set"""
    stale = [name for name in S.CASES if B.pose_optimization(S.case(name))["result"]["stale_mask"]]
    assert len(stale) >= 2, stale


def _analytic_marker_jacobian(Tcw, Twm, p):
    """d(obs - pi(exp(d) T Twm p)) / d(d), d = (omega, upsilon): -dpi/dXc [-[Xc]x | I]"""
    Xm = Twm[:, :3].astype(np.float64) @ p + Twm[:, 3]
    Xc = Tcw[:, :3].astype(np.float64) @ Xm + Tcw[:, 3]
    x, y, z = Xc
    fx, fy = float(S.K4[0]), float(S.K4[1])
    dpi = np.array([[fx / z, 0, -fx * x / z ** 2], [0, fy / z, -fy * y / z ** 2]])
    skew = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return -dpi @ np.concatenate([-skew, np.eye(3)], 1)


@pytest.mark.parametrize("seed", range(6))
def test_numeric_marker_jacobian_matches_the_analytic_one(seed):
    pb = S.problem(20, nmarkers=3, seed=60 + seed)
    for m in pb["markers"]:
        Twm = m["Twm"].reshape(3, 4)
        for k in range(4):
            p = m["local"][3 * k:3 * k + 3].astype(np.float64)
            obs = m["corners"][2 * k:2 * k + 2].astype(np.float64)
            Jn, _ = B.marker_jacobian(pb["Tcw"], Twm, p, obs, S.K4)
            Ja = _analytic_marker_jacobian(pb["Tcw"], Twm, p)
            assert np.abs(Jn - Ja).max() <= 1e-5 * np.abs(Ja).max(), (Jn, Ja)


def test_exp_update_is_left_multiplied():
    pb = S.case("n60")
    u = np.array([0.01, -0.02, 0.03, 0.1, 0.05, -0.2])
    th = np.linalg.norm(u[:3]); a = u[:3] / th
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    V = np.eye(3) + (1 - np.cos(th)) / th * Kx + (th - np.sin(th)) / th * Kx @ Kx
    T = pb["Tcw"].astype(np.float64)
    got = B.exp_update(u, pb["Tcw"])
    assert np.allclose(got[:, :3], R @ T[:, :3], atol=1e-6) and np.allclose(got[:, 3], R @ T[:, 3] + V @ u[3:], atol=1e-6)
