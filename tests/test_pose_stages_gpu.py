"""GPU: every stage of csrc/aruco_pose.hpp (through tests/device_units_probe.hip, the header included unchanged) against the 50-digit
reference of tests/golden/pose_hard_cases.npz, on every family of hard cases.  Only the fixture is read: no mpmath, no oracle.

Bounds.  A stage's error is measured in eps times the stage's own condition (written into the fixture by tests/gen_pose_golden.py from
the reference alone), and may reach 4 x the worst of the plain double evaluation (numpy / LAPACK) over the same cases, at least 4 --
the rule of test_device_units_gpu.py::test_ldlt_solve.  Plain doubles measured: homography 0.19 (condition: kappa_inf of the 8 x 8 system of
the four correspondences), rotations 2.2 (1 / (2 b), b the smaller square root of computeRotations), translation 1.1 (kappa_inf of its
3 x 3 normal equations), eigenvector 2.5 (1 / relative gap).  So the bounds are 4, 9.0, 4.6 and 10.  Each test prints the device's worst;
on an MI355X: homography 0.77, rotations 2.4, translation 1.1, eigenvector 1.4 (the cases' matrices) and 0.63 (random ones)."""
import os

import numpy as np
import pytest

import device_units_build as B
import pose_cases as pc
import pose_contract as contract

pytestmark = pytest.mark.gpu
EPS = contract.EPS
bits = lambda a: np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.fixture(scope="module")
def fx():
    return contract.Fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_hard_cases.npz"))


def families(fx, valid_only=True):
    for f in range(len(fx["fam_names"])):
        idx = np.flatnonzero((fx["fam"] == f) & (fx["valid"] | (not valid_only)))
        if len(idx):
            yield f, idx


def obj8(fx, f, n, dtype=np.float64):
    return np.tile(pc.object_points(fx["fam_size"][f])[:, :2].astype(dtype).ravel(), (n, 1))


def test_normalise_point_rounds_to_the_reference_floats(fx):
    """The normalised corners, five undistortion iterations in double and rounded to float, equal the reference's bit for bit: the
    double before rounding is within a few ulps of exact, so a float differs only where the exact value lies within 1e-15 relative of
    a rounding boundary -- 3e-8 of all values, none of these 2 960.  Eight and twelve coefficients included."""
    for f, idx in families(fx):
        got = B.pose_normalise(fx["corners"][idx].reshape(-1, 2), fx["cam17"][f]).reshape(-1, 4, 2)
        assert np.array_equal(bits(got), bits(fx["img"][idx])), (str(fx["fam_names"][f]), np.abs(got - fx["img"][idx]).max())
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))


def test_smallest_eigenvector_ties_follow_cv_eigen():
    """On diagonal input the Jacobi loop does nothing and the choice among equal eigenvalues is the sort's: cv::eigen (a selection sort
    for descending order that swaps rows) leaves row 2 last where it is among the smallest, else row 0 -- (a, a, b) gives row 0."""
    a, b = 0.25, 3.0
    diag = np.array([[a, a, b], [b, a, a], [a, b, a], [a, a, a], [a, b, b], [b, a, b], [b, b, a], [0, 0, 1], [1, 0, 0]])
    want = np.array([0, 2, 2, 2, 0, 1, 2, 0, 2])
    a6 = np.zeros((len(diag), 6)); a6[:, 0] = diag[:, 0]; a6[:, 3] = diag[:, 1]; a6[:, 5] = diag[:, 2]
    assert np.array_equal(B.pose_eig(a6), np.eye(3)[want])


def eig_ratio(h, ref, gap):
    d = np.minimum(np.abs(h - ref).max(1), np.abs(h + ref).max(1))
    return d / (EPS / np.maximum(gap, EPS))


def test_smallest_eigenvector_against_eigsy(fx):
    """Random symmetric positive (semi-)definite matrices, some with a close pair, and the matrices the hard cases give the estimator
    (smallest eigenvalue zero up to rounding): the unit eigenvector up to sign within eps / gap times the bound."""
    bound = max(4.0, 4.0 * float(fx["W_ev"]))
    v = fx["valid"]
    for name, a6, h, gap in (("random", fx["evx"], fx["evx_h"], fx["evx_gap"]), ("cases", fx["S"][v], fx["ev_h"][v], fx["ev_gap"][v])):
        got = B.pose_eig(a6)
        assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 8 * EPS
        r = eig_ratio(got, h, gap)
        print("smallest_eigenvector %s: device worst %.3g, plain doubles %.3g, bound %.3g" % (name, r.max(), fx["W_ev"], bound))
        assert r.max() <= bound, (name, int(r.argmax()), r.max())


def test_homography4(fx):
    bound = max(4.0, 4.0 * float(fx["W_H"]))
    worst = 0.0
    for f, idx in families(fx):
        H = B.pose_homography(obj8(fx, f, len(idx)), fx["img"][idx])
        assert (H[:, 8] == 1).all()
        r = np.abs(H - fx["H"][idx]).max(1) / (EPS * fx["kH"][idx] * np.abs(fx["H"][idx]).max(1))
        worst = max(worst, r.max())
        assert r.max() <= bound, (str(fx["fam_names"][f]), int(idx[r.argmax()]), r.max())
    print("homography4: device worst %.3g, plain doubles %.3g, bound %.3g" % (worst, fx["W_H"], bound))


def test_rotations_and_radicands(fx):
    """Where a reference radicand is within 64 eps of zero, NaN or a square root below 1e-7 are both right: the device's matrices are NaN
    or within 2.2e-7 of the reference's (|b| < 1e-7 on one side, <= sqrt(64 eps) = 1.2e-7 on the other).  Elsewhere NaN is an error."""
    bound = max(4.0, 4.0 * float(fx["W_rot"]))
    worst, zone_n = 0.0, 0
    for f, idx in families(fx):
        R1, R2 = B.pose_rotations(fx["J"][idx])
        got = np.stack([R1, R2], 1)
        zone = fx["rad_st"][idx].min(1) <= contract.ZONE
        zone_n += int(zone.sum())
        d = np.abs(got - fx["Rst"][idx]).max((1, 2))
        assert (np.isnan(d[zone]) | (d[zone] <= 2.2e-7)).all(), (str(fx["fam_names"][f]), d[zone])
        if (~zone).any():
            r = d[~zone] / (EPS * fx["k_rot"][idx][~zone])
            worst = max(worst, r.max())
            assert r.max() <= bound, (str(fx["fam_names"][f]), int(idx[~zone][r.argmax()]), r.max())          # NaN fails here too
    print("rotations: device worst %.3g, plain doubles %.3g, bound %.3g; %d cases with a zero radicand" % (worst, fx["W_rot"], bound, zone_n))
    assert zone_n >= 4          # the centred pixel-grid squares


def test_translation(fx):
    bound = max(4.0, 4.0 * float(fx["W_t"]))
    worst = 0.0
    for f, idx in families(fx):
        for k in range(2):
            t = B.pose_translation(obj8(fx, f, len(idx)), fx["img"][idx], fx["R"][idx, k])
            r = np.abs(t - fx["tst"][idx, k]).max(1) / (EPS * fx["kT"][idx] * np.abs(fx["tst"][idx, k]).max(1))
            worst = max(worst, r.max())
            assert r.max() <= bound, (str(fx["fam_names"][f]), k, int(idx[r.argmax()]), r.max())
    print("translation: device worst %.3g, plain doubles %.3g, bound %.3g" % (worst, fx["W_t"], bound))


def test_rot2vec(fx):
    """Rotations by 0, 1e-8, 1e-7 (zero branch: exactly 0), 1.2e-7 (acos' argument rounds to 1 - 2^-47, whose arc cosine is FLT_EPSILON to
    three ulps: either branch), 1.3e-7, 1e-6, 1e-3, 1, pi - 1e-3, pi - 1e-6, pi - 1e-8 about three axes, and exactly diag(1, -1, -1):
    Rodrigues(r) within 4 (A eps / (pi - w)^2 + B) of the input matrix, which allows anything from pi - 1e-7 on."""
    r = B.pose_rot2vec(fx["rv_R"])
    assert len(r) == 34 and fx["rv_zero"].sum() == 9 and fx["rv_edge"].sum() == 3
    worst = 0.0
    for i in range(len(r)):
        if fx["rv_zero"][i]:
            assert (r[i] == 0).all() and not np.signbit(r[i]).any(), (i, r[i])
            continue
        if fx["rv_edge"][i] and (r[i] == 0).all():
            continue
        e = contract.e_rot(r[i], fx["rv_R"][i])
        if np.isfinite(fx["rv_tol"][i]) and fx["rv_tol"][i] < 1:
            worst = max(worst, e / fx["rv_tol"][i])
            assert e <= fx["rv_tol"][i], (i, e, fx["rv_tol"][i], fx["rv_pimw"][i])
        else:
            assert np.isnan(r[i]).all() or np.isfinite(r[i]).all(), (i, r[i])
    assert (r[-1] == 0).all()          # the exact half turn: the skew part is exactly 0 and sin(pi) is not
    print("rot2vec: device worst eR / tolerance %.3g" % worst)


def test_reprojection_error(fx):
    """Against the reference's float result (projections rounded to float, float differences and sums) within the project's 1e-3 px
    (relative above 1 px) plus the rotation tolerance of rot2vec carried to pixels; theta = 0 takes the identity branch, and a pose
    with t_z = 0 under the identity puts all four corners at z = 0, where the guard divides by 1."""
    worst = 0.0
    for f, idx in families(fx):
        for k in range(2):
            e = B.pose_reproj(obj8(fx, f, len(idx), np.float32), fx["corners"][idx], fx["cam17"][f], fx["R"][idx, k], fx["t"][idx, k])
            ref, tol = fx["rp_err"][idx, k].astype(np.float64), fx["tolE"][idx, k].astype(np.float64)
            both = np.isfinite(ref) & np.isfinite(e)
            assert ((np.abs(e - ref) <= tol) | ~both).all(), (str(fx["fam_names"][f]), k, e, ref, tol)
            assert (both | ~np.isfinite(tol) | (tol > 1)).all(), (str(fx["fam_names"][f]), k, e, ref)        # NaN only where rot2vec may lose the rotation
            tight = both & (tol < 2e-3 * (1 + ref))
            if tight.any():
                worst = max(worst, np.abs(e - ref)[tight].max())
    print("reprojection_error: device worst difference %.3g px where the tolerance is the plain 1e-3" % worst)
    f = int(fx["rpx_cam"])
    n = len(fx["rpx_t"])
    e = B.pose_reproj(obj8(fx, f, n, np.float32), fx["rpx_corners"], fx["cam17"][f], np.tile(np.eye(3).ravel(), (n, 1)), fx["rpx_t"])
    assert np.isfinite(e).all() and np.abs(e - fx["rpx_err"]).max() <= 1e-3 * (1 + fx["rpx_err"].max()), (e, fx["rpx_err"])


def test_solve_marker_equals_its_two_halves(fx):
    """solve_marker (one lane doing both solutions) against the two solve_marker_half results put together as k_marker_poses does:
    equal bit for bit on every case, the degenerate ones included."""
    n = 0
    for f, idx in families(fx, valid_only=False):
        c, size, cam = fx["corners"][idx], fx["fam_size"][f], fx["cam17"][f]
        whole, a, b = B.pose_solve(c, size, cam), B.pose_solve_half(c, size, cam, 0), B.pose_solve_half(c, size, cam, 1)
        a_first = a[:, 0] < b[:, 0]
        first, second = np.where(a_first[:, None], a, b), np.where(a_first[:, None], b, a)
        put = np.concatenate([first[:, 1:4], first[:, 4:7], second[:, 1:4], second[:, 4:7], first[:, :1], second[:, :1]], 1)
        assert np.array_equal(bits(whole), bits(np.ascontiguousarray(put))), (str(fx["fam_names"][f]), whole, put)
        n += len(idx)
    assert n == fx.n
