"""CPU tests of tests/essential_ref.cpp, the restatement the GPU tests of OptimizeEssentialGraph are measured against: g2o::Sim3's
exponential and logarithm in each of their four branches against the matrix exponential in numpy, the numeric Jacobian against
numpy differences, a consistent graph, the ring that is pulled back to its truth, and the conditions the parity tests put on their
cases (tests/essential_parity.py)."""
import numpy as np
import pytest

import essential_build as B
import essential_cases as S
import essential_parity as P

EPS = np.finfo(np.float64).eps


def _expm(M):
    """the matrix exponential by scaling and squaring of its Taylor series"""
    k = max(0, int(np.ceil(np.log2(max(np.abs(M).sum(axis=1).max(), 1e-300)))) + 4)
    A = M / 2.0 ** k
    out, term = np.eye(len(M)), np.eye(len(M))
    for i in range(1, 30):
        term = term @ A / i
        out = out + term
    for _ in range(k):
        out = out @ out
    return out


def _generator(u):
    w, v, s = u[:3], u[3:6], u[6]
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + s * np.eye(3)
    G[:3, 3] = v
    return G


def _matrix(sim):
    """[s R t; 0 1] of quaternion x y z w, t, s -- the quaternion as it is, not normalised, as g2o rotates with it"""
    x, y, z, w = sim[:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = sim[7] * R
    M[:3, 3] = sim[4:7]
    return M


AX, UP = np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74]), np.array([0.4, -1.1, 0.8])
# |sigma| < 1e-5 or not, theta < 1e-5 (d > 1 - 1e-5 needs theta < 4.5e-3: log's own threshold is on the cosine) or not
BRANCHES = {"small_small": (2e-6, 3e-6), "large_theta": (0.7, 3e-6), "large_sigma": (2e-6, 0.25), "large_large": (0.7, -0.3), "log_small_d": (2e-3, 0.25)}


@pytest.mark.parametrize("name", sorted(BRANCHES))
def test_exp_and_log_against_the_matrix_exponential(name):
    """Tolerance: where a branch replaces the series by its first terms (R = I + Omega + Omega^2, omega = deltaR / 2, A = 1/2, B = 1/6)
    g2o's own truncation is theta^2 (the Omega^2 term is twice the series' term) or sigma; elsewhere 1e3 eps for the few dozen
    operations, divided by the smallest divisor of the closed forms (theta^2 or sigma^2) where that is small."""
    theta, sigma = BRANCHES[name]
    u = np.concatenate([theta * AX, UP, [sigma]])
    S8 = B.sim_exp(u)
    small_t, small_s = theta < 1e-5, abs(sigma) < 1e-5
    tol = 1e3 * EPS + (theta ** 2 if small_t else 0) + (abs(sigma) if small_s else 0) * 2
    if small_t and not small_s:
        # g2o's B of this branch is ((sigma^2 / 2 - sigma + 1) s) / sigma^3, the limit's numerator without its "- 1": W is off by
        # Omega^2 / sigma^3, the translation by theta^2 |upsilon| / |sigma|^3.  The restatement keeps it, as the library does.
        tol += theta ** 2 * np.linalg.norm(UP) / abs(sigma) ** 3
    assert np.abs(_matrix(S8) - _expm(_generator(u))).max() <= tol * 4, name
    # log(exp(v)) = v and exp(log(S)) = S: log's small branch is on d > 1 - 1e-5, i.e. theta < 4.5e-3, where omega = deltaR / 2 errs by theta^3 / 6
    back = B.sim_log(S8)
    tol_log = 1e3 * EPS / min(1.0, theta) + (theta ** 2 if theta < 4.5e-3 else 0) * 4 + (abs(sigma) * 2 if small_s else 0)
    if theta < 4.5e-3 and not small_s:
        tol_log += theta ** 2 * np.linalg.norm(UP) / abs(sigma) ** 3 * 2
    assert np.abs(back - u).max() <= tol_log * 4, (name, back - u)
    again = B.sim_exp(back)
    assert np.abs(_matrix(again) - _matrix(S8)).max() <= tol_log * 8, name


def test_product_and_inverse_are_the_matrices():
    rng = np.random.default_rng(0)
    for _ in range(20):
        a, b = B.sim_exp(rng.uniform(-1, 1, 7)), B.sim_exp(rng.uniform(-1, 1, 7))
        assert np.abs(_matrix(B.sim_mul(a, b)) - _matrix(a) @ _matrix(b)).max() <= 1e3 * EPS
        assert np.abs(_matrix(B.sim_mul(a, B.sim_inverse(a))) - np.eye(4)).max() <= 1e3 * EPS


def _error(C, vi, vj):
    return B.sim_log(B.sim_mul(B.sim_mul(C, vi), B.sim_inverse(vj)))


@pytest.mark.parametrize("fix_scale", [0, 1])
def test_numeric_jacobian_against_numpy_differences(fix_scale):
    """central differences with h = 1e-5 through Sim3(update) * estimate in numpy, against g2o's with 1e-9: the latter's rounding is
    16 eps E / 2e-9 for values up to E (here 10), the former's truncation h^2 times a third derivative of order E"""
    rng = np.random.default_rng(4)
    E = 10.0
    for _ in range(5):
        vi, vj = B.sim_exp(rng.uniform(-1, 1, 7) * [1, 1, 1, 5, 5, 5, 0.2]), B.sim_exp(rng.uniform(-1, 1, 7) * [1, 1, 1, 5, 5, 5, 0.2])
        C = B.sim_mul(B.sim_exp(rng.uniform(-0.05, 0.05, 7)), B.sim_mul(vj, B.sim_inverse(vi)))
        err, Ji, Jj = B.edge(C, vi, vj, fix_scale)
        assert np.array_equal(err, _error(C, vi, vj))
        h = 1e-5
        for side, J in ((0, Ji), (1, Jj)):
            for d in range(7):
                u = np.zeros(7); u[d] = h
                if fix_scale:
                    u[6] = 0
                plus = _error(C, B.sim_mul(B.sim_exp(u), vi), vj) if side == 0 else _error(C, vi, B.sim_mul(B.sim_exp(u), vj))
                minus = _error(C, B.sim_mul(B.sim_exp(-u), vi), vj) if side == 0 else _error(C, vi, B.sim_mul(B.sim_exp(-u), vj))
                assert np.abs(J[:, d] - (plus - minus) / (2 * h)).max() <= 16 * EPS * E / 2e-9 + 10 * E * h * h, (side, d)
        if fix_scale:
            assert not Ji[:, 6].any() and not Jj[:, 6].any()


def test_a_consistent_graph_has_no_error_and_returns_its_input():
    """chi2 = 0 up to what a float pose is: its rotation is orthonormal to 2^-24 an entry, g2o keeps the quaternion it makes of it as it
    is, and conjugate is then not quite inverse: an error entry is at most 8 * 2^-24 * E."""
    pb = S.consistent()
    E = S.extent(pb)
    ne = len(pb["edge_i"])
    lin = B.inspect(pb)
    assert np.abs(lin["err"]).max() <= 8 * 2.0 ** -24 * E and lin["chi2"] <= ne * 7 * (8 * 2.0 ** -24 * E) ** 2
    out = B.optimize(pb)
    ulp = np.spacing(np.float32(E))
    assert np.abs(out["Tcw"] - pb["Tcw"]).max() <= 4 * ulp and np.abs(out["x3Dw"] - pb["x3Dw"]).max() <= 4 * ulp
    none = dict(pb, edge_i=[], edge_j=[], edge_kind=[])
    out = B.optimize(none)
    assert np.array_equal(out["Tcw"], pb["Tcw"]) and np.array_equal(out["x3Dw"], pb["x3Dw"]) and out["result"]["iterations"] == 0


def _to_truth(T, truth):
    rot = float(np.linalg.norm((T[:, :, :3].astype(np.float64) - truth[:, :, :3]).reshape(len(T), -1), axis=1).max() / np.sqrt(2))
    return rot, float(np.abs(T[:, :, 3] - truth[:, :, 3]).max() / S.extent())


def test_the_ring_is_pulled_to_its_truth():
    """24 keyframes, slow drift, the last four corrected onto the truth, loop connections to the first three: within the bound the case
    builder derives from its own drift step, and closer than it started"""
    pb = S.case("ring24_slow")
    assert len(pb["Tcw"]) == 24 and pb["corrected_pos"].tolist() == [20, 21, 22, 23] and pb["edge_kind"][:3].tolist() == [0, 0, 0]
    before = _to_truth(pb["Tcw"], pb["truth"])
    for order in (B.CALLER, P.reversed_order(pb)):
        out = B.optimize(pb, order)
        after = _to_truth(out["Tcw"], pb["truth"])
        print("before", before, "after", after, "bound", pb["bound"], out["result"])
        assert after[0] <= pb["bound"]["rot"] and after[1] <= pb["bound"]["trans"]
        assert after[0] < before[0] and after[1] < before[1]
        assert out["result"]["chi2_last"] < 0.01 * out["result"]["chi2_first"]


def test_the_two_kinds_of_edge_measure_differently():
    """kind 1 reads NonCorrectedSim3 where the keyframe has an entry, kind 0 never does"""
    pb = S.case("chain3")
    a = B.inspect(pb)
    flipped = dict(pb, edge_kind=1 - np.asarray(pb["edge_kind"]))
    b = B.inspect(flipped)
    touching = np.isin(pb["edge_i"], pb["noncorrected_pos"]) | np.isin(pb["edge_j"], pb["noncorrected_pos"])
    assert touching.any() and all(np.abs(a["err"][e] - b["err"][e]).max() > 1e-6 for e in np.nonzero(touching)[0])
    assert all(np.array_equal(a["err"][e], b["err"][e]) for e in np.nonzero(~touching)[0])


def test_conditions_on_the_cases_of_the_gpu_tests():
    """Every case the GPU runs whole is decided at the reference's 20 iterations (tests/essential_parity.py), and there the two orders
    agree on the iteration and trial counts: a parity failure cannot be a marginal rho.  Between them the cases end on the stop rules:
    three small gains in a row, and ten rejected trials."""
    s = P.spread()
    print({k: v for k, v in s.items() if k != "per_case"})
    endings = set()
    for name in P.NAMES:
        pb, r0, r1 = P.problem(name)
        print(name, P.counts(r0), P.counts(r1), "margins", r0["result"]["margin"], r1["result"]["margin"], s["per_case"][name])
        assert pb["iterations"] == 20 and P.counts(r0)[0] < 20, name
        assert P.decided(name), (name, P.margin(name))
        assert P.counts(r0) == P.counts(r1), name
        endings.add("ten_rejections" if P.counts(r0)[1] >= P.counts(r0)[0] + 9 else "small_gains")
    assert endings == {"ten_rejections", "small_gains"}
    for a, b in S.PAIRS:       # the same problem under two plans
        assert all(np.array_equal(S.case(a)[k], S.case(b)[k]) for k in ("Tcw", "edge_i", "edge_j", "edge_kind", "corrected", "noncorrected", "x3Dw"))
        assert S.case(a)["leaf_vertices"] in (2, 4) and S.case(b)["leaf_vertices"] == 64
    assert {P.group(n) for n in P.NAMES} == {"fix_scale", "free_scale"}
    for name in S.CASES:
        pb = S.case(name)
        assert len(pb["Tcw"]) <= 48 and len(pb["edge_i"]) <= 300 and len(pb["x3Dw"]) <= 200


def test_the_not_solved_case_is_never_solved():
    """tests/essential_cases.not_solved: NaN errors from finite inputs, every solve refused, the estimates returned as they came"""
    pb = S.not_solved()
    lin = B.inspect(pb)
    assert not lin["solved"] and np.isnan(lin["chi2"]) and np.isnan(lin["err"]).any() and np.isfinite(pb["corrected"]).all()
    out = B.optimize(pb)
    assert (out["result"]["iterations"], out["result"]["trials"]) == (20, 20)
    clean = B.optimize(dict(pb, iterations=0))
    assert np.array_equal(out["Siw"], clean["Siw"]) and np.array_equal(out["Tcw"], clean["Tcw"])
