"""Unit tests of the device helpers of the optimizers and solvers, on the GPU against plain references:

  A  csrc/se3_quat.hpp     g2o's SE3Quat: product, map, normalisation, exp in both branches, the float conversions
  B  csrc/sim3_group.hpp   g2o::Sim3: product, map, inverse, exp and log in their 2 x 2 branches, the pivoted 3 x 3 solve
  C  csrc/svd_jacobi.hpp   OpenCV's float Jacobi SVD in its four product instantiations
  D  csrc/front_solve.hpp  the partial Cholesky of a front in both storage forms, the substitution back
  E  csrc/ba_edges.hpp     the mono edge's analytic Jacobians, the marker edge's numeric ones, the diagonal block, the wave sums
  F  the steps the passes of the bundle adjustments and the front solvers share: the damped 3 x 3 inverse and the pair item
     (ba_edges.hpp), the children's merge (front_solve.hpp), run_sum behind block_sum (lm_dense.hpp), each bit-equal to a sequential
     restatement in tests/solver_units_host.cpp

The helpers run inside tests/solver_units_probe.hip: the five headers, included unchanged, as a translation unit of their own that
tests/solver_units_build.py compiles with the library's flags.  Inputs and references are in tests/solver_units_cases.py;
tests/test_solver_units_cpu.py checks on the CPU that they are what these tests need and measures the host side.

Three kinds of assertion.  (1) Bit equality with a plain double evaluation in the helper's own order, where only + - * / and sqrt
enter (the flags keep contraction off, divide and sqrt are correctly rounded); the CPU test shows for each that another order gives
other bits.  (2) Where the device's libm enters: the error against g2o's closed form at 50 digits, bounded by BOUND = max(4 x the
worst error of the CPU restatement (glibc) over the same inputs, the group's floor), the convention of test_ldlt_solve; both sides
are printed.  (3) Truth against the definition.  The numeric Jacobians use test_essential_cpu's tolerance as it is.  The
tolerances against the matrix exponential (solver_units_cases.se3_truth_tolerance, sim3_truth_tolerance) are not the project's own
but extend that test's formula in two ways, because its five inputs have |u| about 1 and no small divisor and these classes do: its
1e3 eps is divided by min(1, theta, |sigma|) of the large branches (the divisor its docstring names, as its tol_log divides), and the
whole is scaled by max(1, |u|), up to 5 here; the round trips' tol_log has the second extension only.  SE3Quat's small branch adds
its own truncation theta |upsilon| on t (V = R there).

Measured, host (glibc, x86-64) / device (MI355X), worst errors in the units each test states.  In all but one class the worst input
gives the same bits on both sides:
  se3_exp    tiny 0.90 / 0.90   zero 0 / 0   cancel 15258 / 15258   large 190 / 190   threshold 1864 / 1864
  sim3_exp   small_small 1.34 / 1.34   large_theta 23.5 / 23.5   large_sigma 6.04 / 6.04   large_large 5.23 / 5.23
             theta_threshold 1864 / 1864   sigma_threshold 44079 / 44079
  sim3_log   small_small 1.34 / 1.34   large_d 8.13 / 8.13   log_small_d 2.34 / 2.34   large_large 6.68 / 7.43   products 2.60 / 2.60
  svd        worst ratio of any class: 3x3 2.77, 4x4 4.45, 16x9 7.35, 9x8 7.63 FLT_EPSILON on both sides; all 324 matrices of each
             instantiation are bit-equal to the restatement (W, Vt, and U where it is asked for)
  front      rounded class at all nine shapes, worst of L11, L21, Schur, r: device 0.055, numpy 0.036 (the device's worst at n = 168
             and 280: 0.026 and 0.018); substitution: device 0.034, numpy 0.021 (eps kappa)
The large figures of `cancel`, `large` and the thresholds are g2o's closed forms, not a libm: b = (1 - cos theta) / theta^2 loses
eps / theta^2 and enters the translation through V = I + b Omega + c Omega^2 with one factor theta, so t carries eps / theta; C =
(exp(sigma) - 1) / sigma does the same with sigma (tests/test_solver_units_cpu.py)."""
import numpy as np
import pytest

import solver_units_build as B
import solver_units_cases as S

pytestmark = pytest.mark.gpu

bits, same_bits = S.bits, S.same_bits
SE3_FLOOR, SIM3_FLOOR, SIM3_LOG_FLOOR = S.SE3_FLOOR, S.SIM3_FLOOR, S.SIM3_LOG_FLOOR


def bound(host_worst, floor):
    return max(4 * host_worst, floor)


def first_difference(got, want):
    bad = np.flatnonzero((bits(np.asarray(got)).reshape(len(got), -1) != bits(np.asarray(want)).reshape(len(want), -1)).any(1))
    return len(bad), (int(bad[0]), np.asarray(got)[bad[0]], np.asarray(want)[bad[0]]) if len(bad) else None


def test_probe_sees_a_gpu():
    assert B.probe().su_device_count() >= 1


# ====================================================================================== A. se3_quat.hpp
def test_se3_mul_map_and_normalize_equal_the_plain_evaluation():
    """kind 1; the product and map also against the 4 x 4 matrices at 50 digits (1e3 eps, test_product_and_inverse's tolerance)"""
    a, b, p = S.se3_pairs()
    got_mul, got_map = B.se3_mul(B.probe(), a, b), B.se3_map(B.probe(), a, p)
    assert same_bits(got_mul, B.se3_mul(B.host(), a, b)), first_difference(got_mul, B.se3_mul(B.host(), a, b))
    assert same_bits(got_map, B.se3_map(B.host(), a, p)), first_difference(got_map, B.se3_map(B.host(), a, p))
    for i in range(0, len(a), 10):
        E = max(1.0, np.abs(a[i]).max(), np.abs(b[i]).max(), np.abs(p[i]).max()) ** 2
        assert S.max_abs(S.matrix_of(got_mul[i]) - S.matrix_of(a[i]) * S.matrix_of(b[i])) <= 1e3 * S.EPS * E
        want = S.matrix_of(a[i]) * S.MP.matrix([float(c) for c in p[i]] + [1])
        assert max(abs(float(S.MP.mpf(float(got_map[i][c])) - want[c])) for c in range(3)) <= 1e3 * S.EPS * E
    q = S.normalize_inputs()
    got = B.normalize(B.probe(), q)
    assert same_bits(got, B.normalize(B.host(), q)), first_difference(got, B.normalize(B.host(), q))
    # the edges, stated: -0.0 is not negative, a zero quaternion and one whose n2 underflows stay as they are (the latter negated)
    assert same_bits(got[-6], q[-6]) and same_bits(got[-5], q[-5]) and same_bits(got[-4], q[-4]) and same_bits(got[-3], q[-4])
    assert np.signbit(got[-7, 3]) and got[-7, 1] < 0 < got[-7, 0]


def test_se3_float_conversions_equal_the_plain_evaluation():
    """kind 1: se3_from_float on every branch of quat_from_matrix, to_float of the result and of random poses"""
    Rt = S.float_poses()
    got = B.se3_from_float(B.probe(), Rt)
    assert same_bits(got, B.se3_from_float(B.host(), Rt)), first_difference(got, B.se3_from_float(B.host(), Rt))
    poses = np.concatenate([got, S.se3_pairs()[0]])
    back = B.to_float(B.probe(), poses)
    assert same_bits(back, B.to_float(B.host(), poses)), first_difference(back, B.to_float(B.host(), poses))


@pytest.mark.parametrize("name", ["tiny", "zero", "threshold"])
def test_se3_exp_small_branch_equals_the_plain_evaluation(name):
    """kind 1 below theta = 1e-5 (sqrt only).  At the threshold the device took the branch the double theta selects: its result is the
    closed form of that branch, and the other closed form is |Omega upsilon| / 2 ~ 5e-6 away in t (V = R = I + Omega + Omega^2 below
    the threshold, I + Omega / 2 + ... above; the large branch's own rounding there is eps / theta ~ 1e-11)."""
    u = S.se3_exp_inputs()[name]
    got, want = B.se3_exp(B.probe(), u), B.se3_exp(B.host(), u)
    small = np.array([S.se3_small(x) for x in u])
    assert same_bits(got[small], want[small]), first_difference(got[small], want[small])
    if name == "threshold":
        for x, g in zip(u, got):
            stated, other = np.array(S.se3_exp_form(x, S.se3_small(x))), np.array(S.se3_exp_form(x, not S.se3_small(x)))
            assert np.abs(g - stated).max() <= 1e-3 * np.abs(stated - other).max(), (x, g, stated, other)


@pytest.mark.parametrize("name", ["tiny", "zero", "cancel", "large", "threshold"])
def test_se3_exp_error_against_the_closed_form(name):
    """kind 2, unit eps max(1, |u|) on q and t, floor 16"""
    u = S.se3_exp_inputs()[name]
    host, dev = S.se3_exp_worst(name, B.se3_exp(B.host(), u)), S.se3_exp_worst(name, B.se3_exp(B.probe(), u))
    print("se3_exp", name, "host", host, "device", dev, "bound", bound(host, SE3_FLOOR))
    assert dev <= bound(host, SE3_FLOOR)


@pytest.mark.parametrize("name", ["tiny", "cancel", "large", "threshold"])
def test_se3_exp_is_the_matrix_exponential(name):
    """kind 3: [R t; 0 1] against expm of the generator at 50 digits, every fifth input"""
    u = S.se3_exp_inputs()[name]
    got = B.se3_exp(B.probe(), u)
    for x, g in list(zip(u, got))[::5]:
        assert S.max_abs(S.matrix_of(g) - S.MP.expm(S.generator(x))) <= S.se3_truth_tolerance(x), x


# ====================================================================================== B. sim3_group.hpp
def test_sim3_mul_map_and_inverse_equal_the_plain_evaluation():
    """kind 1 on exponentials (their quaternions are not normalised in the small branch); S inverse(S) is the identity"""
    u = np.concatenate([S.sim3_exp_inputs()[n][:50] for n in S.SIM3_EXP_CLASSES])
    a = B.sim3_exp(False, u)
    b, p = a[::-1].copy(), S.se3_pairs()[2][:len(a)]
    for name, got, want in (("mul", B.sim3_mul(True, a, b), S.sim3_mul_plain(a, b)), ("map", B.sim3_map(True, a, p), S.sim3_map_plain(a, p)),
                            ("inverse", B.sim3_inverse(True, a), S.sim3_inverse_plain(a))):
        assert same_bits(got, want), (name, first_difference(got, want))
    one = B.sim3_mul(True, a, B.sim3_inverse(True, a))
    for i in range(0, len(a), 10):
        assert S.max_abs(S.matrix_of(one[i]) - S.MP.eye(4)) <= 1e3 * S.EPS * max(1.0, np.abs(a[i]).max()), i


@pytest.mark.parametrize("name", sorted(S.sim3_exp_inputs()))
def test_sim3_exp_error_and_truth(name):
    """kind 2 (unit eps max(1, |u|) on q, t, s; floor 16) and, on every fifth input, kind 3 against expm; at the thresholds the device
    took the branches the double theta and sigma select"""
    u = S.sim3_exp_inputs()[name]
    got = B.sim3_exp(True, u)
    host, dev = S.sim3_exp_worst(name, B.sim3_exp(False, u)), S.sim3_exp_worst(name, got)
    print("sim3_exp", name, "host", host, "device", dev, "bound", bound(host, SIM3_FLOOR))
    assert dev <= bound(host, SIM3_FLOOR)
    for x, g in list(zip(u, got))[::5]:
        assert S.max_abs(S.matrix_of(g) - S.MP.expm(S.generator(x))) <= S.sim3_truth_tolerance(x), x
    if name == "theta_threshold":
        for x, g in zip(u, got):
            st, ss = S.sim3_exp_branches(x)
            stated, other = np.array(S.sim3_exp_form(x, st, ss)), np.array(S.sim3_exp_form(x, not st, ss))
            assert np.abs(g - stated)[:4].max() <= 1e-3 * np.abs(stated - other)[:4].max(), (x, g, stated, other)


_LOG = {}


def _log_inputs():
    if not _LOG:
        _LOG.update(S.sim3_log_inputs(lambda u: B.sim3_exp(True, u)))
    return _LOG


@pytest.mark.parametrize("name", sorted(S.SIM3_LOG_CLASSES) + ["products"])
def test_sim3_log_error_against_the_closed_form(name):
    """kind 2 on the device's own exponentials, as in the product.  Unit eps max(1, |S|), over sqrt(1 - d^2) where omega comes from
    acos(d): d carries eps and acos' slope is 1 / sqrt(1 - d^2) there.  Floor 32 (solver_units_cases.SIM3_LOG_FLOOR)."""
    s8 = _log_inputs()[name]
    if name in S.SIM3_LOG_CLASSES:
        assert all(S.log_branches(x) == S.SIM3_LOG_CLASSES[name] for x in s8)
    host, dev = S.sim3_log_worst(s8, B.sim3_log(False, s8)), S.sim3_log_worst(s8, B.sim3_log(True, s8))
    print("sim3_log", name, "host", host, "device", dev, "bound", bound(host, SIM3_LOG_FLOOR))
    assert dev <= bound(host, SIM3_LOG_FLOOR)


@pytest.mark.parametrize("name", sorted(S.SIM3_LOG_CLASSES))
def test_sim3_round_trips(name):
    """kind 3: log(exp(u)) = u and exp(log(S)) = S within test_essential_cpu's tol_log"""
    u, s8 = S.sim3_log_sources()[name], _log_inputs()[name]
    back = B.sim3_log(True, s8)
    again = B.sim3_exp(True, back)
    for x, b, s, a in zip(u, back, s8, again):
        tol = S.sim3_tol_log(x)
        assert np.abs(b - x).max() <= 4 * tol, (x, b - x)
        assert S.max_abs(S.matrix_of(a) - S.matrix_of(s)) <= 8 * tol, x


def test_lu3_solve():
    """kind 1.  Dyadic systems whose elimination is exact in doubles: the device equals the rational solution on each of the six pivot
    paths, ties included.  Random systems: bit-equal to the header's order.  A zero column: the restatement's not finite result."""
    sy = S.lu3_systems()
    got = B.lu3(True, sy["A"], sy["b"])
    assert np.array_equal(got, sy["x"]), [(sy["path"][i], sy["tie"][i]) for i in np.flatnonzero((got != sy["x"]).any(1))][:5]
    A, b = S.lu3_rounded()
    got = B.lu3(True, A, b)
    assert same_bits(got, S.lu3_plain(A, b)), first_difference(got, S.lu3_plain(A, b))
    A, b = S.lu3_zero_column()
    got, want = B.lu3(True, A, b), B.lu3(False, A, b)
    assert not np.isfinite(want).all(1).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


# ====================================================================================== C. svd_jacobi.hpp
@pytest.mark.parametrize("shape", sorted(S.SVD_SHAPES))
def test_svd_jacobi(shape):
    """Every ratio of solver_units_cases.svd_measures within max(4 x the restatement's, 16) FLT_EPSILON, W descending, class by class;
    the denormal class (every W <= FLT_MIN: the fill path makes all of U) against the restatement only: U bit for bit (the fill has no
    hypot), Vt bit for bit, W within 4 denormal steps.  Printed, not asserted: how many matrices are bit-equal to the restatement (hypot is the only
    inexact call)."""
    M, N, N1, want_u = S.SVD_SHAPES[shape]
    equal = total = 0
    for cls in S.SVD_CLASSES:
        At = S.svd_inputs(shape, cls)
        W, Vt, out = B.svd(True, shape, At)
        hW, hVt, hout = B.svd(False, shape, At)
        same = (bits(W) == bits(hW)).all(1) & (bits(Vt) == bits(hVt)).all((1, 2))
        if want_u:
            same &= (bits(out) == bits(hout)).all((1, 2))
        equal, total = equal + int(same.sum()), total + len(At)
        if cls == "denormal":
            # Vt bit for bit: of the rotations only hypot is inexact, and its last double bit reaches the float c and s once in 2^29
            assert np.abs(W.astype(np.float64) - hW).max() <= 4 * 2.0 ** -149 and same_bits(Vt, hVt)
            if want_u:
                assert (W <= np.finfo(np.float32).tiny).all() and same_bits(out, hout)
            continue
        dev, host = S.svd_measures(shape, At, W, Vt, out, True), S.svd_measures(shape, At, hW, hVt, hout, False)
        print("svd", shape, cls, "host", {k: round(host[k], 2) for k in S.SVD_RATIOS}, "device", {k: round(dev[k], 2) for k in S.SVD_RATIOS})
        assert dev["descending"], cls
        for k in S.SVD_RATIOS:
            assert dev[k] <= bound(host[k], S.SVD_FLOOR), (cls, k, dev[k], host[k])
        if cls in ("three_i", "equal_values", "zero"):
            # no pair rotates: W is the columns' norms sorted by a strict '<' and Vt that permutation, as OpenCV's sort is described
            # (solver_units_cases.selection_sort), not as the restatement finds them
            eW, eVt = S.svd_unrotated_expected(shape, cls)
            assert same_bits(W, eW) and same_bits(Vt, eVt), cls
    print("svd", shape, "bit-equal to the restatement:", equal, "of", total)


# ====================================================================================== D. front_solve.hpp
def _lower(F):
    return np.tril(F)


@pytest.mark.parametrize("shape", S.FRONT_SHAPES, ids=str)
def test_front_partial_llt_exact(shape):
    """M = L L^T with dyadic L: both storage forms give L11, L21, the Schur complement L22 L22^T and r exactly, and leave the upper
    triangle and the guard words alone.  k == 0 keeps every bit of M and r."""
    n, k = S.front_dims(shape)
    c = S.front_exact(shape)
    wantF, wantr = S.front_exact_expected(shape)
    for packed in ([False, True] if n <= S.FRONT_PACKED_MAX else [False]):
        F, r, ret, fail, kept = B.front_llt(packed, c["M"], k, c["r"])
        assert kept and (ret == 1).all() and (fail == 0).all(), packed
        assert np.array_equal(np.tril(F), np.tril(wantF)) and np.array_equal(r, wantr), packed
        assert same_bits(np.triu(F, 1), np.triu(c["M"], 1)), packed
        if k == 0:
            assert same_bits(F, c["M"]) and same_bits(r, c["r"])


@pytest.mark.parametrize("shape", S.FRONT_ROUNDED_SHAPES, ids=str)
def test_front_partial_llt_rounded(shape):
    """Random positive definite systems, kappa up to 1e8: both storage forms equal the sequential right-looking loop bit for bit
    (kind 1) on every system at every shape (n = 280 in rows of n only: its triangle does not fit LDS; n = 168 is the packed case that
    needs more than 48 KB of it), and L11, L21, the Schur complement and r are within max(4 x numpy's cholesky and solves, 4) eps
    kappa of the 50-digit factorisation (solver_units_cases.front_mp_plan: everything up to n = 56, two systems and every seventh row
    of the Schur complement at n = 168 and 280)"""
    n, k = S.front_dims(shape)
    c = S.front_rounded(shape)
    F0, r0, ret, fail, kept = B.front_llt(False, c["M"], k, c["r"])
    assert kept and (ret == 1).all() and not fail.any()
    if n <= S.FRONT_PACKED_MAX:
        F1, r1, ret1, fail1, kept1 = B.front_llt(True, c["M"], k, c["r"])
        assert kept1 and (ret1 == 1).all() and not fail1.any()
        assert same_bits(F0, F1) and same_bits(r0, r1)
    for s in range(len(c["M"])):
        Fs, rs, ok = S.front_sequential(c["M"][s], k, c["r"][s])
        assert ok and same_bits(F0[s], Fs) and same_bits(r0[s], rs), s
    worst = {}
    systems, schur_rows = S.front_mp_plan(shape)
    for s in systems:
        Fm, rm = S.front_mp(c["M"][s], k, c["r"][s], schur_rows)
        want = S.front_parts(np.array(Fm, object), np.array(rm, object), k)
        dev, ref = S.front_parts(F0[s], r0[s], k), S.front_parts(*S.front_numpy(c["M"][s], k, c["r"][s]), k)
        for part in want:
            h, d = S.front_ratio(ref[part], want[part], c["kappa"][s]), S.front_ratio(dev[part], want[part], c["kappa"][s])
            worst[part] = max(worst.get(part, (0, 0)), (d, h))
            assert d <= bound(h, S.FRONT_FLOOR), (s, part, d, h)
    print("front", shape, "worst (device, numpy there)", worst)


@pytest.mark.parametrize("shape", S.FRONT_FAIL_SHAPES, ids=str)
def test_front_partial_llt_failing_pivot_is_a_return_value(shape):
    """a first zero, negative, NaN or infinite pivot at column 0, in the middle and at k - 1: false in every thread, fail_s 1, the
    kernel ends, the guard words around M and r are kept, and M and r are what the sequential loop holds where it stops (rows of n) or
    M as it came (the LDS copy is not written back)"""
    n, k = S.front_dims(shape)
    cases = S.front_failing(shape)
    M, r = np.array([c[2] for c in cases]), np.array([c[3] for c in cases])
    for packed in (False, True):
        F, rr, ret, fail, kept = B.front_llt(packed, M, k, r)
        assert kept and (ret == 0).all() and (fail == 1).all(), packed
        for s, (name, col, Ms, rs) in enumerate(cases):
            Fs, rq, ok = S.front_sequential(Ms, k, rs)
            assert not ok and same_bits(rr[s], rq), (packed, name)
            assert same_bits(F[s], Ms if packed else Fs), (packed, name)


@pytest.mark.parametrize("shape", [s for s in S.FRONT_SHAPES if s[1] > 0], ids=str)
def test_front_substitute_back(shape):
    """a scattered vtx list and a given boundary solution.  Exact class: the own rows are the dyadic solution exactly.  Rounded class:
    bit-equal to the helper's order, within max(4 x numpy's solve, 4) eps kappa of the 50-digit solution.  Every other row of xt keeps
    its bits."""
    R, nown, nb = shape
    n, k = S.front_dims(shape)
    for rounded in ([False, True] if shape in S.FRONT_ROUNDED_SHAPES else [False]):
        c = S.front_back_cases(shape, rounded)
        xt = B.front_back(R, nown, nb, c["vtx"], c["xt"], c["F"], c["r"])
        worst = (0, 0)
        for s in range(len(xt)):
            own = xt[s, c["vtx"][s, :nown]].ravel()
            other = np.ones(xt.shape[1], bool)
            other[c["vtx"][s, :nown]] = False
            assert same_bits(xt[s, other], c["xt"][s, other]), (rounded, s)
            if not rounded:
                assert np.array_equal(own, c["x_own"][s]), (s, own, c["x_own"][s])
                continue
            assert same_bits(own, S.back_sequential(c["F"][s], c["r"][s], c["xb"][s], k)), s
            want, kappa = S.back_mp(c["F"][s], c["r"][s], c["xb"][s], k), S.front_rounded(shape)["kappa"][s]
            d, h = S.front_ratio(own, want, kappa), S.front_ratio(S.back_numpy(c["F"][s], c["r"][s], c["xb"][s], k), want, kappa)
            worst = max(worst, (d, h))
            assert d <= bound(h, S.FRONT_FLOOR), (s, d, h)
        if rounded:
            print("front_substitute_back", shape, "worst (device, numpy there)", worst)


# ====================================================================================== E. ba_edges.hpp
def test_mono_edge_equals_the_plain_evaluation_and_the_true_derivative():
    """kind 1: err, Jp and Jx.  Kind 3: g2o's column order (rotation first) and signs against the derivative of
    obs - pi(exp(delta) T X) taken at 50 digits: rounding only, 64 eps max |J|."""
    T, X, obs = S.mono_inputs()
    err, Jp, Jx = B.mono(T, X, obs, S.CAM)
    werr, wJp, wJx = S.mono_plain(T, X, obs, S.CAM)
    assert same_bits(err, werr) and same_bits(Jp, wJp) and same_bits(Jx, wJx), (first_difference(Jp, wJp), first_difference(Jx, wJx))
    tJp, tJx = S.mono_true_jacobians()
    for i in range(len(T)):
        tol = 64 * S.EPS * max(np.abs(tJp[i]).max(), np.abs(tJx[i]).max())
        assert np.abs(Jp[i] - tJp[i]).max() <= tol and np.abs(Jx[i] - tJx[i]).max() <= tol, (i, Jp[i] - tJp[i], Jx[i] - tJx[i])


def test_marker_edge_equals_the_restatement_and_the_true_derivative():
    """Both vertices.  The steps of 1e-9 take se3_exp's small branch, so no libm enters: kind 1 against the restatement's entry
    (ref_ba_marker_edge), which is stronger than the kind-2 bound.  Kind 3: the numeric Jacobians against the derivative at 50
    digits with the project's numeric-Jacobian tolerance, E the size of the projected values."""
    Tcw, Twm, p, obs = S.marker_inputs()
    err, Jc, Jm = B.marker(True, Tcw, Twm, p, obs, S.CAM)
    werr, wJc, wJm = B.marker(False, Tcw, Twm, p, obs, S.CAM)
    assert same_bits(err, werr) and same_bits(Jc, wJc) and same_bits(Jm, wJm), (first_difference(Jc, wJc), first_difference(Jm, wJm))
    sc, sm = B.se3_from_float(B.probe(), Tcw), B.se3_from_float(B.probe(), Twm)
    tJc, tJm = S.marker_true_jacobians(tuple(map(tuple, sc)), tuple(map(tuple, sm)))
    E = float(np.abs(obs).max() + np.abs(err).max())
    tol = S.numeric_jacobian_tolerance(E)
    worst = max(np.abs(Jc - tJc).max(), np.abs(Jm - tJm).max())
    print("marker numeric Jacobians: worst", worst, "tolerance", tol, "largest entry", max(np.abs(tJc).max(), np.abs(tJm).max()))
    assert worst <= tol


def test_diag_block_and_rot_of_equal_the_plain_evaluation():
    J, w, r0, r1 = S.diag_inputs()
    got = B.diag_block(J, w, r0, r1)
    assert same_bits(got, S.diag_plain(J, w, r0, r1)), first_difference(got, S.diag_plain(J, w, r0, r1))
    q = np.concatenate([S.se3_pairs()[0][:, :4], S.normalize_inputs()[:50]])
    assert same_bits(B.rot_of(q), S.rot_of_plain(q)), first_difference(B.rot_of(q), S.rot_of_plain(q))


def test_wave_sum_and_max_in_the_butterfly_order():
    """every lane holds the butterfly's result (xor 32, 16, ... 1); a NaN is dropped by fmax: the maximum of the other 63"""
    rows = S.wave_rows()
    assert same_bits(B.wave(B.SUM, rows), S.butterfly(rows, np.add))
    assert same_bits(B.wave(B.MAX, rows), S.butterfly(rows, np.fmax))
    nan = S.wave_rows_with_nan()
    got = B.wave(B.MAX, nan)
    assert same_bits(got, S.butterfly(nan, np.fmax)) and same_bits(got[:, 0], np.fmax.reduce(nan, axis=1)) and np.isfinite(got).all()


# ====================================================================================== the steps the passes share
# each held to the sequential host restatement of tests/solver_units_host.cpp, bit for bit (only + - * / enter)
def test_damped_inverse_equals_the_restatement():
    H6, lam, _ = S.dinv_inputs()
    got, want = B.dinv3(B.probe(), H6, lam), B.dinv3(B.host(), H6, lam)
    assert same_bits(got, want), first_difference(got, want)


@pytest.mark.parametrize("nitems,diag", S.PAIR_CASES)
def test_pair_item_equals_the_restatement(nitems, diag):
    args = S.pair_inputs(nitems, diag)
    got, want = B.pair_items(B.probe(), *args[:4], diag, *args[4:]), B.pair_items(B.host(), *args[:4], diag, *args[4:])
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (first_difference(got[0], want[0]), first_difference(got[1], want[1]))


@pytest.mark.parametrize("R", (6, 7))
def test_children_merge_equals_the_restatement(R):
    desc, cmap, fronts = S.merge_case(R)
    for node in (0, 3):        # both children, left then right; the right child alone
        got, want = B.merge(B.probe(), R, desc, cmap, fronts, node), B.merge(B.host(), R, desc, cmap, fronts, node)
        assert same_bits(got, want), (node, np.flatnonzero(bits(got) != bits(want))[:8])


@pytest.mark.parametrize("n", S.RUN_SUM_SIZES)
def test_run_sum_then_block_sum_equals_the_restatement(n):
    assert B.probe().su_lm_threads() == B.host().se3.su_lm_threads() == S.RUN_SUM_THREADS
    v = S.run_sum_inputs(n)
    got, want = B.run_sum(B.probe(), v), B.run_sum(B.host(), v)
    assert same_bits(np.array([got]), np.array([want])), (got, want)
