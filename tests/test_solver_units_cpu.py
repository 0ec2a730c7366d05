"""CPU tests of tests/solver_units_cases.py and the host side of tests/solver_units_build.py: that the cases are what
tests/test_solver_units_gpu.py needs (every named branch and pivot path with its count, a differently ordered evaluation that gives
other bits next to every bit-equality reference but those of the two float conversions, the conditions on the inputs), that the 50-digit references agree with a second
route, what the host restatements' worst errors are, and that the probe compiles for gfx950.

Host restatement, worst errors measured here (glibc, x86-64), in the units the GPU tests use:
  se3_exp    tiny 0.90   zero 0   cancel 15258   large 190   threshold 1864          (eps max(1, |u|))
  sim3_exp   small_small 1.3   large_theta 23.5   large_sigma 6.0   large_large 5.2   theta_threshold 1864   sigma_threshold 44079
  sim3_log   small_small 1.3   large_d 8.1   log_small_d 2.3   large_large 6.7   products 2.6
  svd        no ratio above 7.7 FLT_EPSILON (|Vt Vt^T - I| at 9 x 8); |U^T U - I| of the zero matrix 0.78
  front      numpy's cholesky and solves, and the sequential loop: at most 0.094 eps kappa on any of L11, L21, Schur, r
The classes `cancel`, `large`, `large_theta` and the thresholds do not stay under the floor of 16 in the unit eps max(1, |u|), and no
libm could make them: b = (1 - cos theta) / theta^2 loses eps / theta^2 to cancellation, and while R = I + a Omega + b Omega^2 takes
it with theta^2 (eps, as intended), the translation takes it through V = I + b Omega + c Omega^2 (W = A Omega + ... in Sim3) with one
factor theta only: t carries eps |upsilon| / theta by g2o's construction.  Near |sigma| = 1e-5 with a small angle g2o's B is of order
sigma^-3 (test_essential_cpu describes it).  For these classes the margin below is asserted on the error times theta (times
|sigma|^3 / theta^2 for sigma_threshold's small angles): the bound of the GPU test is 4 x the host's either way."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.linalg

import solver_units_build as B
import solver_units_cases as S

SE3_FLOOR, SIM3_FLOOR, SIM3_LOG_FLOOR = S.SE3_FLOOR, S.SIM3_FLOOR, S.SIM3_LOG_FLOOR


# ====================================================================================== branches and counts
def test_se3_exp_classes_take_their_branches():
    inp = S.se3_exp_inputs()
    for name, small in (("tiny", True), ("zero", True), ("cancel", False), ("large", False)):
        assert len(inp[name]) >= 200 and all(S.se3_small(u) == small for u in inp[name]), name
    th = [S.theta_of(u) for u in inp["tiny"]] + [S.theta_of(u) for u in inp["cancel"]] + [S.theta_of(u) for u in inp["large"]]
    assert min(th) >= 1e-9 and max(th) <= 3.1 and min(S.theta_of(u) for u in inp["cancel"]) >= 1e-5 and max(S.theta_of(u) for u in inp["cancel"]) <= 1e-3
    # the threshold: theta as the header computes it (sum of squares, sqrt) against 1e-5, input by input
    sides = [(float(np.abs(u[:3]).max()), S.theta_of(u), S.se3_small(u)) for u in inp["threshold"]]
    print(sides)
    below, at, above = np.nextafter(1e-5, 0), 1e-5, np.nextafter(1e-5, 1)
    axis = [u for u in inp["threshold"] if np.count_nonzero(u[:3]) == 1]
    assert len(axis) == 9 and len(inp["threshold"]) == 12
    for u in axis:                       # along an axis sqrt(t * t) is t for these three: below is small, 1e-5 and above are not
        t = float(np.abs(u[:3]).max())
        assert S.theta_of(u) == t and S.se3_small(u) == (t == below) and t in (below, at, above)
    assert {s[2] for s in sides} == {True, False}
    # the two closed forms are told apart at the threshold: the small branch takes V = R = I + Omega + Omega^2 where the large one has
    # I + Omega / 2 + ..., so t differs by |Omega upsilon| / 2 ~ 5e-6 (the normalised quaternions differ by theta^3 only)
    for u in inp["threshold"]:
        a, b = np.array(S.se3_exp_form(u, True)), np.array(S.se3_exp_form(u, False))
        assert np.abs(a - b).max() > 1e-6


def test_sim3_classes_take_their_branches():
    inp = S.sim3_exp_inputs()
    for name, want in S.SIM3_EXP_CLASSES.items():
        assert len(inp[name]) >= 200 and all(S.sim3_exp_branches(u) == want for u in inp[name]), name
    assert {S.sim3_exp_branches(u) for u in inp["theta_threshold"]} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {S.sim3_exp_branches(u) for u in inp["sigma_threshold"]} == {(a, b) for a in (True, False) for b in (True, False)}
    for u in inp["theta_threshold"]:
        st, ss = S.sim3_exp_branches(u)
        assert np.abs(np.array(S.sim3_exp_form(u, st, ss)) - np.array(S.sim3_exp_form(u, not st, ss)))[:4].max() > 1e4 * S.EPS
    logs = S.sim3_log_inputs(lambda u: B.sim3_exp(False, u))
    for name, want in S.SIM3_LOG_CLASSES.items():
        assert len(logs[name]) >= 200 and all(S.log_branches(x) == want for x in logs[name]), name
    th = [S.theta_of(u) for u in S.sim3_log_sources()["log_small_d"]]
    assert min(th) > 1e-5 and max(th) < 4.5e-3              # above exp's threshold, below log's: test_essential_cpu's log_small_d
    assert len(logs["products"]) >= 50
    for name, s8 in logs.items():                            # theta <= 3.0: away from the pole of theta / (2 sqrt(1 - d^2)) at pi
        assert all(math.acos(min(1.0, S.log_d(x))) <= 3.0 for x in s8), name
    # the small branch's quaternions are not normalised
    q = logs["small_small"][:, :4]
    assert (np.abs(np.linalg.norm(q, axis=1) - 1) > 0).any()


def test_lu3_systems_take_every_pivot_path():
    sy = S.lu3_systems()
    for path in S.LU3_PATHS:
        assert sy["path"].count(path) >= 20, path
    assert sy["tie"].sum() >= 20 and sy["path"].count((0, False)) >= 20      # ties; a first pivot that needs no swap
    # exact in doubles: the restatement and the plain evaluation give the rational solution itself
    assert np.array_equal(B.lu3(False, sy["A"], sy["b"]), sy["x"]) and np.array_equal(S.lu3_plain(sy["A"], sy["b"]), sy["x"])
    # the second route: mpmath's lu_solve to 1e-30
    for A, b, x in list(zip(sy["A"], sy["b"], sy["x"]))[::10]:
        got = S.MP.lu_solve(S.MP.matrix(A.reshape(3, 3).tolist()), S.MP.matrix(b.tolist()))
        assert max(abs(float(got[i] - S.MP.mpf(float(x[i])))) for i in range(3)) <= 1e-30
    A, b = S.lu3_zero_column()
    assert not np.isfinite(B.lu3(False, A, b)).all(1).any()


# ====================================================================================== order matters
def _differs(a, b):
    return S.rows_differing(a, b) > 0.5


def test_plain_references_are_the_restatements_and_another_order_is_not():
    H = B.host()
    for name in ("tiny", "zero", "threshold"):
        u = np.array([x for x in S.se3_exp_inputs()[name] if S.se3_small(x)])
        host = B.se3_exp(H, u)
        assert S.same_bits(host, [S.se3_exp_form(x, True) for x in u]), name
        if name == "tiny":      # with omega = 0 the result is (0 0 0 1, upsilon) in any order
            assert _differs(host, np.array([S.se3_exp_form(x, True, variant=True) for x in u]))
    a, b, p = S.se3_pairs()
    assert S.same_bits(B.se3_map(H, a, p), S.K.rotate_ref(a[:, :4], p) + a[:, 4:]) and _differs(B.se3_map(H, a, p), S.se3_map_by_matrix(a, p))
    assert _differs(B.se3_mul(H, a, b)[:, 4:], S.se3_mul_by_matrix(a, b))
    qq = S.normalize_plain(S.K.qmul_ref(a[:, :4], b[:, :4]))
    assert S.same_bits(B.se3_mul(H, a, b)[:, :4], qq) and _differs(qq, S.normalize_plain(S.qmul_paired(a[:, :4], b[:, :4])))
    q = S.normalize_inputs()
    assert S.same_bits(B.normalize(H, q), S.normalize_plain(q)) and _differs(B.normalize(H, q), S.normalize_reciprocal(q))
    # se3_from_float is quat_from_matrix and the normalisation, each shown above and in test_device_units_cpu.py; to_float rounds to
    # float, which hides the order of the double operations: these two have no other-order evaluation of their own
    Rt = S.float_poses()
    branches = {S.K.quat_branch(m[:, :3].astype(np.float64)) for m in Rt.reshape(-1, 3, 4)}
    assert branches == {-1, 0, 1, 2}
    # g2o::Sim3
    s = B.sim3_exp(False, np.concatenate([S.sim3_exp_inputs()[n][:50] for n in S.SIM3_EXP_CLASSES]))
    t = s[::-1].copy()
    assert S.same_bits(B.sim3_mul(False, s, t), S.sim3_mul_plain(s, t)) and S.same_bits(B.sim3_inverse(False, s), S.sim3_inverse_plain(s))
    assert S.same_bits(B.sim3_map(False, s, p), S.sim3_map_plain(s, p))
    assert _differs(S.sim3_mul_plain(s, t)[:, :4], S.qmul_paired(s[:, :4], t[:, :4]))
    assert _differs(S.sim3_inverse_plain(s)[:, 4:7], S.sim3_inverse_by_matrix(s)[:, 4:7]) and _differs(S.sim3_map_plain(s, p), S.sim3_map_by_matrix(s, p))
    A, bb = S.lu3_rounded()
    assert S.same_bits(B.lu3(False, A, bb), S.lu3_plain(A, bb)) and _differs(S.lu3_plain(A, bb), S.lu3_plain(A, bb, pivot=False))
    # the edges
    T, X, obs = S.mono_inputs()
    plain, other = S.mono_plain(T, X, obs, S.CAM), S.mono_plain(T, X, obs, S.CAM, variant=True)
    assert _differs(plain[1], other[1]) and _differs(plain[2], other[2])
    qq = np.concatenate([a[:, :4], q[:50]])
    assert _differs(S.rot_of_plain(qq), S.rot_of_one_by_one(qq))
    J, w, r0, r1 = S.diag_inputs()
    assert _differs(S.diag_plain(J, w, r0, r1), S.diag_plain(J, w, r0, r1, variant=True))
    rows = S.wave_rows()
    assert _differs(S.butterfly(rows, np.add)[:, 0], S.left_to_right_sum(rows)) and (S.butterfly(rows, np.add) == S.butterfly(rows, np.add)[:, :1]).all()
    nan = S.wave_rows_with_nan()
    assert np.isnan(nan).sum(1).tolist() == [1] * len(nan) and np.isfinite(S.butterfly(nan, np.fmax)).all()
    assert np.array_equal(S.butterfly(nan, np.fmax)[:, 0], np.fmax.reduce(nan, axis=1))


def test_mono_reference_is_the_true_derivative():
    """the plain evaluation against the derivative from the definition: what the GPU test asks of the device, asked of its reference"""
    T, X, obs = S.mono_inputs()
    err, Jp, Jx = S.mono_plain(T, X, obs, S.CAM)
    tJp, tJx = S.mono_true_jacobians()
    z = S.K.rotate_ref(T[:, :4], X)[:, 2] + T[:, 6]
    assert z.min() < 0.51 and z.max() > 49 and abs(T[-1, 3]) < 1e-8
    nz = np.ones((2, 6), bool)
    nz[0, 4] = nz[1, 3] = False
    assert (np.abs(tJp[:, nz]) > 1e-3).all() and (np.abs(tJx) > 1e-3).all()
    for i in range(len(T)):
        tol = 64 * S.EPS * max(np.abs(tJp[i]).max(), np.abs(tJx[i]).max())
        assert np.abs(Jp[i] - tJp[i]).max() <= tol and np.abs(Jx[i] - tJx[i]).max() <= tol, i
    # a flipped sign or two swapped columns are far outside
    assert np.abs(Jp[:, :, [3, 4, 5, 0, 1, 2]] - tJp).max() > 1 and np.abs(-Jp[:, 0, 1] - tJp[:, 0, 1]).min() > 1


def test_marker_restatement_is_the_true_derivative():
    Tcw, Twm, p, obs = S.marker_inputs()
    err, Jc, Jm = B.marker(False, Tcw, Twm, p, obs, S.CAM)
    sc, sm = B.se3_from_float(B.host(), Tcw), B.se3_from_float(B.host(), Twm)
    tJc, tJm = S.marker_true_jacobians(tuple(map(tuple, sc)), tuple(map(tuple, sm)))
    E = float(np.abs(obs).max() + np.abs(err).max())
    worst = max(np.abs(Jc - tJc).max(), np.abs(Jm - tJm).max())
    print("marker numeric Jacobians: host worst", worst, "tolerance", S.numeric_jacobian_tolerance(E))
    assert worst <= S.numeric_jacobian_tolerance(E) and min(np.abs(tJc).max(), np.abs(tJm).max()) > 10


# ====================================================================================== the 50-digit references by a second route
def test_expm_agrees_with_a_second_route():
    rng = np.random.default_rng(5)
    for scale in (1e-6, 1e-2, 1.0, 3.0):
        for n in (6, 7):
            u = rng.uniform(-1, 1, n) * scale
            G = S.generator(u)
            a, b = S.MP.expm(G), S.expm_series(G)
            assert S.max_abs(a - b) <= 1e-30 * max(1.0, S.max_abs(a))
            Gd = np.array([[float(G[i, j]) for j in range(4)] for i in range(4)])
            sp = scipy.linalg.expm(Gd)
            assert max(abs(float(a[i, j]) - sp[i, j]) for i in range(4) for j in range(4)) <= 1e-13 * max(1.0, np.abs(sp).max())


# ====================================================================================== the host restatements' worst errors
def _theta_min(us):
    return min(S.theta_of(u) for u in us if S.theta_of(u) >= S.THRESH)


def test_host_errors_of_se3_exp_leave_the_floor_a_margin():
    H = B.host()
    for name, u in S.se3_exp_inputs().items():
        worst = S.se3_exp_worst(name, B.se3_exp(H, u))
        print("se3_exp", name, "host worst", worst)
        if name in ("tiny", "zero"):
            assert worst <= SE3_FLOOR / 2, name
        else:       # eps / theta in t: see the module's docstring
            scaled = max(S.err_units(g, w, S.se3_exp_unit(x)) * min(1.0, S.theta_of(x) if not S.se3_small(x) else 1.0)
                         for x, g, w in zip(u, B.se3_exp(H, u), S.se3_exp_closed(name)))
            print("   times theta", scaled)
            assert scaled <= SE3_FLOOR / 2, name


def test_host_errors_of_sim3_leave_the_floor_a_margin():
    for name, u in S.sim3_exp_inputs().items():
        got = B.sim3_exp(False, u)
        worst = S.sim3_exp_worst(name, got)
        print("sim3_exp", name, "host worst", worst)
        if name in ("small_small", "large_sigma", "large_large"):
            assert worst <= SIM3_FLOOR / 2, name
            continue

        def factor(x):
            st, ss = S.sim3_exp_branches(x)
            f = 1.0 if st else min(1.0, S.theta_of(x))                # A = (1 - cos theta) / theta^2 times Omega
            if not ss:
                f *= min(1.0, abs(x[6]))                              # C = (exp(sigma) - 1) / sigma
                if st:
                    f *= min(1.0, abs(x[6]) ** 3 / S.theta_of(x) ** 2)    # B of order sigma^-3 times Omega^2
            return f
        scaled = max(S.err_units(g, w, S.sim3_unit(x)) * factor(x) for x, g, w in zip(u, got, S.sim3_exp_closed(name)))
        print("   conditioned", scaled)
        assert scaled <= SIM3_FLOOR / 2, name
    logs = S.sim3_log_inputs(lambda u: B.sim3_exp(False, u))
    for name, s8 in logs.items():
        worst = S.sim3_log_worst(s8, B.sim3_log(False, s8))
        print("sim3_log", name, "host worst", worst)
        assert worst <= SIM3_LOG_FLOOR / 2, name


def test_svd_inputs_and_host_ratios():
    bit_rows = 0
    for shape, (M, N, N1, want_u) in S.SVD_SHAPES.items():
        assert B.SVD_SHAPES is S.SVD_SHAPES
        for cls in S.SVD_CLASSES:
            At = S.svd_inputs(shape, cls)
            assert At.shape[1:] == (N1, M) and At.dtype == np.float32 and not At[:, N:].any()
            s = np.linalg.svd(np.swapaxes(At[:, :N].astype(np.float64), 1, 2), compute_uv=False)
            if cls == "random":
                assert len(At) == S.SVD_N >= 200
                if shape in S.SVD_NULL_SHAPES:      # the condition on the null-vector users' inputs
                    assert ((s[:, -2] - s[:, -1]) >= S.MIN_GAP * s[:, 0]).all()
            if cls == "rank_deficient":
                assert (s[:, -1] <= 1e-6 * s[:, 0]).all()
            if cls == "equal_values":
                assert (np.diff(np.round(s, 6)) == 0).any(1).all()
                cols = np.linalg.norm(At[:, :N].astype(np.float64), axis=2)
                assert (np.diff(cols[0]) > 0).any()                      # given out of order
            if cls == "denormal":
                assert (np.abs(At[At != 0]) < np.finfo(np.float32).tiny).all() and At.any()
                continue
            W, Vt, out = B.svd(False, shape, At)
            r = S.svd_measures(shape, At, W, Vt, out, False)
            print("svd", shape, cls, {k: round(r[k], 2) for k in S.SVD_RATIOS})
            assert r["descending"] and all(r[k] <= S.SVD_FLOOR / 2 for k in S.SVD_RATIOS), (shape, cls, r)
            if cls == "zero":
                assert r["u"] < 1
            if cls in ("three_i", "equal_values", "zero"):      # the sort's strict '<', stated without the restatement
                eW, eVt = S.svd_unrotated_expected(shape, cls)
                assert S.bits(W).tolist() == S.bits(eW).tolist() and S.bits(Vt).tolist() == S.bits(eVt).tolist(), (shape, cls)
                if cls == "equal_values":
                    assert not np.array_equal(eVt[0], np.eye(N)) and np.array_equal(eVt[1], np.eye(N))
            bit_rows += len(At)
    assert bit_rows > 1000


# ====================================================================================== the fronts
@pytest.mark.parametrize("shape", S.FRONT_SHAPES, ids=str)
def test_front_cases(shape):
    """the exact class is exact: the sequential loop, run on doubles, gives L, the Schur complement and r themselves, and so does
    the 50-digit factorisation; the failing cases fail where they say"""
    n, k = S.front_dims(shape)
    c = S.front_exact(shape)
    wantF, wantr = S.front_exact_expected(shape)
    for s in range(len(c["M"])):
        F, r, ok = S.front_sequential(c["M"][s], k, c["r"][s])
        assert ok and np.array_equal(np.tril(F), wantF[s]) and np.array_equal(r, wantr[s]), s
    if n <= 56:
        Fm, rm = S.front_mp(c["M"][0], k, c["r"][0])
        assert all(Fm[i][j] == S.MP.mpf(float(wantF[0][i, j])) for i in range(n) for j in range(i + 1)) and all(rm[i] == S.MP.mpf(float(wantr[0][i])) for i in range(n))
    if shape in S.FRONT_FAIL_SHAPES:
        cases = S.front_failing(shape)
        assert len(cases) == 12 and {c[1] for c in cases} == {0, k // 2, k - 1}
        for name, col, M, r in cases:
            F, rr, ok = S.front_sequential(M, k, r)
            d = F[col, col]
            assert not ok and (not d > 0 or not np.isfinite(d)) and all(np.isfinite(F[j, j]) and F[j, j] > 0 for j in range(col)), name
    if shape[1] > 0:
        b = S.front_back_cases(shape, False)
        for s in range(len(b["F"])):
            assert np.array_equal(S.back_sequential(b["F"][s], b["r"][s], b["xb"][s], k), b["x_own"][s]), s
            assert len(set(b["vtx"][s].tolist())) == shape[1] + shape[2]
        assert any(not np.array_equal(v, np.arange(shape[1] + shape[2])) for v in b["vtx"])      # scattered


def test_front_shapes_straddle_the_strides():
    ns = sorted(S.front_dims(s)[0] for s in S.FRONT_SHAPES)
    assert ns == [6, 12, 14, 14, 18, 18, 56, 168, 280] and 0 in [S.front_dims(s)[1] for s in S.FRONT_SHAPES]
    assert min(ns) < 16 < max(ns) and any(16 < n < 32 for n in ns) and max(ns) > 256
    assert S.FRONT_PACKED_MAX * (S.FRONT_PACKED_MAX + 1) // 2 * 8 <= 160 * 1024 - 1024 < 280 * 281 // 2 * 8


@pytest.mark.parametrize("shape", S.FRONT_ROUNDED_SHAPES, ids=str)
def test_front_rounded_cases_and_numpy_errors(shape):
    """kappa within 1e8; the order matters; numpy's cholesky and solves, measured against the 50-digit factorisation, leave the floor of
    4 eps kappa a margin of 2"""
    n, k = S.front_dims(shape)
    c = S.front_rounded(shape)
    assert c["kappa"].max() <= S.KAPPA_MAX * 1.01 and c["kappa"].min() >= 50 and c["kappa"].max() >= 1e7
    differ = 0
    worst = 0.0
    systems, schur_rows = S.front_mp_plan(shape)
    assert len(systems) >= 2 and (schur_rows is None or (len(schur_rows) >= 14 and {(i - k) % 16 for i in schur_rows} == set(range(16))))
    for s in systems:
        Fs, rs, ok = S.front_sequential(c["M"][s], k, c["r"][s])
        Fl, rl = S.front_left_looking(c["M"][s], k, c["r"][s])
        assert ok
        differ += not (S.same_bits(np.tril(Fs), np.tril(Fl)) and S.same_bits(rs, rl))
        Fm, rm = S.front_mp(c["M"][s], k, c["r"][s], schur_rows)
        want = S.front_parts(np.array(Fm, object), np.array(rm, object), k)
        ref, seq = S.front_parts(*S.front_numpy(c["M"][s], k, c["r"][s]), k), S.front_parts(Fs, rs, k)
        for part in want:
            worst = max(worst, S.front_ratio(ref[part], want[part], c["kappa"][s]), S.front_ratio(seq[part], want[part], c["kappa"][s]))
    print("front", shape, "numpy and sequential worst", worst)
    assert worst <= S.FRONT_FLOOR / 2
    if k > 0:
        assert differ > len(systems) / 2
        b = S.front_back_cases(shape, True)
        d = sum(not S.same_bits(S.back_sequential(b["F"][s], b["r"][s], b["xb"][s], k), S.back_row_wise(b["F"][s], b["r"][s], b["xb"][s], k))
                for s in range(len(b["F"])))
        assert d > len(b["F"]) / 2
        for s in range(len(b["F"])):
            want = S.back_mp(b["F"][s], b["r"][s], b["xb"][s], k)
            assert S.front_ratio(S.back_numpy(b["F"][s], b["r"][s], b["xb"][s], k), want, c["kappa"][s]) <= S.FRONT_FLOOR / 2


# ====================================================================================== the probe builds
def test_probe_cross_compiles_for_gfx950():
    so = B.compile_probe(os.path.join(tempfile.mkdtemp(prefix="solver_units_cc_"), "solver_units_probe.so"))
    assert os.path.getsize(so) > 0
    # every call the wrappers declare is exported (the library's flags hide what is not marked)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).split()
    assert not [name for name in list(B._SE3) + list(B._DEVICE) + list(B._PASSES) if name not in exported]


# ====================================================================================== the steps the passes share
def test_damped_inverse_cases_and_the_restatement():
    """the classes and their count; D (H + lambda I) = I within the bound the condition number gives; one cofactor's sign is far outside"""
    H6, lam, cls = S.dinv_inputs()
    assert len(H6) == S.DINV_N == 65 and cls.count("identity") == 1 and min(cls.count(c) for c in ("two", "six", "single")) >= 20
    M = S.dinv_full(H6, lam)
    D = B.dinv3(B.host(), H6, lam)
    assert np.array_equal(D[0], np.eye(3)) and np.array_equal(D, np.swapaxes(D, 1, 2))
    worst, kmax = 0.0, {}
    for i in range(len(M)):
        bound, k = S.dinv_bound(M[i])
        kmax[cls[i]] = max(kmax.get(cls[i], 0), k)
        err = np.abs(D[i] @ M[i] - np.eye(3)).max()
        worst = max(worst, err / bound)
        assert err <= bound, (i, cls[i], err, bound)
        if cls[i] == "single":           # rank 2 plus lambda: the plain J^T J is singular to rounding
            s = np.linalg.svd(M[i] - lam[i] * np.eye(3), compute_uv=False)
            assert s[2] <= 1e-12 * s[0]
            flipped = D[i].copy()
            flipped[0, 1] = flipped[1, 0] = -D[i][0, 1]
            assert np.abs(flipped @ M[i] - np.eye(3)).max() > 1e3 * bound
    print("damped inverse: worst |D M - I| / bound", worst, "largest condition number per class", kmax)
    assert kmax["single"] > 1e3


@pytest.mark.parametrize("nitems,diag", S.PAIR_CASES)
def test_pair_item_cases_and_the_restatement(nitems, diag):
    Wi, Wj, Dm, bl, acc0, accb0 = S.pair_inputs(nitems, diag)
    assert np.abs(acc0).min() > 0 and np.abs(accb0).min() > 0
    acc, accb = B.pair_items(B.host(), Wi, Wj, Dm, bl, diag, acc0, accb0)
    want = acc0 + np.einsum("siab,sibc,sidc->sad", Wi, Dm, Wj)
    wantb = accb0 + (np.einsum("siab,sibc,sic->sa", Wi, Dm, bl) if diag else 0)
    tol = 64 * S.EPS * max(1.0, np.abs(want).max())
    assert np.abs(acc - want).max() <= tol and np.abs(accb - wantb).max() <= tol
    if not diag:
        assert S.same_bits(accb, accb0)
    if nitems:           # W_i for W_j, and an assignment for the addition, are far outside
        assert np.abs(B.pair_items(B.host(), Wj, Wi, Dm, bl, diag, acc0, accb0)[0] - want).max() > 1e-3
        assert np.abs(acc - acc0 - want).max() > 1e-3


@pytest.mark.parametrize("R", (6, 7))
def test_merge_cases_and_the_restatement(R):
    """the sequential restatement is the dense scatter, bit for bit; the children's order and the swap show"""
    desc, cmap, fronts = S.merge_case(R)
    n = 3 * R
    for node in (0, 3):
        got = B.merge(B.host(), R, desc, cmap, fronts, node)
        assert S.same_bits(got, S.merge_dense(R, desc, cmap, fronts, node)), node
        F0, F1 = fronts[desc[node][0]:][:n * n].reshape(n, n), got[desc[node][0]:][:n * n].reshape(n, n)
        other = np.ones(len(fronts), bool)
        other[desc[node][0]:desc[node][0] + n * n + n] = False
        assert S.same_bits(got[other], fronts[other]) and S.same_bits(np.triu(F1, 1), np.triu(F0, 1))       # nothing else is written
        changed = S.bits(F1) != S.bits(F0)
        if node == 0:
            # left: the parent's vertices 2 and 0 with their cross block at (2, 0); right: vertex 0; vertex 1 receives nothing
            want = np.zeros((3, 3), bool)
            want[0, 0] = want[2, 2] = want[2, 0] = True
            assert np.array_equal(changed.reshape(3, R, 3, R).any((1, 3)), want)
            assert changed[2 * R:, :R].all()            # the cross block whole: its upper half came through the swap
            swapped = S.merge_dense(R, desc, cmap, fronts, node, order=(1, 0))
            d = S.bits(swapped) != S.bits(got)
            assert d.any() and not d[other].any()
            blk = d[desc[0][0]:][:n * n].reshape(n, n)
            assert blk[:R, :R].any() and not blk[R:].any()       # only where both children add
        else:
            assert np.array_equal(changed.reshape(3, R, 3, R).any((1, 3)), np.diag([True, False, False]))


@pytest.mark.parametrize("n", S.RUN_SUM_SIZES)
def test_run_sum_cases_and_the_restatement(n):
    v = S.run_sum_inputs(n)
    got = B.run_sum(B.host(), v)
    assert B.host().se3.su_lm_threads() == S.RUN_SUM_THREADS
    assert abs(got - math.fsum(v)) <= max(n, 1) * S.EPS * np.abs(v).sum()
    if n <= 1:
        assert got == (v[0] if n else 0.0)
    if n > S.RUN_SUM_THREADS:          # the order shows: a strided assignment, and one sum from the left, give other bits
        assert got != S.run_sum_strided(v)
    if n == max(S.RUN_SUM_SIZES):
        assert got != float(np.add.reduce(v)) or got != sum(v.tolist())
        assert np.log10(np.abs(v).max() / np.abs(v).min()) > 10
