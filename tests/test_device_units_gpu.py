"""Unit tests of the device helpers that several kernels share, on the GPU against plain references:

  A  include/orbfe_math.h     the device compile equals the host compile (g++ -ffp-contract=off) bit for bit
  B  csrc/wave_dpp.hpp        the DPP scans and reductions equal numpy on rows of 64 lanes
  C  csrc/lm_dense.hpp        quaternions, projection error, Huber, the pivoted LDLT, the fixed-order workgroup sum
  D  csrc/ransac_sets.hpp     decode_set's sparse draw equals the reference's list draw
  E  csrc/sim3_points.hpp     rigid

The helpers run inside tests/device_units_probe.hip: the five headers, included unchanged, as a translation unit of their own that
tests/device_units_build.py compiles with the library's flags.  That is not the instantiations inside the product kernels: the
end-to-end tests of the extractor, matcher, optimizers and solvers remain the check of those.  The inputs and references are in
tests/device_units_cases.py; tests/test_device_units_cpu.py checks on the CPU that they are what these tests need."""
import numpy as np
import pytest

import device_units_build as B
import device_units_cases as K

pytestmark = pytest.mark.gpu

bits = K.bits


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


def where_differ(got, want, *inputs):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    return len(bad), [(tuple(np.asarray(a).ravel()[bad[0]] for a in inputs), got.ravel()[bad[0]], want.ravel()[bad[0]])] if len(bad) else []


def test_probe_sees_a_gpu():
    assert B.probe().du_device_count() >= 1


# ====================================================================================== A. numerics contract: device == host, bit for bit
# No tolerance and no exceptions.  orbfe_fast_atan2's frame inputs are integers (image moments); the sets scaled by 2^-100 and 2^-140
# (denormal) agree as well: the library's flags do not flush float denormals on gfx950.  With contraction left on in the probe's
# flags the atan2 sets differ, so these tests do see the flags.
@pytest.mark.parametrize("name", sorted(K.atan2_sets()))
def test_fast_atan2_device_equals_host(name):
    y, x = K.atan2_sets()[name]
    got, want = B.atan2(B.probe(), y, x), B.atan2(B.host(), y, x)
    assert same_bits(got, want), where_differ(got, want, y, x)


@pytest.mark.parametrize("name", sorted(K.sincos_sets()))
def test_sincosf_device_equals_host(name):
    a = K.sincos_sets()[name]
    (gs, gc), (ws, wc) = B.sincos(B.probe(), a), B.sincos(B.host(), a)
    assert same_bits(gs, ws), where_differ(gs, ws, a)
    assert same_bits(gc, wc), where_differ(gc, wc, a)


@pytest.mark.parametrize("name", sorted(K.round_sets()))
def test_rounding_helpers_device_equals_host(name):
    v = K.round_sets()[name]
    for fn, got, want in zip(("round_d", "round_f", "floor_d", "ceil_d"), B.rounders(B.probe(), v), B.rounders(B.host(), v)):
        assert np.array_equal(got, want), (fn, where_differ(got, want, v))


@pytest.mark.parametrize("ndist", K.NDIST)
def test_undistort_point_device_equals_host(ndist):
    uv, cam, k12 = K.undistort_grid(), K.TUM1_K.astype(np.float64), K.undistort_k12(ndist)
    got, want = B.undistort(B.probe(), uv, cam, k12), B.undistort(B.host(), uv, cam, k12)
    assert same_bits(got, want), where_differ(got, want, np.repeat(uv[:, 0], 2), np.repeat(uv[:, 1], 2))


# ====================================================================================== B. wave_dpp.hpp
def test_wave_scans_equal_cumsum():
    rows = K.wave_rows_i32(True)
    got = B.wave_i32(B.SCAN, rows)
    want = np.cumsum(rows, axis=1, dtype=np.int32)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))
    got = B.wave_i32(B.ROW16, rows)
    assert np.array_equal(got, K.cumsum16(rows)), np.flatnonzero((got != K.cumsum16(rows)).any(1))


@pytest.mark.parametrize("op,sums,ref", [(B.SUM, True, lambda r: np.sum(r, axis=1, dtype=np.int32)), (B.MAX, False, lambda r: r.max(1)),
                                         (B.MIN, False, lambda r: r.min(1))], ids=["sum", "max", "min"])
def test_wave_reductions_are_uniform_and_equal_numpy(op, sums, ref):
    rows = K.wave_rows_i32(sums)
    got = B.wave_i32(op, rows)
    assert (got == got[:, :1]).all(), "not the same in all 64 lanes: rows %s" % np.flatnonzero((got != got[:, :1]).any(1))
    assert np.array_equal(got[:, 0], ref(rows)), np.flatnonzero(got[:, 0] != ref(rows))


@pytest.mark.parametrize("name", sorted(K.wave_rows_u64()))
def test_wave_max_min_u64(name):
    rows = K.wave_rows_u64()[name]
    for op, want in ((B.U_MAX, rows.max(1)), (B.U_MIN, rows.min(1))):
        got = B.wave_u64(op, rows)
        assert (got == got[:, :1]).all(), (op, np.flatnonzero((got != got[:, :1]).any(1)))
        assert np.array_equal(got[:, 0], want), (op, np.flatnonzero(got[:, 0] != want))


def test_second_minimum_after_masking_the_first():
    """k_knn2_csr's pattern: m1 = wave_min_u64(key), k2 = wave_min_u64(key == m1 ? ~0 : key) on rows with a duplicated minimum"""
    rows, best, second = K.knn_key_rows()
    m1, k2 = B.wave_u64(B.U_MIN2, rows)
    assert (m1 == m1[:, :1]).all() and (k2 == k2[:, :1]).all()
    assert np.array_equal(m1[:, 0], best), np.flatnonzero(m1[:, 0] != best)
    assert np.array_equal(k2[:, 0], second), np.flatnonzero(k2[:, 0] != second)


@pytest.mark.parametrize("name", sorted(K.wave_rows_f64()))
def test_wave_sum_f64_exact_on_integers(name):
    rows = K.wave_rows_f64()[name]
    got = B.wave_f64(rows)
    assert (bits(got) == bits(got)[:, :1]).all()
    assert same_bits(got[:, 0], rows.sum(1)), np.flatnonzero(got[:, 0] != rows.sum(1))


# ====================================================================================== C. lm_dense.hpp
def test_quat_from_matrix_every_branch():
    R = K.quat_matrices()
    taken = [K.quat_branch(m) for m in R]
    assert all(taken.count(b) >= 2 for b in (-1, 0, 1, 2)), taken
    q, rot = B.quat(R)
    want = np.stack([K.quat_ref(m) for m in R])
    err = np.abs(q - want)
    assert err.max() <= 4 * np.finfo(np.float64).eps, (err.max() / np.finfo(np.float64).eps, int(err.max(1).argmax()))
    assert np.abs(rot - R).max() <= 1e-15, (np.abs(rot - R).max(), int(np.abs(rot - R).reshape(len(R), -1).max(1).argmax()))


def test_rotate_qmul_project_chi2_bit_equal():
    d = K.dense_inputs()
    got = B.rotate(d["qa"], d["v"])
    assert same_bits(got, K.rotate_ref(d["qa"], d["v"])), where_differ(got, K.rotate_ref(d["qa"], d["v"]))
    got = B.qmul(d["qa"], d["qb"])
    assert same_bits(got, K.qmul_ref(d["qa"], d["qb"])), where_differ(got, K.qmul_ref(d["qa"], d["qb"]))
    err, chi2 = B.project(d["Xc"], d["obs"], d["cam"], d["info"])
    werr, wchi2 = K.project_ref(d["Xc"], d["obs"], d["cam"], d["info"])
    assert same_bits(err, werr), where_differ(err, werr)
    assert same_bits(chi2, wchi2), where_differ(chi2, wchi2)


def test_huber_both_branches_and_the_equality_case():
    chi2, delta, quad = K.huber_inputs()
    rho = B.huber(chi2, delta)
    w0, w1 = K.huber_ref(chi2, delta)
    assert same_bits(rho[:, 0], w0) and same_bits(rho[:, 1], w1), (rho, w0, w1)
    at = chi2 == delta * delta
    # chi2 == delta^2: the quadratic branch's values
    assert at.sum() == 2 and (rho[at, 0] == chi2[at]).all() and (rho[at, 1] == 1.0).all()
    assert (rho[quad, 1] == 1.0).all() and (rho[chi2 > 1.01 * delta * delta, 1] < 1.0).all()


@pytest.mark.parametrize("N", [6, 7])
def test_ldlt_solve(N):
    """ldlt_solve<N> on 200 systems H = P L D L^T P^T per N whose entries are dyadic, so that H is an exact double, its inertia is known
    and the exact solution comes from rational elimination.  Verdicts and the untouched / zero entries of x are exact; the solution's
    error r = |x - x*|_inf / (eps kappa_inf |x*|_inf) may reach 4 x the worst r of numpy.linalg.solve over the same systems, at least 4.

    The margin is for another elimination order (LAPACK's LU with row pivoting against the LDLT with diagonal pivoting), which moves
    roundings by a small factor, not by an order of magnitude.

    Measured: numpy.linalg.solve worst r = 0.084 (N = 6) and 0.104 (N = 7), so the bound is 4 for both; the device's worst r on an
    MI355X = 0.090 (N = 6) and 0.063 (N = 7).  The test prints both."""
    cases = K.ldlt_systems(N)
    a = [c for c in cases if c["cls"] == "a"]
    assert 3 * sum(c["first_pivot"] != 0 for c in a) >= len(a)
    ok, x = B.ldlt(np.stack([c["H"] for c in cases]), np.stack([c["b"] for c in cases]), K.SENTINEL)
    bound = max(4.0, 4.0 * K.ldlt_numpy_worst(N))
    worst = 0.0
    for i, c in enumerate(cases):
        assert bool(ok[i]) == c["ok"], (i, c["cls"], ok[i])
        if not c["ok"]:
            assert (x[i] == K.SENTINEL).all(), (i, c["cls"], x[i])
            continue
        zero = np.setdiff1d(np.arange(N), c["keep"])
        assert (x[i][zero] == 0).all(), (i, c["cls"], x[i])
        if len(c["keep"]):
            r = K.ldlt_ratio(c, x[i])
            worst = max(worst, r)
            assert r <= bound, (i, c["cls"], r, bound, x[i], c["x"])
            if c["cls"] == "f":
                assert np.array_equal(x[i], c["x"]), (i, x[i], c["x"])
    print("ldlt_solve<%d>: worst r of numpy.linalg.solve %.3f, of the device %.3f, bound %.3f" % (N, K.ldlt_numpy_worst(N), worst, bound))


@pytest.mark.parametrize("N", [2, 7])
def test_block_sum_in_the_documented_order(N):
    v = K.block_sum_inputs(N)
    want = np.stack([K.block_sum_ref(b) for b in v])
    plain = np.stack([K.left_to_right(b) for b in v])
    assert (bits(want) != bits(plain)).mean() > 0.5            # the order matters on these inputs, else equality would prove nothing
    got = B.block_sum(v)
    assert same_bits(got, want), where_differ(got, want)


def test_block_count():
    c = K.block_count_inputs()
    assert sorted(set(c.sum(1))) == [0, 1, 255, 256]
    assert np.array_equal(B.block_count(c), c.sum(1))


# ====================================================================================== D. ransac_sets.hpp
@pytest.mark.parametrize("Kset", [8, 3])
def test_decode_set_equals_the_reference_draw(Kset):
    for N in K.set_sizes(Kset):
        words, want = K.set_words(Kset, N), K.set_expected(Kset, N)
        for name in words:
            got = B.decode(Kset, N, words[name])
            assert np.array_equal(got, want[name]), (N, name, np.flatnonzero((got != want[name]).any(1))[:5])
            s = np.sort(got, 1)
            assert (s[:, 0] >= 0).all() and (s[:, -1] < N).all() and (np.diff(s, axis=1) > 0).all(), (N, name)


def test_clampn():
    n, cap = K.clampn_inputs()
    assert np.array_equal(B.clampn(n, cap), np.clip(n.astype(np.int64), 0, cap.astype(np.int64)).astype(np.int32))


# ====================================================================================== E. sim3_points.hpp
def test_rigid_bit_equal_to_double_sums_rounded_once():
    T, p = K.rigid_inputs()
    want = K.rigid_ref(T, p)
    assert (bits(want) != bits(K.rigid_float_only(T, p))).any()      # a float-only evaluation would be told apart
    got = B.rigid(T, p)
    assert same_bits(got, want), where_differ(got, want)
