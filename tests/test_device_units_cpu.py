"""The CPU side of tests/test_device_units_gpu.py: the host compile of include/orbfe_math.h against float64 libm on exactly the GPU
test's input sets, the plain references against second statements of the same rule, the conditions the case builders of
tests/device_units_cases.py promise (so that a later edit cannot hollow the GPU tests out), the probe's cross-compile for gfx950
with the library's flags, and the host file under the sanitizers as a program of its own."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import device_units_build as B
import device_units_cases as K

bits = K.bits


# ---------------------------------------------------------------------------------------------------- orbfe_math.h, host compile
def test_fast_atan2_host_within_0_02_degrees_of_atan2():
    """On the integer sets (the frame path's domain: image moments) within 0.02 degrees of atan2, the bound of tests/test_oracle_cpu.py;
    measured worst 0.0096 over the 461 121 pairs.  The signed-zero and scaled sets cannot be held to atan2: the eps in the divisor
    (OpenCV's, 2.2e-16) swamps operands of 2^-100, and -0.0 counts as not negative; there the result only has to stay in [0, 360]."""
    sets = K.atan2_sets()
    assert len(sets["grid"][0]) == 261121 and len(sets["moments"][0]) == 200000
    worst = 0.0
    for name, (y, x) in sets.items():
        a = B.atan2(B.host(), y, x)
        assert ((a >= 0) & (a <= 360)).all(), name
        if name in ("grid", "moments"):
            d = np.abs(a.astype(np.float64) - np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360.0)
            d = np.minimum(d, 360 - d)
            worst = max(worst, d.max())
            assert d.max() < 0.02, (name, d.max(), y[d.argmax()], x[d.argmax()])
    print("worst fastAtan2 error %.4f degrees" % worst)
    g = dict(zip(zip(*[v.tolist() for v in sets["grid"]]), B.atan2(B.host(), *sets["grid"]).tolist()))
    assert g[(0, 0)] == 0 and g[(0, 5)] == 0 and g[(5, 0)] == 90 and g[(0, -5)] == 180 and g[(-5, 0)] == 270


def test_sincosf_host_equals_rounded_double_libm():
    sets = K.sincos_sets()
    assert [len(sets[k]) for k in ("sweep", "quadrant_flips", "uniform")] == [26278, 153612, 300000]
    for name, a in sets.items():
        s, c = B.sincos(B.host(), a)
        ws, wc = np.sin(a.astype(np.float64)).astype(np.float32), np.cos(a.astype(np.float64)).astype(np.float32)
        assert np.array_equal(bits(s), bits(ws)) and np.array_equal(bits(c), bits(wc)), (name, int((s != ws).sum()), int((c != wc).sum()))
    # the flip set does straddle the points where the quadrant index changes
    f = sets["quadrant_flips"].astype(np.float64)
    n = np.rint(f * (2 / math.pi))
    assert len(np.unique(n)) >= 12801 and (np.diff(n[:9 * 12801].reshape(-1, 9), axis=1) >= 0).all()
    half = n[9 * 12801:].reshape(-1, 3)
    assert (half[:, 0] != half[:, 2]).mean() > 0.9


def test_rounding_helpers_host_against_python():
    for name, v in K.round_sets().items():
        rd, rf, fl, ce = B.rounders(B.host(), v)
        for i, x in enumerate(v.tolist()):
            assert rd[i] == round(x) and fl[i] == math.floor(x) and ce[i] == math.ceil(x), (name, x)
            assert rf[i] == round(float(np.float32(x))), (name, x)
    h = K.round_sets()["halves"]
    assert (h[1::3] % 1 == 0.5).all() and (h[0::3] < h[1::3]).all() and (h[1::3] < h[2::3]).all() and len(h) == 3 * 2047


def test_undistort_inputs_and_identity_without_distortion():
    import match_batch_cases as mc
    assert np.array_equal(K.TUM1_K, mc.TUM1_K) and np.array_equal(K.TUM1_DIST, mc.TUM1_DIST)
    assert np.array_equal(K.DIST12[:8], np.concatenate([mc.TUM1_DIST, [0.01, -0.02, 0.005]]).astype(np.float32))
    uv = K.undistort_grid()
    assert len(uv) == 33 * 25 and uv.min(0).tolist() == [-40, -40] and uv.max(0).tolist() == [679, 519]
    cam = K.TUM1_K.astype(np.float64)
    assert np.abs(B.undistort(B.host(), uv, cam, K.undistort_k12(0)) - uv).max() < 1e-4
    outs = [B.undistort(B.host(), uv, cam, K.undistort_k12(n)) for n in K.NDIST]
    assert all(np.isfinite(o).all() for o in outs)
    assert all((bits(a) != bits(b)).any() for a, b in zip(outs, outs[1:]))       # every added coefficient group changes the result


# ---------------------------------------------------------------------------------------------------- wave rows
def test_wave_rows_hold_the_patterns():
    for sums in (True, False):
        r = K.wave_rows_i32(sums)
        assert r.shape == (332, 64) and np.array_equal(r[:64], np.eye(64)) and np.array_equal(r[64:128], -np.eye(64))
        assert (r[128] == K.INT_MIN).all() and (r[129] == K.INT_MAX).all() and set(r[130]) == {K.INT_MIN, K.INT_MAX} and r[130, 0] != r[131, 0]
    assert np.abs(K.wave_rows_i32(True)[132:].astype(np.int64)).max() <= 2 ** 24
    assert np.abs(K.wave_rows_i32(False)[132:].astype(np.int64)).max() > 2 ** 30
    u = K.wave_rows_u64()
    hi, lo = u["high_word_only"] >> np.uint64(32), u["high_word_only"] & np.uint64(0xffffffff)
    assert (lo == lo[:, :1]).all() and (np.ptp(hi, axis=1) > 0).all()
    hi, lo = u["low_word_only"] >> np.uint64(32), u["low_word_only"] & np.uint64(0xffffffff)
    assert (hi == hi[:, :1]).all() and (np.ptp(lo, axis=1) > 0).all()
    assert np.array_equal(u["max_in_lane_i"].argmax(1), np.arange(64)) and np.array_equal(u["min_in_lane_i"].argmin(1), np.arange(64))
    assert ((u["zero_and_ones"] == 0).any(1)[:64]).all() and ((u["zero_and_ones"] == 2 ** 64 - 1).any(1)[:64]).all()
    rows, best, second = K.knn_key_rows()
    assert ((best >> np.uint64(32)) == (second >> np.uint64(32))).all() and (best < second).all()      # a duplicated minimum
    s = np.sort(rows, 1)
    assert np.array_equal(s[:, 0], best) and np.array_equal(s[:, 1], second)
    f = K.wave_rows_f64()
    assert all((v == np.rint(v)).all() and np.abs(v).sum(1).max() < 2.0 ** 53 for v in f.values())
    assert (f["integers"] < 0).any() and (f["integers"] > 0).any() and f["one_hot_2^52+1"].max() == 2.0 ** 52 + 1


# ---------------------------------------------------------------------------------------------------- lm_dense cases
def test_quat_cases_take_every_branch_and_the_reference_is_a_rotation():
    R = K.quat_matrices()
    assert len(R) == len(K.QUAT_AXES) * len(K.QUAT_ANGLES) + 1
    taken = [K.quat_branch(m) for m in R]
    assert all(taken.count(b) >= 2 for b in (-1, 0, 1, 2)), taken
    tie = R[-1]
    assert tie[0, 0] == tie[1, 1] > tie[2, 2] and np.trace(tie) <= 0 and K.quat_branch(tie) == 0
    qt = K.quat_ref(tie)
    assert qt[0] > 0 > qt[1] and abs(qt[0] + qt[1]) < 1e-15         # '>=' in the branch choice would return -q here
    for m, b in zip(R, taken):
        q = K.quat_ref(m)
        assert abs(np.linalg.norm(q) - 1) < 1e-15 and np.abs(K.quat_to_matrix(q) - m).max() < 1e-15
        if b >= 0:
            assert 4 * q[b] ** 2 >= 1 - 1e-15        # the square root's argument: no cancellation


def test_dense_references_agree_with_matrix_forms():
    d = K.dense_inputs()
    R = np.stack([K.quat_to_matrix(q) for q in d["qa"]])
    assert np.abs(K.rotate_ref(d["qa"], d["v"]) - np.einsum("nij,nj->ni", R, d["v"])).max() < 1e-13
    qb = d["qb"] / np.linalg.norm(d["qb"], axis=1, keepdims=True)
    Rb = np.stack([K.quat_to_matrix(q) for q in qb])
    Rab = np.stack([K.quat_to_matrix(q) for q in K.qmul_ref(d["qa"], qb)])
    assert np.abs(Rab - R @ Rb).max() < 1e-14
    e, chi2 = K.project_ref(d["Xc"], d["obs"], d["cam"], d["info"])
    assert np.abs(chi2 - d["info"] * (e ** 2).sum(1)).max() < 1e-9 and 0.1 < np.abs(e).mean() < 10


def test_huber_cases():
    chi2, delta, quad = K.huber_inputs()
    assert set(delta) == set(K.HUBER_DELTAS) and (chi2 == delta * delta).sum() == 2
    assert K.HUBER_DELTAS == (math.sqrt(5.991), math.sqrt(7.815))
    for d in K.HUBER_DELTAS:          # at equality the two branches give the same bits, so the values are what the GPU test can hold
        assert K.huber_linear(d * d, d) == (d * d, 1.0)
    assert np.array_equal(chi2 <= delta * delta, quad) and quad.sum() >= 6 and (~quad).sum() >= 6
    r0, r1 = K.huber_ref(chi2, delta)
    assert np.array_equal(r0[quad], chi2[quad]) and (r1[quad] == 1).all()
    above = ~quad
    assert (r0[above] <= chi2[above] * (1 + 1e-15)).all() and (r0[above][1::5] < chi2[above][1::5]).all() and (r0[above] > delta[above] ** 2 * (1 - 1e-15)).all() and (r1[above] <= 1).all()


@pytest.mark.parametrize("N", [6, 7])
def test_ldlt_cases(N):
    cases = K.ldlt_systems(N)
    assert len(cases) == 200 and {c["cls"]: sum(d["cls"] == c["cls"] for d in cases) for c in cases} == K.LDLT_CLASSES
    eig = {c: [np.linalg.eigvalsh(d["H"]) for d in cases if d["cls"] == c] for c in K.LDLT_CLASSES}
    assert all((e > 0).all() for e in eig["a"] + eig["f"])
    assert all((e < 0).sum() == 1 and (e > 0).sum() == N - 1 for e in eig["b"]) and all((e < 0).all() for e in eig["c"])
    assert all((d["H"] == 0).all() and d["b"].any() for d in cases if d["cls"] == "d")
    for d in cases:
        assert np.array_equal(d["H"], d["H"].T) and d["ok"] == (d["cls"] not in "bc")
        if d["ok"] and len(d["keep"]):
            assert 1 <= d["kappa"] <= K.KAPPA_MAX and np.abs(d["H"] @ d["x"] - d["b"])[d["keep"]].max() < 1e-9 * max(1, d["kappa"])
        if d["cls"] == "e":
            zero = np.setdiff1d(np.arange(N), d["keep"])
            assert len(zero) == N - 5 and (d["H"][zero] == 0).all() and (d["H"][:, zero] == 0).all() and (d["b"][zero] != 0).all()
            assert (np.linalg.eigvalsh(d["H"][np.ix_(d["keep"], d["keep"])]) > 0).all()
        if d["cls"] == "f":
            dg = np.diag(d["H"])
            assert np.array_equal(d["H"], np.diag(dg)) and len(set(dg)) == N and np.array_equal(d["x"], d["b"] / dg)
    a = [c for c in cases if c["cls"] == "a"]
    assert 3 * sum(c["first_pivot"] != 0 for c in a) >= len(a)
    assert any(np.array_equal(np.argsort(-np.diag(c["H"])), np.arange(N)) for c in cases if c["cls"] == "f")        # descending: no swap
    assert any(np.array_equal(np.argsort(np.diag(c["H"])), np.arange(N)) for c in cases if c["cls"] == "f")         # ascending
    # the reference solver's own error in the test's measure: the GPU test allows 4 x this, at least 4
    worst = K.ldlt_numpy_worst(N)
    print("numpy.linalg.solve worst r, N = %d: %.3f" % (N, worst))
    assert 0 < worst < 4


@pytest.mark.parametrize("N", [2, 7])
def test_block_sum_cases_are_order_sensitive(N):
    v = K.block_sum_inputs(N)
    want = np.stack([K.block_sum_ref(b) for b in v])
    plain = np.stack([K.left_to_right(b) for b in v])
    assert (bits(want) != bits(plain)).mean() > 0.5
    e = np.frexp(np.abs(v))[1]
    assert e.min() <= 2 and e.max() >= 60 and (v < 0).any() and (v > 0).any()
    # the butterfly is a sum: of integers it is exact and equals any order
    ints = np.rint(v[0] / 2.0 ** 30)
    assert np.array_equal(K.block_sum_ref(ints), K.left_to_right(ints))
    c = K.block_count_inputs()
    assert sorted(set(c.sum(1))) == [0, 1, 255, 256]


# ---------------------------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("Kset", [8, 3])
def test_draw_restatement_against_the_sparse_form(Kset):
    sizes = K.set_sizes(Kset)
    assert sizes[:2] == (Kset, Kset + 1) and set(sizes) >= {9, 10, 16, 100, 2000}
    collisions = 0
    for N in sizes:
        words, want = K.set_words(Kset, N), K.set_expected(Kset, N)
        assert set(words) == {"random", "all_zero", "all_rand_max", "three_values", "one_word_repeated", "out_of_range"}
        assert sum(len(w) for n, w in words.items() if n != "out_of_range") == 3000
        assert all(w.min() >= 0 for n, w in words.items() if n != "out_of_range") and words["out_of_range"].min() == K.INT_MIN
        for name, w in words.items():
            sparse = np.array([K.draw_sparse(row, N) for row in w[::3]], np.int32)
            assert np.array_equal(sparse, want[name][::3]), (N, name)
            s = np.sort(want[name], 1)
            assert (s[:, 0] >= 0).all() and (s[:, -1] < N).all() and (np.diff(s, axis=1) > 0).all(), (N, name)
        # the collisions decode_set has to handle: the same position drawn twice, and a draw of the current last entry
        r = np.array([[K.clamp_word(int(x), N - j) for j, x in enumerate(row)] for row in words["three_values"]])
        collisions += int((r[:, 1:] == r[:, :1]).any(1).sum()) + int((r == N - 1 - np.arange(Kset)).any(1).sum())
    assert collisions > 1000


def test_draw_restatement_against_initializer_ref():
    import initializer_build
    for N in K.set_sizes(8):
        for name, w in K.set_words(8, N).items():
            if name != "out_of_range":        # the reference's loop has no clamp: rand() words only
                assert np.array_equal(initializer_build.decode_sets(N, w.ravel()), K.set_expected(8, N)[name]), (N, name)


def test_clampn_and_rigid_cases():
    n, cap = K.clampn_inputs()
    assert {-1, 0, K.INT_MIN, K.INT_MAX} <= set(n.tolist()) and ((n.astype(np.int64) == cap.astype(np.int64) + 1).sum() >= 4) and (n == cap).sum() >= 5
    T, p = K.rigid_inputs()
    assert T.shape == (1000, 12) and T.dtype == p.dtype == np.float32
    assert (bits(K.rigid_ref(T, p)) != bits(K.rigid_float_only(T, p))).any()
    assert np.abs(K.rigid_ref(T, p) - K.rigid_float_only(T, p)).max() < 1e-4


# ---------------------------------------------------------------------------------------------------- builds
def test_probe_compiles_for_gfx950_with_the_library_flags():
    import __graft_entry__ as entry
    so = os.path.join(tempfile.mkdtemp(prefix="device_units_cc_"), "device_units_probe.so")
    cmd = B.hipcc_command(so)
    extra = [f for f in os.environ.get("ORBFE_EXTRA_HIPCC_FLAGS", "").split() if f]
    assert cmd[1:-3] == entry.HIPCC_FLAGS + extra and "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd
    subprocess.check_call(cmd)
    assert os.path.getsize(so) > 0
    names = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert all(n in names for n in list(B._MATH) + list(B._DEVICE) + list(B._POSE)) and len(B._POSE) == 9
    # the probe is no part of the product library
    assert "device_units_probe.hip" not in entry.HIP_SOURCES
    lib = subprocess.check_output(["nm", "-D", "--defined-only", entry.LIB], text=True)
    assert " du_" not in lib


def test_host_file_runs_clean_under_the_sanitizers():
    exe = B.sanitizer_program()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "1681 values per call, 0 violations" in r.stdout, r.stdout
